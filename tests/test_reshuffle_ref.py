"""The blind re-shuffle argument on the host, in the reference helper alone
(tests/reshuffle_ref.py; no GPU, no library): completeness over k = 2..6 and the
edge inputs, every region of the proof bound, statements that do not hold
rejected even when a proof is forced, the proof bound to its label and to the
order of its cards, and the merged form of the first two checks."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import reshuffle_ref as rr  # noqa: E402
from oracle import bulletproofs as bp, ristretto as r255  # noqa: E402
from oracle.merlin import pedersen_gens_default  # noqa: E402

L = rr.L


def other_point(tag: bytes) -> bytes:
    return rr.rand_cards(1, b"other-" + tag)[0]


@pytest.fixture(scope="module")
def proved():
    """k -> (cards_in, perm, cards_out, proof), proved once."""
    out = {}
    for k in range(2, 7):
        cards, perm = rr.rand_cards(k, b"ref-%d" % k), rr.rand_perm(k, b"ref-%d" % k)
        co, pf = rr.prove(cards, perm, rr.seed32(b"ref-%d" % k))
        out[k] = (cards, perm, co, pf)
    return out


@pytest.mark.parametrize("k", range(2, 7))
def test_prove_then_verify(proved, k):
    cards, perm, co, pf = proved[k]
    assert len(pf) == rr.proof_len(k) and [name for name, _, _ in rr.regions(k)][-1] == "inner"
    assert sum(n for _, _, n in rr.regions(k)) == len(pf)
    assert rr.verify_parts(cards, co, pf) == (True, True)
    assert co == rr.reblind(cards, perm, rr.draws(rr.seed32(b"ref-%d" % k), k)[0])


@pytest.mark.parametrize("name", rr.EDGES)
@pytest.mark.parametrize("k", [2, 5])
def test_edge_inputs(k, name):
    """An input card equal to the identity, two equal input cards, r_0 = 0, pi
    the identity and pi the reversal."""
    cards, perm, blinds = rr.edge_case(k, name)
    co, pf = rr.prove(cards, perm, rr.seed32(b"edge-%d" % k), blinds)
    assert rr.verify(cards, co, pf)
    if name == "zero-blind":
        assert r255.equal(r255.decode(co[0]), r255.decode(cards[perm[0]]))  # (r_0 = 0: the card itself)
    if name == "pi-identity":
        assert all(co[i] != cards[i] for i in range(k))  # (still re-blinded)


@pytest.mark.parametrize("region", ["A", "E", "Ti", "T", "z", "om", "zR", "Vk", "inner"])
@pytest.mark.parametrize("k", [2, 3])
def test_each_region_is_bound(proved, k, region):
    """A point replaced by another valid point, a scalar by itself + 1: the
    first field of each of the nine regions."""
    cards, _, co, pf = proved[k]
    o = {name: off for name, off, _ in rr.regions(k)}[region]
    if region in ("z", "om", "zR"):
        new = rr.sb(int.from_bytes(pf[o:o + 32], "little") + 1)
    elif region == "inner":
        o += 8 * 32  # tau_x, the inner proof's first scalar
        new = rr.sb(int.from_bytes(pf[o:o + 32], "little") + 1)
    else:
        new = other_point(region.encode())
    bad = pf[:o] + new + pf[o + 32:]
    assert bad != pf and not rr.verify(cards, co, bad)


def test_output_that_is_no_reblinding_is_rejected(proved):
    """C'_0 + B is no re-blinding of any input: the honest prover's sigma part
    fails (check (ii)), with the inner proof intact."""
    k = 4
    cards, perm, co, _ = proved[k]
    g, _ = pedersen_gens_default()
    moved = [r255.encode(r255.ed_add(r255.decode(co[0]), g))] + co[1:]
    out, pf = rr.prove(cards, perm, rr.seed32(b"ref-%d" % k), cards_out=moved)
    assert out == moved
    assert rr.verify_parts(cards, moved, pf) == (False, True)


def test_output_that_repeats_an_input_is_rejected():
    """C'_1 built from the same C_j as C'_0: no bijection.  The honest prover
    refuses it; forced through, the inner proof fails (the pairs (pi(i), b_i)
    are no permutation of (j, e_j)), and so does check (ii)."""
    k = 4
    cards = rr.rand_cards(k, b"repeat")
    pi = [2, 2, 0, 1]
    with pytest.raises(AssertionError):
        rr.prove(cards, pi, rr.seed32(b"repeat"))
    co, pf = rr.prove(cards, pi, rr.seed32(b"repeat"), force=True)
    sigma, inner = rr.verify_parts(cards, co, pf)
    assert not inner and not sigma  # (check (ii) too: sum_i b_i C_pi(i) counts C_2 twice and C_3 never)


def test_bound_to_label_and_card_order(proved):
    k = 5
    cards, _, co, pf = proved[k]
    assert rr.verify(cards, co, pf, b"bp-perm")
    assert not rr.verify(cards, co, pf, b"another label")
    swapped_in = [cards[1], cards[0]] + cards[2:]
    swapped_out = [co[1], co[0]] + co[2:]
    assert not rr.verify(swapped_in, co, pf)
    assert not rr.verify(cards, swapped_out, pf)
    assert rr.verify_parts(cards, co, pf[:-1]) == (False, False)  # a short proof


def test_noncanonical_scalar_and_bad_point_are_rejected(proved):
    k = 3
    cards, _, co, pf = proved[k]
    o = {name: off for name, off, _ in rr.regions(k)}
    assert not rr.verify(cards, co, pf[:o["z"]] + rr.L.to_bytes(32, "little") + pf[o["z"] + 32:])
    undecodable = b"\xff" * 32
    assert not rr.verify(cards, co, pf[:o["E"]] + undecodable + pf[o["E"] + 32:])
    assert not rr.verify(cards, [undecodable] + co[1:], pf)


@pytest.mark.parametrize("k", [2, 4, 6])
def test_merged_terms_sum_to_the_identity(proved, k):
    cards, _, co, pf = proved[k]
    P = rr.Parsed(cards, co, pf, b"bp-perm")
    rho = rr.batch_weight(rr.seed32(b"verifier"), 7, P.c)
    sc, pts = rr.merged_terms(P, rho)
    assert len(sc) == len(pts) == 4 * k + 3
    assert r255.equal(bp.msm(sc, pts), r255.IDENTITY)
    # not for a proof whose z_0 moved
    o = {name: off for name, off, _ in rr.regions(k)}["z"]
    bad = pf[:o] + rr.sb(P.z[0] + 1) + pf[o + 32:]
    sc, pts = rr.merged_terms(rr.Parsed(cards, co, bad, b"bp-perm"), rho)
    assert not r255.equal(bp.msm(sc, pts), r255.IDENTITY)
