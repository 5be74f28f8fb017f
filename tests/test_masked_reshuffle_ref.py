"""The masked re-shuffle argument on the host, in the reference helper alone
(tests/masked_reshuffle_ref.py; no GPU, no library): completeness over k = 2..6
and the edge inputs, every region of the proof bound, the proof bound to its
label, its key, the order of its cards and the order of a card's halves, forced
proofs of false statements failing exactly the check they should (one re-mask
scalar binds both halves of a card), the merged form of the first three checks,
and unmasking with the key's discrete log."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import masked_reshuffle_ref as mr  # noqa: E402
from oracle import bulletproofs as bp, ristretto as r255  # noqa: E402
from oracle.merlin import pedersen_gens_default  # noqa: E402

L = mr.L
ALL = (True, True, True, True)


def add_to(enc: bytes, point) -> bytes:
    return r255.encode(r255.ed_add(r255.decode(enc), point))


@pytest.fixture(scope="module")
def proved():
    """k -> (key, cards_in, perm, cards_out, proof), proved once."""
    out = {}
    for k in range(2, 7):
        tag = b"mref-%d" % k
        key, cards, perm = mr.rand_point(tag), mr.rand_cards(k, tag), mr.rand_perm(k, tag)
        co, pf = mr.prove(key, cards, perm, mr.seed32(tag))
        out[k] = (key, cards, perm, co, pf)
    return out


@pytest.mark.parametrize("k", range(2, 7))
def test_prove_then_verify(proved, k):
    key, cards, perm, co, pf = proved[k]
    assert len(pf) == mr.proof_len(k) == mr.rr.proof_len(k) + 32
    assert [name for name, _, _ in mr.regions(k)][-1] == "inner"
    assert sum(n for _, _, n in mr.regions(k)) == len(pf)
    assert mr.verify_parts(key, cards, co, pf) == ALL
    assert co == mr.remask(key, cards, perm, mr.draws(mr.seed32(b"mref-%d" % k), k)[0])


def test_proof_length_at_52_cards():
    assert mr.proof_len(52) == 9312


@pytest.mark.parametrize("name", mr.EDGES)
@pytest.mark.parametrize("k", [2, 5])
def test_edge_inputs(k, name):
    """The open deck, a card (identity, identity), two equal cards, r_0 = 0, pi
    the identity and the reversal, K the identity."""
    key, cards, perm, blinds = mr.edge_case(k, name)
    co, pf = mr.prove(key, cards, perm, mr.seed32(b"edge-%d" % k), blinds)
    assert mr.verify_parts(key, cards, co, pf) == ALL
    if name == "zero-blind":
        assert co[0] == cards[perm[0]]  # (r_0 = 0: the card itself)
    if name == "pi-identity":
        assert all(co[i][:32] != cards[i][:32] and co[i][32:] != cards[i][32:] for i in range(k))
    if name == "open-deck":
        assert all(c[:32] == mr.IDENTITY for c in cards) and all(c[:32] != mr.IDENTITY for c in co)
    if name == "key-identity":
        assert all(co[i][32:] == cards[perm[i]][32:] for i in range(k))  # (W is only permuted)


@pytest.mark.parametrize("region", ["A", "E", "Ti", "TU", "TW", "z", "om", "zR", "Vk", "inner"])
@pytest.mark.parametrize("k", [2, 3])
def test_each_region_is_bound(proved, k, region):
    """A point replaced by another valid point, a scalar by itself + 1: the
    first field of each of the ten regions."""
    key, cards, _, co, pf = proved[k]
    o = {name: off for name, off, _ in mr.regions(k)}[region]
    if region in ("z", "om", "zR"):
        new = mr.sb(int.from_bytes(pf[o:o + 32], "little") + 1)
    elif region == "inner":
        o += 8 * 32  # tau_x, the inner proof's first scalar
        new = mr.sb(int.from_bytes(pf[o:o + 32], "little") + 1)
    else:
        new = mr.rand_point(b"other-" + region.encode())
    bad = pf[:o] + new + pf[o + 32:]
    assert bad != pf and not mr.verify(key, cards, co, bad)


def test_bound_to_label_key_card_order_and_halves(proved):
    k = 5
    key, cards, _, co, pf = proved[k]
    assert mr.verify(key, cards, co, pf, b"bp-perm")
    assert not mr.verify(key, cards, co, pf, b"another label")
    assert not mr.verify(mr.rand_point(b"another key"), cards, co, pf)
    assert not mr.verify(key, [cards[1], cards[0]] + cards[2:], co, pf)
    assert not mr.verify(key, cards, [co[1], co[0]] + co[2:], pf)
    flip = lambda c: c[32:] + c[:32]
    assert not mr.verify(key, [flip(cards[0])] + cards[1:], co, pf)
    assert not mr.verify(key, cards, [flip(co[0])] + co[1:], pf)
    assert not mr.verify(key, [flip(c) for c in cards], [flip(c) for c in co], pf)
    assert mr.verify_parts(key, cards, co, pf[:-1]) == (False,) * 4  # a short proof


def test_noncanonical_scalar_and_bad_point_are_rejected(proved):
    k = 3
    key, cards, _, co, pf = proved[k]
    o = {name: off for name, off, _ in mr.regions(k)}
    undecodable = b"\xff" * 32
    assert not mr.verify(key, cards, co, pf[:o["z"]] + L.to_bytes(32, "little") + pf[o["z"] + 32:])
    assert not mr.verify(key, cards, co, pf[:o["TW"]] + undecodable + pf[o["TW"] + 32:])
    assert not mr.verify(key, cards, [co[0][:32] + undecodable] + co[1:], pf)
    assert not mr.verify(undecodable, cards, co, pf)


def test_moved_W_fails_check_ii_W_alone(proved):
    k = 4
    key, cards, perm, co, _ = proved[k]
    g, _ = pedersen_gens_default()
    moved = [co[0][:32] + add_to(co[0][32:], g)] + co[1:]
    out, pf = mr.prove(key, cards, perm, mr.seed32(b"mref-%d" % k), cards_out=moved)
    assert out == moved
    assert mr.verify_parts(key, cards, moved, pf) == (True, True, False, True)


def test_moved_U_fails_check_ii_U_alone(proved):
    k = 4
    key, cards, perm, co, _ = proved[k]
    g, _ = pedersen_gens_default()
    moved = [add_to(co[0][:32], g) + co[0][32:]] + co[1:]
    _, pf = mr.prove(key, cards, perm, mr.seed32(b"mref-%d" % k), cards_out=moved)
    assert mr.verify_parts(key, cards, moved, pf) == (True, False, True, True)


def test_one_remask_scalar_binds_both_halves(proved):
    """U'_0 = U_pi(0) + r B but W'_0 = W_pi(0) + (r + 1) K: each half alone is a
    re-masking, under different scalars.  z_R carries one sum_i b_i r_i for both
    checks, so (ii-W) fails with everything else intact."""
    k = 4
    key, cards, perm, co, _ = proved[k]
    moved = [co[0][:32] + add_to(co[0][32:], r255.decode(key))] + co[1:]
    _, pf = mr.prove(key, cards, perm, mr.seed32(b"mref-%d" % k), cards_out=moved)
    assert mr.verify_parts(key, cards, moved, pf) == (True, True, False, True)
    # the same output is a valid statement half by half: U alone and W alone re-mask
    r = mr.draws(mr.seed32(b"mref-%d" % k), k)[0]
    assert moved[0][32:] == mr.remask(key, cards, perm, [r[0] + 1] + r[1:])[0][32:]
    assert moved[0][:32] == mr.remask(key, cards, perm, r)[0][:32]


def test_output_that_repeats_an_input_is_rejected():
    """No bijection: the honest prover refuses it; forced through, the inner
    proof fails, and so do both (ii) checks."""
    k = 4
    key, cards = mr.rand_point(b"repeat"), mr.rand_cards(k, b"repeat")
    pi = [2, 2, 0, 1]
    with pytest.raises(AssertionError):
        mr.prove(key, cards, pi, mr.seed32(b"repeat"))
    co, pf = mr.prove(key, cards, pi, mr.seed32(b"repeat"), force=True)
    one, two_u, two_w, inner = mr.verify_parts(key, cards, co, pf)
    assert one and not inner and not two_u and not two_w


@pytest.mark.parametrize("k", [2, 4, 6])
def test_merged_terms_sum_to_the_identity(proved, k):
    key, cards, _, co, pf = proved[k]
    P = mr.Parsed(key, cards, co, pf, b"bp-perm")
    rho = mr.batch_weight(mr.seed32(b"verifier"), 7, P.c)
    sc, pts = mr.merged_terms(P, rho)
    assert len(sc) == len(pts) == 6 * k + 5
    assert r255.equal(bp.msm(sc, pts), r255.IDENTITY)
    o = {name: off for name, off, _ in mr.regions(k)}["z"]
    bad = pf[:o] + mr.sb(P.z[0] + 1) + pf[o + 32:]
    sc, pts = mr.merged_terms(mr.Parsed(key, cards, co, bad, b"bp-perm"), rho)
    assert not r255.equal(bp.msm(sc, pts), r255.IDENTITY)


def test_unmask_returns_the_permuted_deck():
    k = 5
    sk = mr.rand_scalar(b"unmask-sk")
    key = mr.key_of(sk)
    M = [mr.rand_point(b"unmask-M%d" % j) for j in range(k)]
    perm = mr.rand_perm(k, b"unmask")
    co, pf = mr.prove(key, mr.open_deck(M), perm, mr.seed32(b"unmask"))
    assert mr.verify(key, mr.open_deck(M), co, pf)
    assert mr.unmask(co, sk) == [M[perm[i]] for i in range(k)]
    assert mr.unmask(co, sk + 1) != [M[perm[i]] for i in range(k)]


def test_three_chained_shuffles_unmask_to_the_composed_permutation():
    k = 4
    sks = [mr.rand_scalar(b"chain-sk%d" % j) for j in range(3)]
    key = mr.key_of(sum(sks))
    M = [mr.rand_point(b"chain-M%d" % j) for j in range(k)]
    cards, src = mr.open_deck(M), list(range(k))
    for s in range(3):
        perm = mr.rand_perm(k, b"chain-%d" % s)
        nxt, pf = mr.prove(key, cards, perm, mr.seed32(b"chain-%d" % s), label=b"chain")
        assert mr.verify(key, cards, nxt, pf, b"chain")
        src = [src[perm[i]] for i in range(k)]
        cards = nxt
    assert mr.unmask(cards, sum(sks)) == [M[j] for j in src]
