"""Large circuits on the GPU (bpp_circuit_create_ex): the large-circuit kernels
forced onto small circuits reproduce the pinned bytes (TILED); each of them
alone and together on circuits no old entry point accepts, checked against the
curve-free helper (tests/circuit_large_ref.py), the host witness and the three
verifiers; an unsatisfied assert refused by name with nothing written and no
secret left; a 1024-wide group beside a 4-wide one in bpp_verify_groups; the old
provers' bytes unchanged afterwards."""
import ctypes
import json
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_large_ref as lr  # noqa: E402
import circuit_pub_ref as cp  # noqa: E402
import circuit_ref as cr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402

pytestmark = pytest.mark.gpu
L = bp.L
GOLDEN = json.loads((HERE / "golden" / "circuit.json").read_text())["cases"]
GOLDEN_PUB = json.loads((HERE / "golden" / "circuit_pub.json").read_text())["cases"]
LARGE = ["chain683", "q1508", "shuffle416", "rangemany18"]


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 2048)
    yield g
    g.close()


def enc(rows):
    return None if rows is None else [[cr.sb(x) for x in row] for row in rows]


unhex = lambda rows: [[bytes.fromhex(h) for h in row] for row in rows]


# ------------------------------------------- 1. TILED reproduces the pinned bytes

@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c["name"])
def test_tiled_gives_the_golden_bytes(gens, case):
    import bpperm
    desc = cr.satisfying(case["name"], 0)[0]
    pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, tiled=True), label=case["label"].encode())
    assert pr.circuit.digest.hex() == case["digest"]
    proofs, Vs = pr.prove_batch(unhex(case["v"]), unhex(case["aux"]),
                                b"".join(bytes.fromhex(s) for s in case["seeds"]),
                                unhex(case["gammas"]) if case["gammas"] else None)
    assert [p.hex() for p in proofs] == case["proofs"]
    assert [v.hex() for v in Vs] == ["".join(v) for v in case["V"]]
    assert all(pr.verify(p, v) for p, v in zip(proofs, Vs))
    assert pr.verify_batch(proofs, Vs)
    assert pr.verify_batch_each(proofs, Vs) == [True] * len(proofs)


@pytest.mark.parametrize("case", GOLDEN_PUB, ids=lambda c: c["name"])
def test_tiled_gives_the_golden_bytes_with_public_inputs(gens, case):
    import bpperm
    desc = cp.satisfying(case["name"], 0)[0]
    pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, tiled=True), label=case["label"].encode())
    assert pr.circuit.digest.hex() == case["digest"]
    pub = unhex(case["pub"])
    proofs, Vs = pr.prove_batch(unhex(case["v"]), None, b"".join(bytes.fromhex(s) for s in case["seeds"]),
                                unhex(case["gammas"]), pub=pub)
    assert [p.hex() for p in proofs] == case["proofs"]
    assert [v.hex() for v in Vs] == ["".join(v) for v in case["V"]]
    assert all(pr.verify(p, v, pub=u) for p, v, u in zip(proofs, Vs, pub))
    assert pr.verify_batch(proofs, Vs, pub=pub)
    assert pr.verify_batch_each(proofs, Vs, pub=pub) == [True] * len(proofs)


def _tamper(proofs, Vs, i, what, v_at=0):
    p, v = bytearray(proofs[i]), bytearray(Vs[i])
    if what == "V":
        v[32 * v_at + 5] ^= 1
    elif what == "t_hat":
        p[32 * 10 + 3] ^= 1
    else:  # "L": the first round's L
        p[32 * 11 + 7] ^= 1
    return proofs[:i] + [bytes(p)] + proofs[i + 1:], Vs[:i] + [bytes(v)] + Vs[i + 1:]


def test_tiled_batch_names_the_tampered_proof(gens):
    """8 proofs of the heavy circuit made plain, verified under TILED: the
    flags are no part of the statement, and the tiled verifier names exactly the
    tampered proof."""
    import bpperm
    got = [cr.satisfying("heavy", i) for i in range(8)]
    desc = got[0][0]
    plain = bpperm.CircuitProver(gens, desc)
    tiled = bpperm.CircuitProver(gens, bpperm.Circuit(desc, tiled=True))
    seeds = b"".join(cr.seed32(b"lt8-%d" % i) for i in range(8))
    proofs, Vs = plain.prove_batch(enc([g[1] for g in got]), None, seeds)
    assert tiled.prove_batch(enc([g[1] for g in got]), None, seeds) == (proofs, Vs)
    assert tiled.verify_batch(proofs, Vs) and plain.verify_batch(proofs, Vs)
    for what, i in (("V", 0), ("t_hat", 3), ("L", 6)):
        bp_, bv = _tamper(proofs, Vs, i, what, v_at=2)
        assert not tiled.verify_batch(bp_, bv)
        assert tiled.verify_batch_each(bp_, bv) == [j != i for j in range(8)]
        assert not tiled.verify(bp_[i], bv[i])


@pytest.mark.parametrize("n_asserts", [166, 167], ids=["len768", "len769"])
def test_table_seams_tiled_equals_plain(gens, n_asserts):
    """The circuit built for the split table's seams (circuit_large_ref
    seam_circuit: distinct coefficients on the rows around e = 256, 512, 768),
    at a table length of exactly 768 and of 769: tiled and plain bytes are
    identical, each verifies the other's, and the helper's scalars agree."""
    import bpperm
    desc = lr.seam_circuit(n_asserts)
    vs = [lr.seam_instance(n_asserts, i) for i in range(3)]
    plain = bpperm.CircuitProver(gens, desc)
    tiled = bpperm.CircuitProver(gens, bpperm.Circuit(desc, tiled=True))
    assert tiled.circuit.Q + 1 == 602 + n_asserts and tiled.circuit.n_p == 512
    seeds = [cr.seed32(b"seam-%d-%d" % (n_asserts, i)) for i in range(3)]
    a = plain.prove_batch(enc(vs), None, b"".join(seeds))
    b = tiled.prove_batch(enc(vs), None, b"".join(seeds))
    assert a == b
    want = lr.prover_scalars(desc, vs[2], [], seeds[2], None, None, b[1][2], b[0][2])
    _, tau_x, mu, t_hat = lr.proof_fields(b[0][2])
    assert (t_hat, tau_x, mu) == want
    assert tiled.verify_batch(*a) and plain.verify_batch(*b)
    assert tiled.verify_batch_each(*a) == [True] * 3 and all(tiled.verify(p, v) for p, v in zip(*a))


# ----------------------------------- 2. each new kernel alone and together

@pytest.fixture(scope="module")
def proved(gens):
    """name -> (desc, prover, vs, auxs, pubs, seeds, proofs, Vs): three proofs of
    each large circuit, proved once on the device-witness path."""
    import bpperm
    cache = {}

    def get(name):
        if name not in cache:
            desc, vs, auxs, pubs = lr.large_case(name, 3)
            pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, large=True))
            seeds = [cr.seed32(b"lg-%s-%d" % (name.encode(), i)) for i in range(3)]
            proofs, Vs = pr.prove_batch(enc(vs), enc(auxs), b"".join(seeds), pub=enc(pubs))
            cache[name] = (desc, pr, vs, auxs, pubs, seeds, proofs, Vs)
        return cache[name]

    return get


@pytest.mark.parametrize("name", LARGE)
def test_large_circuit_proves_and_verifies(proved, monkeypatch, name):
    """chain683: the wide witness kernel, one-table row kernels, 683 levels;
    q1508: the LDS witness kernel, split tables; shuffle416: both, with public
    inputs, a deck per proof; rangemany18: 1152 free gates at n_p = 2048, Q =
    2323.  The prover's t_hat, tau_x and mu equal the helper's, the host witness
    gives the same bytes, and the three verifiers accept."""
    desc, pr, vs, auxs, pubs, seeds, proofs, Vs = proved(name)
    c = pr.circuit
    assert (c.n_p, c.Q) == {"chain683": (1024, 1367), "q1508": (512, 1508), "shuffle416": (1024, 1662),
                            "rangemany18": (2048, 2323)}[name]
    for i in range(3):
        want = lr.prover_scalars(desc, vs[i], auxs[i] if auxs else [], seeds[i], None, pubs[i] if pubs else None,
                                 Vs[i], proofs[i])
        _, tau_x, mu, t_hat = lr.proof_fields(proofs[i])
        assert (t_hat, tau_x, mu) == want, i
    monkeypatch.setenv("BPP_CIRCUIT_HOST_WITNESS", "1")
    host = pr.prove_batch(enc(vs), enc(auxs), b"".join(seeds), pub=enc(pubs))
    monkeypatch.delenv("BPP_CIRCUIT_HOST_WITNESS")
    assert host == (proofs, Vs)
    pub = enc(pubs)
    assert all(pr.verify(proofs[i], Vs[i], pub=pub[i] if pub else None) for i in range(3))
    assert pr.verify_batch(proofs, Vs, pub=pub)
    assert pr.verify_batch_each(proofs, Vs, pub=pub) == [True] * 3


def _rejects_all(pr, proofs, Vs, pub):
    assert not pr.verify_batch(proofs, Vs, pub=pub)
    assert pr.verify_batch_each(proofs, Vs, pub=pub) == [False] * len(proofs)
    assert not any(pr.verify(p, v, pub=pub[i] if pub else None) for i, (p, v) in enumerate(zip(proofs, Vs)))


@pytest.mark.parametrize("name", LARGE)
def test_large_circuit_rejections(gens, proved, name):
    """Every proof rejects: one flipped byte in V, in t_hat or in an L of each; a
    description with a changed coefficient in its last combination (rangemany18,
    q1508: an assert's row, past 1507 and at 1507; shuffle416: the assert on the
    chains' ends; chain683: the last gate's right side); shuffle416: every proof
    given another proof's deck."""
    import bpperm
    desc, pr, vs, auxs, pubs, seeds, proofs, Vs = proved(name)
    pub = enc(pubs)
    for what in ("V", "t_hat", "L"):
        bp_, bv = proofs, Vs
        for i in range(3):
            bp_, bv = _tamper(bp_, bv, i, what)
        _rejects_all(pr, bp_, bv, pub)
    other = bpperm.CircuitProver(gens, bpperm.Circuit(lr.changed_coefficient(desc, len(desc.lc_coef) - 1), large=True))
    assert other.circuit.digest != pr.circuit.digest
    _rejects_all(other, proofs, Vs, pub)
    if pub:
        _rejects_all(pr, proofs, Vs, pub[1:] + pub[:1])
        swapped = [pub[1], pub[0], pub[2]]
        assert pr.verify_batch_each(proofs, Vs, pub=swapped) == [False, False, True]


def test_large_flags_verify_each_others_proofs(gens, proved):
    """chain683 exists under LARGE and under TILED (not without flags): the
    same bytes from both, and each verifies the other's."""
    import bpperm
    desc, pr, vs, auxs, pubs, seeds, proofs, Vs = proved("chain683")
    tiled = bpperm.CircuitProver(gens, bpperm.Circuit(desc, tiled=True))
    assert tiled.prove_batch(enc(vs), None, b"".join(seeds)) == (proofs, Vs)
    assert tiled.verify_batch(proofs, Vs) and tiled.verify_batch_each(proofs, Vs) == [True] * 3


# ------------------------------------ 3. an unsatisfied assert in a large circuit

@pytest.mark.parametrize("streams", [1, 3])
def test_large_unsatisfied_assert_is_refused_by_name(ctx, gens, monkeypatch, streams):
    """Proof 1 of 3 claims 2^64 < 2^64 in its last value: BPP_ERR_ARG naming
    proof 1 and the last assert (that value's bit sum), no output byte written,
    no secret left -- the wide kernel's wires included -- and none after the
    passing batch that follows."""
    import bpperm
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    desc, vs, auxs, _ = lr.large_case("rangemany18", 3)
    pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, large=True))
    good_v, good_aux = list(vs[1]), auxs[1]
    vs[1] = vs[1][:-1] + [1 << 64]
    auxs[1] = desc.aux_of(vs[1][:-1] + [0])
    seeds = b"".join(cr.seed32(b"lua-%d" % i) for i in range(3))
    pf = ctypes.create_string_buffer(b"\xa5" * (pr.proof_len * 3))
    V = ctypes.create_string_buffer(b"\x5a" * (32 * pr.m * 3))
    bpperm.PermProver(gens, 52).prove_batch([3, 4, 5])  # a test-hook batch leaves its secrets in place
    assert ctx.secret_residue() > 0
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc(vs), enc(auxs), seeds, out=(pf, V))
    assert e.value.code == 1 and "proof 1" in str(e.value) and "assert %d " % (desc.n_asserts - 1) in str(e.value)
    assert pf.raw[:pr.proof_len * 3] == b"\xa5" * (pr.proof_len * 3) and V.raw[:32 * pr.m * 3] == b"\x5a" * (32 * pr.m * 3)
    assert ctx.secret_residue() == 0
    vs[1], auxs[1] = good_v, good_aux
    bpperm.PermProver(gens, 52).prove_batch([3, 4, 5])
    assert ctx.secret_residue() > 0
    got = pr.prove_batch(enc(vs), enc(auxs), seeds)
    assert ctx.secret_residue() == 0
    assert pr.verify_batch(*got)


# ----------------------------------------------------- 4. mixed-width groups

def test_verify_groups_wide_beside_narrow(gens, proved):
    """One shuffle_of_public(416) group (n_p = 1024) beside an opens_to group (n_p
    = 4) in one bpp_verify_groups call, in both orders: the narrow circuit's
    generators are the wide one's first four.  each=True names the one tampered
    proof of the wide group."""
    import bpperm
    desc, pr, vs, auxs, pubs, seeds, proofs, Vs = proved("shuffle416")
    pub = enc(pubs)
    got = [cp.satisfying("opens", i) for i in range(2)]
    op = bpperm.CircuitProver(gens, got[0][0], label=b"opens")
    opub = enc([g[3] for g in got])
    oproofs, oVs = op.prove_batch(enc([g[1] for g in got]), None, b"".join(cr.seed32(b"lgo-%d" % i) for i in range(2)),
                                  pub=opub)
    wide, narrow = (pr, proofs, Vs, pub), (op, oproofs, oVs, opub)
    assert bpperm.verify_groups(gens, [wide, narrow]) and bpperm.verify_groups(gens, [narrow, wide])
    assert bpperm.verify_groups(gens, [wide, narrow], each=True) == [[True] * 3, [True] * 2]
    bp_, bv = _tamper(proofs, Vs, 1, "t_hat")
    bad = (pr, bp_, bv, pub)
    assert not bpperm.verify_groups(gens, [bad, narrow]) and not bpperm.verify_groups(gens, [narrow, bad])
    assert bpperm.verify_groups(gens, [bad, narrow], each=True) == [[True, False, True], [True] * 2]
    assert bpperm.verify_groups(gens, [narrow, bad], each=True) == [[True] * 2, [True, False, True]]


# ------------------------------- 5. the existing entry points after a large batch

def test_old_provers_unchanged_after_a_large_batch(gens):
    """PermProver(52)'s seeded bytes (the golden config-1 proof among them) and
    two_half_shuffle(3)'s are the same before and after a large batch on the
    same context."""
    import bpperm
    gold = json.loads((HERE / "golden" / "protocol.json").read_text())["config1"]
    old = bpperm.PermProver(gens, 52, label=gold["label"].encode())
    th = [cr.satisfying("twohalf3", i) for i in range(3)]
    prog = bpperm.CircuitProver(gens, th[0][0])
    tseeds = b"".join(cr.seed32(b"lgold-%d" % i) for i in range(3))
    before = old.prove_batch([gold["seed"], 12, 13])
    tbefore = prog.prove_batch(enc([t[1] for t in th]), None, tseeds)
    assert before[0][0].hex() == gold["proof"] and before[1][0].hex() == "".join(gold["V"])
    desc, vs, auxs, pubs = lr.large_case("shuffle416", 3)
    big = bpperm.CircuitProver(gens, bpperm.Circuit(desc, large=True))
    got = big.prove_batch(enc(vs), None, pub=enc(pubs))
    assert big.verify_batch(*got, pub=enc(pubs))
    assert old.prove_batch([gold["seed"], 12, 13]) == before
    assert prog.prove_batch(enc([t[1] for t in th]), None, tseeds) == tbefore
    assert old.verify_batch(*before) and prog.verify_batch(*tbefore)
