"""bpp_circuit_* on the GPU: proofs of caller-defined circuits byte-exact against
the reference helper (tests/circuit_ref.py) and the committed golden file,
accepted and rejected by the three verifiers, kept apart from two-half proofs of
the same matrices, on both witness paths, under the prover's switches, with an
unsatisfied assert refused by name, the batch's secrets wiped and the old
provers' bytes unchanged."""
import copy
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_child  # noqa: E402
import circuit_ref as cr  # noqa: E402
import shuffle_ref as sr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402

pytestmark = pytest.mark.gpu
L = bp.L
GOLDEN = json.loads((HERE / "golden" / "circuit.json").read_text())["cases"]


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens512(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 512)
    yield g
    g.close()


def enc(rows):
    return [[cr.sb(x) for x in row] for row in rows]


def instances(name, n):
    """desc and n satisfied instances (v, aux rows as ints) of a named case."""
    got = [cr.satisfying(name, i) for i in range(n)]
    return got[0][0], [g[1] for g in got], [g[2] for g in got]


@pytest.mark.parametrize("with_gammas", [False, True], ids=["drawn", "supplied"])
@pytest.mark.parametrize("name", ["member2", "twohalf2", "twohalf3", "range3", "heavy", "wide70"])
def test_circuit_bit_exact_vs_helper(gens, name, with_gammas):
    """One gate at n_p = 4 (member2), n = n_p = 4 and n_p = 8 (twohalf2, 3),
    free sides with n_aux = 6 (range3), heavy W_O and W_V columns at n_p = 16
    (heavy), m = 71 over n_p = 4 (wide70).  Three proofs per call, 0 and l - 1
    among the values and blindings; V and proof bytes equal the helper's, and
    the three verifiers accept."""
    import bpperm
    desc, vs, auxs = instances(name, 3)
    seeds = [cr.seed32(b"gc-%s-%d" % (name.encode(), i)) for i in range(3)]
    gam = None
    if with_gammas:
        gam = [[cr.rand_scalar(b"gcg-%s-%d-%d" % (name.encode(), i, j)) for j in range(desc.m_in)] for i in range(3)]
        gam[1][0], gam[1][-1] = 0, L - 1
        gam[2][0] = L - 1
    pr = bpperm.CircuitProver(gens, desc)
    assert pr.proof_len == cr.proof_len(desc) and pr.m == desc.m_in + 1
    proofs, Vs = pr.prove_batch(enc(vs), enc(auxs), b"".join(seeds), enc(gam) if gam else None)
    for i in range(3):
        want = cr.prove_circuit(desc, vs[i], auxs[i], seeds[i], gam[i] if gam else None)
        assert Vs[i] == b"".join(want.V), i
        assert proofs[i] == want.to_bytes(), i
        assert pr.verify(proofs[i], Vs[i])
    assert pr.verify_batch(proofs, Vs)
    assert pr.verify_batch_each(proofs, Vs) == [True] * 3


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c["name"])
def test_circuit_golden(gens, case):
    import bpperm
    desc = cr.satisfying(case["name"], 0)[0]
    unhex = lambda rows: [[bytes.fromhex(h) for h in row] for row in rows]
    pr = bpperm.CircuitProver(gens, desc, label=case["label"].encode())
    assert pr.circuit.digest.hex() == case["digest"]
    proofs, Vs = pr.prove_batch(unhex(case["v"]), unhex(case["aux"]),
                                b"".join(bytes.fromhex(s) for s in case["seeds"]),
                                unhex(case["gammas"]) if case["gammas"] else None)
    assert [p.hex() for p in proofs] == case["proofs"]
    assert [v.hex() for v in Vs] == ["".join(v) for v in case["V"]]
    assert all(pr.verify(p, v) for p, v in zip(proofs, Vs))
    assert pr.verify_batch(proofs, Vs)
    assert pr.verify_batch_each(proofs, Vs) == [True] * len(proofs)


def test_two_half_program_against_perm_prover(ctx, gens):
    """two_half_shuffle(3) and PermProver(3) prove the same matrices: equal
    proof_len and m, each verifier rejects the other's proofs (the "circuit"
    digest in the transcript), and a verified batch of 8 costs the same work --
    the same launches."""
    import bpperm
    two, prog = bpperm.PermProver(gens, 3), bpperm.CircuitProver(gens, gd.two_half_shuffle(3))
    assert two.proof_len == prog.proof_len and two.m == prog.m
    tp, tv = two.prove_batch(list(range(8)))
    desc, vs, auxs = instances("twohalf3", 8)
    pp, pv = prog.prove_batch(enc(vs), None, b"".join(cr.seed32(b"thp-%d" % i) for i in range(8)))
    ctx.work_reset()
    assert two.verify_batch(tp, tv)
    w_two = ctx.work()
    ctx.work_reset()
    assert prog.verify_batch(pp, pv)
    w_prog = ctx.work()
    assert w_prog == w_two and w_two["msm_terms"] > 0
    assert not prog.verify_batch(tp, tv) and not two.verify_batch(pp, pv)
    assert prog.verify_batch_each(tp, tv) == [False] * 8 and two.verify_batch_each(pp, pv) == [False] * 8
    assert not prog.verify(tp[0], tv[0]) and not two.verify(pp[0], pv[0])


@pytest.fixture(scope="module")
def batch8(gens):
    import bpperm
    desc, vs, auxs = instances("heavy", 8)
    pr = bpperm.CircuitProver(gens, desc)
    proofs, Vs = pr.prove_batch(enc(vs), None, b"".join(cr.seed32(b"b8-%d" % i) for i in range(8)))
    return desc, pr, proofs, Vs


def _tamper(proofs, Vs, i, what):
    p, v = bytearray(proofs[i]), bytearray(Vs[i])
    if what == "V":
        v[32 * 2 + 5] ^= 1
    elif what == "t_hat":
        p[32 * 10 + 3] ^= 1
    elif what == "L":
        p[32 * 11 + 7] ^= 1
    else:  # mu = l: not a canonical scalar
        p[32 * 9: 32 * 10] = L.to_bytes(32, "little")
    return proofs[:i] + [bytes(p)] + proofs[i + 1:], Vs[:i] + [bytes(v)] + Vs[i + 1:]


@pytest.mark.parametrize("what,i", [("V", 0), ("t_hat", 3), ("L", 5), ("mu", 7)])
def test_circuit_batch_names_the_tampered_proof(batch8, what, i):
    desc, pr, proofs, Vs = batch8
    assert pr.verify_batch(proofs, Vs)
    bp_, bv = _tamper(proofs, Vs, i, what)
    assert not pr.verify_batch(bp_, bv)
    each = pr.verify_batch_each(bp_, bv)
    assert each == [j != i for j in range(8)]
    assert each == [pr.verify(p, v) for p, v in zip(bp_, bv)]


def test_circuit_changed_coefficient_and_label_reject_all(gens, batch8):
    import bpperm
    desc, pr, proofs, Vs = batch8
    other = copy.copy(desc)
    other.lc_coef = list(desc.lc_coef)
    t = 0  # gate 0's left side: 1 v_0 -> 3 v_0
    other.lc_coef[t] = cr.sb(int.from_bytes(other.lc_coef[t], "little") + 2)
    assert bpperm.Circuit(other).digest != pr.circuit.digest
    for bad in (bpperm.CircuitProver(gens, other), bpperm.CircuitProver(gens, desc, label=b"another")):
        assert not bad.verify_batch(proofs, Vs)
        assert bad.verify_batch_each(proofs, Vs) == [False] * 8
        assert not any(bad.verify(p, v) for p, v in zip(proofs, Vs))


@pytest.mark.parametrize("streams", [1, 3])
def test_unsatisfied_assert_is_refused_by_name(gens, monkeypatch, streams):
    """Proof 2 of 4 claims 8 < 2^3: BPP_ERR_ARG naming proof 2 and assert 6 (the
    bit sum), the caller's output buffers untouched, no secret left behind, and
    the next valid batch on the same context gives a fresh context's bytes."""
    import bpperm
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    desc = gd.in_range(3)
    pr = bpperm.CircuitProver(gens, desc)
    vs = [[5], [0], [8], [7]]
    auxs = [desc.aux_of([x[0] % 8]) for x in vs]
    seeds = b"".join(cr.seed32(b"ua-%d" % i) for i in range(4))
    pf = ctypes.create_string_buffer(b"\xa5" * (pr.proof_len * 4))
    V = ctypes.create_string_buffer(b"\x5a" * (32 * pr.m * 4))
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc(vs), enc(auxs), seeds, out=(pf, V))
    assert e.value.code == 1 and "proof 2" in str(e.value) and "assert 6" in str(e.value)
    assert pf.raw[:pr.proof_len * 4] == b"\xa5" * (pr.proof_len * 4) and V.raw[:32 * pr.m * 4] == b"\x5a" * (32 * pr.m * 4)
    assert pr.ctx.secret_residue() == 0
    vs[2] = [3]
    auxs[2] = desc.aux_of(vs[2])
    got = pr.prove_batch(enc(vs), enc(auxs), seeds)
    assert pr.verify_batch(*got)
    fresh = bpperm.Context(0)
    try:
        g2 = bpperm.Gens(fresh, 8)
        assert bpperm.CircuitProver(g2, desc).prove_batch(enc(vs), enc(auxs), seeds) == got
        g2.close()
    finally:
        fresh.close()


@pytest.mark.parametrize("n", [277, 278, 300])
def test_product_chain_on_both_witness_paths(gens512, monkeypatch, n):
    """A product chain of n gates: n dependency levels, n_p = 512 (the paths
    beyond POW_LO).  The device witness and the host witness give identical
    bytes, and the batch verifies.  n = 277 is the last chain whose program and
    inputs k_witness_program stages in LDS beside the wires (32 + 96 n + 32 +
    4 (roundup8(11 n + 3) + 24 n + 8) = 65 504 B of 65 536), n = 278 the first
    it reads from global memory (65 728 B)."""
    import bpperm
    desc, vs, auxs = instances("chain%d" % n, 3)
    pr = bpperm.CircuitProver(gens512, desc)
    assert pr.circuit.n_p == 512
    seeds = b"".join(cr.seed32(b"ch-%d" % i) for i in range(3))
    proofs, Vs = pr.prove_batch(enc(vs), None, seeds)
    assert pr.verify_batch(proofs, Vs)
    assert pr.verify_batch_each(proofs, Vs) == [True] * 3
    monkeypatch.setenv("BPP_CIRCUIT_HOST_WITNESS", "1")
    host, hostV = pr.prove_batch(enc(vs), None, seeds)
    monkeypatch.delenv("BPP_CIRCUIT_HOST_WITNESS")
    assert host == proofs and hostV == Vs


def test_two_circuits_of_one_shape_alternated(gens):
    """A, B, A on one context: same sizes, different coefficients (the program
    and CSR uploads are cached by content).  A's bytes repeat, and each batch
    verifies only under its own circuit."""
    import bpperm
    A, B = bpperm.CircuitProver(gens, gd.member_of([3, 7])), bpperm.CircuitProver(gens, gd.member_of([3, 9]))
    assert (A.circuit.Q, A.circuit.n_p, A.m) == (B.circuit.Q, B.circuit.n_p, B.m)
    seeds = b"".join(cr.seed32(b"aba-%d" % i) for i in range(3))
    a1 = A.prove_batch(enc([[3], [7], [7]]), None, seeds)
    b1 = B.prove_batch(enc([[9], [3], [9]]), None, seeds)
    a2 = A.prove_batch(enc([[3], [7], [7]]), None, seeds)
    assert a1 == a2 and a1 != b1
    assert A.verify_batch(*a1) and B.verify_batch(*b1)
    assert not A.verify_batch(*b1) and not B.verify_batch(*a1)
    assert A.verify_batch_each(*b1) == [False] * 3 and B.verify_batch_each(*a2) == [False] * 3


@pytest.mark.parametrize("env", [{"BPP_PROVE_STREAMS": "3"}, {"BPP_PROVE_DEV_V": "0"}, {"BPP_PROVE_DEV_V": "1"}],
                         ids=["streams3", "dev_v0", "dev_v1"])
def test_circuit_bytes_under_switches(ctx, env):
    """The same proofs under BPP_PROVE_STREAMS=3 and both settings of
    BPP_PROVE_DEV_V, each in a child process."""
    want_p, want_v = circuit_child.prove(ctx)
    e = {k: v for k, v in os.environ.items() if k not in ("BPP_PROVE_STREAMS", "BPP_PROVE_DEV_V")}
    e.update(env)
    r = subprocess.run([sys.executable, str(HERE / "circuit_child.py")], capture_output=True, text=True, env=e,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines() if line.startswith(("PROOFS ", "V ")))
    assert out["PROOFS"] == want_p.hex() and out["V"] == want_v.hex()


@pytest.mark.parametrize("streams", [1, 3])
def test_circuit_leaves_no_secret_bytes(ctx, gens, monkeypatch, streams):
    import bpperm
    n = 7
    desc = gd.in_range(6)
    pr = bpperm.CircuitProver(gens, desc)
    vs = [[(9 * i + 4) % 64] for i in range(n)]
    auxs = [desc.aux_of(x) for x in vs]
    seeds = b"".join(cr.seed32(b"cres-%d" % i) for i in range(n))
    gam = [[cr.rand_scalar(b"crg-%d" % p)] for p in range(n)]
    monkeypatch.setenv("BPP_PROVE_STREAMS", "1")
    want = pr.prove_batch(enc(vs), enc(auxs), seeds, enc(gam))
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    bpperm.PermProver(gens, 52).prove_batch([3, 4, 5])  # a test-hook batch leaves its secrets in place
    assert ctx.secret_residue() > 0
    got = pr.prove_batch(enc(vs), enc(auxs), seeds, enc(gam))
    assert ctx.secret_residue() == 0
    assert got == want
    assert pr.verify_batch(*got)


def test_old_provers_unchanged_after_a_circuit_batch(gens):
    """A seeded batch (the golden config-1 proof among it), a shuffle batch and
    a deck batch give the same bytes before and after a circuit batch on the
    same context."""
    import bpperm
    k = 52
    sb = lambda xs: [sr.scalar_bytes(x) for x in xs]
    gold = json.loads((HERE / "golden" / "protocol.json").read_text())["config1"]
    pr = bpperm.PermProver(gens, k, label=gold["label"].encode())
    dk = bpperm.DeckProver(gens, k)
    cards = [sb(sr.rand_scalar(b"occ-%d-%d" % (p, i)) for i in range(k)) for p in range(2)]
    perms = [sr.rand_perm(k, b"occ-%d" % p) for p in range(2)]
    sseeds = b"".join(sr.seed32(b"occ-%d" % p) for p in range(2))
    before = pr.prove_batch([gold["seed"], 12, 13])
    sbefore = pr.prove_shuffle_batch(cards, perms, sseeds)
    dbefore = dk.prove_batch(perms, sseeds)
    assert before[0][0].hex() == gold["proof"] and before[1][0].hex() == "".join(gold["V"])
    desc, vs, auxs = instances("twohalf52", 3)
    cp = bpperm.CircuitProver(gens, desc)
    got = cp.prove_batch(enc(vs), None)
    assert cp.verify_batch(*got)
    assert pr.prove_batch([gold["seed"], 12, 13]) == before
    assert pr.prove_shuffle_batch(cards, perms, sseeds) == sbefore
    assert dk.prove_batch(perms, sseeds) == dbefore
    assert pr.verify_batch(before[0] + sbefore[0], before[1] + sbefore[1]) and dk.verify_batch(*dbefore)
