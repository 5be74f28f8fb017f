"""bpp_circuit_*_pub on the GPU: proofs of circuits with per-proof public inputs
byte-exact against the reference helper (tests/circuit_pub_ref.py) and the
committed golden file, accepted by the three verifiers under their own public
inputs and rejected, by name, under any other; both witness paths; an
unsatisfied public assert refused by name; the old entry points and the new
ones kept apart; the prover's switches; the batch's secrets wiped and the old
provers' bytes unchanged."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_pub_child  # noqa: E402
import circuit_pub_ref as cp  # noqa: E402
import circuit_ref as cr  # noqa: E402
import shuffle_ref as sr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402

pytestmark = pytest.mark.gpu
L = cp.L
GOLDEN = json.loads((HERE / "golden" / "circuit_pub.json").read_text())["cases"]


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens256(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 256)
    yield g
    g.close()


def enc(rows):
    return [[cp.sb(x) for x in row] for row in rows]


def instances(name, n):
    """desc and n satisfied instances (v, pub rows as ints) of a named case."""
    got = [cp.satisfying(name, i) for i in range(n)]
    assert not any(g[2] for g in got)  # (no case here has free sides)
    return got[0][0], [g[1] for g in got], [g[3] for g in got]


@pytest.mark.parametrize("with_gammas", [False, True], ids=["drawn", "supplied"])
@pytest.mark.parametrize("name", ["opens", "memberpub2", "memberpub13", "sum3", "shufflepub2", "shufflepub3",
                                  "heavypub", "widepub300", "widepub400"])
def test_circuit_pub_bit_exact_vs_helper(gens, name, with_gammas):
    """One gate at n_p = 4 and n_pub = 1 (opens), 12 gates at n_p = 16
    (memberpub13), an assert alone reading the public input (sum3), a public
    chain beside the committed one (shufflepub2: n = 2 at n_p = 4, shufflepub3:
    n = n_p = 4), one public input in 13 rows (heavypub), n_pub = 300 over n_p =
    4 -- more W_U entries than the kernel has lanes (widepub300), and n_pub =
    400, the first of these whose proof, V and public words together pass the
    48 KB the replay stages in LDS, so it reads them from global memory
    (widepub400: 4 groups x (136 + 8 x 406) words = 54 144 B).  Three proofs
    per call, 0 and l - 1 among the public inputs and blindings; V and proof
    bytes equal the helper's, and the three verifiers accept."""
    import bpperm
    desc, vs, pubs = instances(name, 3)
    seeds = [cp.seed32(b"gcp-%s-%d" % (name.encode(), i)) for i in range(3)]
    gam = None
    if with_gammas:
        gam = [[cp.rand_scalar(b"gcpg-%s-%d-%d" % (name.encode(), i, j)) for j in range(desc.m_in)] for i in range(3)]
        gam[1][0], gam[1][-1] = 0, L - 1
        gam[2][0] = L - 1
    pr = bpperm.CircuitProver(gens, desc)
    assert pr.proof_len == cp.proof_len(desc) and pr.m == desc.m_in + 1 and pr.circuit.n_pub == desc.n_pub
    proofs, Vs = pr.prove_batch(enc(vs), None, b"".join(seeds), enc(gam) if gam else None, pub=enc(pubs))
    for i in range(3):
        want = cp.prove_circuit(desc, vs[i], [], pubs[i], seeds[i], gam[i] if gam else None)
        assert Vs[i] == b"".join(want.V), i
        assert proofs[i] == want.to_bytes(), i
        assert pr.verify(proofs[i], Vs[i], pub=enc(pubs)[i])
    assert pr.verify_batch(proofs, Vs, pub=enc(pubs))
    assert pr.verify_batch_each(proofs, Vs, pub=enc(pubs)) == [True] * 3


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c["name"])
def test_circuit_pub_golden(gens, case):
    import bpperm
    desc = cp.satisfying(case["name"], 0)[0]
    unhex = lambda rows: [[bytes.fromhex(h) for h in row] for row in rows]
    pr = bpperm.CircuitProver(gens, desc, label=case["label"].encode())
    assert pr.circuit.digest.hex() == case["digest"]
    pub = unhex(case["pub"])
    proofs, Vs = pr.prove_batch(unhex(case["v"]), None, b"".join(bytes.fromhex(s) for s in case["seeds"]),
                                unhex(case["gammas"]), pub=pub)
    assert [p.hex() for p in proofs] == case["proofs"]
    assert [v.hex() for v in Vs] == ["".join(v) for v in case["V"]]
    assert all(pr.verify(p, v, pub=u) for p, v, u in zip(proofs, Vs, pub))
    assert pr.verify_batch(proofs, Vs, pub=pub)
    assert pr.verify_batch_each(proofs, Vs, pub=pub) == [True] * len(proofs)


@pytest.fixture(scope="module")
def batch5(gens):
    """Five proofs of member_of_public(13) over five sets: not a multiple of the
    replay's groups per block, so its pad group runs."""
    import bpperm
    desc, vs, pubs = instances("memberpub13", 5)
    pr = bpperm.CircuitProver(gens, desc)
    proofs, Vs = pr.prove_batch(enc(vs), None, b"".join(cp.seed32(b"b5-%d" % i) for i in range(5)), pub=enc(pubs))
    return pr, proofs, Vs, [b"".join(row) for row in enc(pubs)]


def test_count_5_verifies(batch5):
    pr, proofs, Vs, pubs = batch5
    assert pr.verify_batch(proofs, Vs, pub=pubs)
    assert pr.verify_batch_each(proofs, Vs, pub=pubs) == [True] * 5


def _flip(b, at):
    b = bytearray(b)
    b[at] ^= 1
    return bytes(b)


@pytest.mark.parametrize("what", ["pub3", "swap14", "V2"])
def test_rejections_are_named_per_proof(batch5, what):
    pr, proofs, Vs, pubs = batch5
    Vs, pubs = list(Vs), list(pubs)
    if what == "pub3":  # one byte of proof 3's public inputs (the low byte of u_7: still canonical)
        pubs[3] = _flip(pubs[3], 32 * 7)
        bad = {3}
    elif what == "swap14":
        pubs[1], pubs[4] = pubs[4], pubs[1]
        bad = {1, 4}
    else:
        Vs[2] = _flip(Vs[2], 5)
        bad = {2}
    assert not pr.verify_batch(proofs, Vs, pub=pubs)
    each = pr.verify_batch_each(proofs, Vs, pub=pubs)
    assert each == [j not in bad for j in range(5)]
    assert each == [pr.verify(p, v, pub=u) for p, v, u in zip(proofs, Vs, pubs)]


def test_shuffle_of_public_52_eight_decks_one_batch(ctx, gens):
    """102 gates, n_p = 128, n_pub = 52: eight tables, eight decks, one circuit
    and one merged MSM."""
    import bpperm
    desc, vs, pubs = instances("shufflepub52", 8)
    assert (desc.n_gates, desc.m_in, desc.n_pub) == (102, 52, 52)
    pr = bpperm.CircuitProver(gens, desc)
    assert pr.circuit.n_p == 128
    proofs, Vs = pr.prove_batch(enc(vs), None, b"".join(cp.seed32(b"s52-%d" % i) for i in range(8)), pub=enc(pubs))
    assert ctx.secret_residue() == 0
    assert pr.verify_batch(proofs, Vs, pub=enc(pubs))
    wrong = list(pubs)
    wrong[6] = pubs[5]
    assert not pr.verify_batch(proofs, Vs, pub=enc(wrong))
    assert pr.verify_batch_each(proofs, Vs, pub=enc(wrong)) == [j != 6 for j in range(8)]


def test_public_chain_on_both_witness_paths(gens256, monkeypatch):
    """o_g = o_{g-1} (v + u_g): the last chain whose program, inputs and public
    inputs k_witness_program stages in LDS, and the first it reads from global
    memory (the counts from witness_program_staged_lds <= 64 KB, restated in the
    helper).  The device witness and the host witness give identical bytes, and
    the batch verifies."""
    import bpperm
    lo, hi = cp.chain_straddle()
    assert cp.witness_program_staged_lds(cp.chain_pub_circuit(lo)) <= cp.K_LDS_MAX
    assert cp.witness_program_staged_lds(cp.chain_pub_circuit(hi)) > cp.K_LDS_MAX
    assert hi == lo + 1 and hi <= 256
    for n in (lo, hi):
        desc, vs, pubs = instances("chainpub%d" % n, 3)
        pr = bpperm.CircuitProver(gens256, desc)
        assert pr.circuit.n_p == 256 and pr.circuit.n_pub == n
        seeds = b"".join(cp.seed32(b"chp-%d" % i) for i in range(3))
        proofs, Vs = pr.prove_batch(enc(vs), None, seeds, pub=enc(pubs))
        assert pr.verify_batch(proofs, Vs, pub=enc(pubs))
        assert pr.verify_batch_each(proofs, Vs, pub=enc(pubs)) == [True] * 3
        monkeypatch.setenv("BPP_CIRCUIT_HOST_WITNESS", "1")
        host = pr.prove_batch(enc(vs), None, seeds, pub=enc(pubs))
        monkeypatch.delenv("BPP_CIRCUIT_HOST_WITNESS")
        assert host == (proofs, Vs), n


@pytest.mark.parametrize("streams", [1, 3])
def test_unsatisfied_public_assert_is_refused_by_name(gens, monkeypatch, streams):
    """Proof 2 of 4 claims that V_0 opens to another value: BPP_ERR_ARG naming
    proof 2 and assert 0, the caller's output buffers untouched, no secret left
    behind."""
    import bpperm
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    desc, vs, pubs = instances("opens", 4)
    pubs[2] = [(vs[2][0] + 1) % L]
    pr = bpperm.CircuitProver(gens, desc)
    seeds = b"".join(cp.seed32(b"upa-%d" % i) for i in range(4))
    pf = ctypes.create_string_buffer(b"\xa5" * (pr.proof_len * 4))
    V = ctypes.create_string_buffer(b"\x5a" * (32 * pr.m * 4))
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc(vs), None, seeds, out=(pf, V), pub=enc(pubs))
    assert e.value.code == 1 and "proof 2" in str(e.value) and "assert 0" in str(e.value)
    assert pf.raw[:pr.proof_len * 4] == b"\xa5" * (pr.proof_len * 4) and V.raw[:32 * pr.m * 4] == b"\x5a" * (32 * pr.m * 4)
    assert pr.ctx.secret_residue() == 0
    pubs[2] = list(vs[2])
    got = pr.prove_batch(enc(vs), None, seeds, pub=enc(pubs))
    assert pr.verify_batch(*got, pub=enc(pubs))


def test_compatibility_both_ways(gens):
    import bpperm
    lib = gens.ctx.lib
    # a circuit without public inputs through the _pub entry points, pub = NULL
    desc, vs, auxs = cr.satisfying("range3", 0)[0], [], []
    for i in range(3):
        _, v, aux = cr.satisfying("range3", i)
        vs.append(v)
        auxs.append(aux)
    seeds = b"".join(cp.seed32(b"cbw-%d" % i) for i in range(3))
    old = bpperm.CircuitProver(gens, desc)
    assert old.circuit.n_pub == 0
    want = old.prove_batch(enc(vs), enc(auxs), seeds)
    assert old.prove_batch(enc(vs), enc(auxs), seeds, pub=[b""] * 3) == want
    proofs, Vs = want
    assert old.verify_batch(proofs, Vs, pub=[b""] * 3) and old.verify_batch(proofs, Vs)
    assert old.verify_batch_each(proofs, Vs, pub=[b""] * 3) == [True] * 3
    assert all(old.verify(p, v, pub=b"") for p, v in zip(proofs, Vs))
    bad_V = [Vs[0], _flip(Vs[1], 3), Vs[2]]
    assert old.verify_batch_each(proofs, bad_V, pub=[b""] * 3) == old.verify_batch_each(proofs, bad_V) == [True, False, True]
    assert not old.verify_batch(proofs, bad_V, pub=[b""] * 3) and not old.verify(proofs[1], bad_V[1], pub=b"")
    # a public circuit through the old prover and the three old verifiers
    pdesc, pvs, ppubs = instances("memberpub2", 3)
    pr = bpperm.CircuitProver(gens, pdesc)
    pp, pv = pr.prove_batch(enc(pvs), None, seeds, pub=enc(ppubs))
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc(pvs), None, seeds)
    assert e.value.code == 1
    for call in (lambda: pr.verify(pp[0], pv[0]), lambda: pr.verify_batch(pp, pv), lambda: pr.verify_batch_each(pp, pv)):
        with pytest.raises(bpperm.BppError) as e:
            call()
        assert e.value.code == 1
    # a non-canonical public scalar: the prover and the three verifiers, ok_out all zero
    nc = [list(row) for row in enc(ppubs)]
    nc[1][1] = L.to_bytes(32, "little")
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc(pvs), None, seeds, pub=nc)
    assert e.value.code == 4
    for call in (lambda: pr.verify(pp[1], pv[1], pub=nc[1]), lambda: pr.verify_batch(pp, pv, pub=nc)):
        with pytest.raises(bpperm.BppError) as e:
            call()
        assert e.value.code == 4
    ok = ctypes.create_string_buffer(b"\x01" * 3)
    rc = lib.bpp_circuit_verify_batch_each_pub(pr.ctx.h, gens.h, pr.circuit.h, 3, pr.label, len(pr.label), b"".join(pp),
                                               b"".join(pv), b"".join(b"".join(r) for r in nc), ok)
    assert rc == 4 and ok.raw[:3] == b"\0\0\0"
    assert pr.verify_batch_each(pp, pv, pub=enc(ppubs)) == [True] * 3


@pytest.mark.parametrize("env", [{"BPP_PROVE_STREAMS": "3"}, {"BPP_PROVE_DEV_V": "0"}, {"BPP_PROVE_DEV_V": "1"}],
                         ids=["streams3", "dev_v0", "dev_v1"])
def test_circuit_pub_bytes_under_switches(ctx, env):
    """The same proofs under BPP_PROVE_STREAMS=3 and both settings of
    BPP_PROVE_DEV_V, each in a child process."""
    want_p, want_v = circuit_pub_child.prove(ctx)
    e = {k: v for k, v in os.environ.items() if k not in ("BPP_PROVE_STREAMS", "BPP_PROVE_DEV_V")}
    e.update(env)
    r = subprocess.run([sys.executable, str(HERE / "circuit_pub_child.py")], capture_output=True, text=True, env=e,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines() if line.startswith(("PROOFS ", "V ")))
    assert out["PROOFS"] == want_p.hex() and out["V"] == want_v.hex()


def test_old_provers_unchanged_after_a_public_circuit_batch(gens):
    """A seeded batch (the golden config-1 proof among it), a deck batch and a
    plain circuit batch give the same bytes before and after a public-circuit
    batch on the same context."""
    import bpperm
    k = 52
    gold = json.loads((HERE / "golden" / "protocol.json").read_text())["config1"]
    pr = bpperm.PermProver(gens, k, label=gold["label"].encode())
    dk = bpperm.DeckProver(gens, k)
    plain = bpperm.CircuitProver(gens, gd.member_of([3, 7, 9]))
    perms = [sr.rand_perm(k, b"opp-%d" % p) for p in range(2)]
    sseeds = b"".join(sr.seed32(b"opp-%d" % p) for p in range(2))
    pv = enc([[3], [9]])
    before = pr.prove_batch([gold["seed"], 12, 13])
    dbefore = dk.prove_batch(perms, sseeds)
    cbefore = plain.prove_batch(pv, None, sseeds)
    assert before[0][0].hex() == gold["proof"] and before[1][0].hex() == "".join(gold["V"])
    desc, vs, pubs = instances("shufflepub52", 3)
    cp_ = bpperm.CircuitProver(gens, desc)
    got = cp_.prove_batch(enc(vs), None, pub=enc(pubs))
    assert cp_.verify_batch(*got, pub=enc(pubs))
    assert pr.prove_batch([gold["seed"], 12, 13]) == before
    assert dk.prove_batch(perms, sseeds) == dbefore
    assert plain.prove_batch(pv, None, sseeds) == cbefore
    assert pr.verify_batch(*before) and dk.verify_batch(*dbefore) and plain.verify_batch(*cbefore)
