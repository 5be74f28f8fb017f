"""Circuit hints on the GPU: k_hint_aux alone against the plain-Python reference
(tests/circuit_hints_ref.py) on hand-built programs, proofs made without aux
byte-exact against the reference prover (tests/circuit_ref.py) and against the
library's own supplied-aux path, on every witness kernel and under the prover's
switches, verified across hinted and plain circuits, with an unsatisfied
statement refused by name and the derived values wiped."""
import ctypes
import hashlib
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_hints_ref as hr  # noqa: E402
import circuit_ref as cr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402

pytestmark = pytest.mark.gpu
L = hr.L


def sb(x):
    return (x % L).to_bytes(32, "little")


def enc(rows):
    return [[sb(x) for x in row] for row in rows]


def rnd(tag):
    return int.from_bytes(hashlib.sha512(tag).digest(), "little") % L


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


# --------------------------------------------------------- the kernel alone

# inputs of the hand-built programs: v_0..v_5 the designed w of BIT / NOT_BIT,
# v_0, v_1, v_6, v_2, v_5 those of INV / IS_ZERO; u_0..u_2 public
V_ROW = [0, 1, L - 1, 2**252, 2**252 - 1, rnd(b"gh-v5"), 2, rnd(b"gh-v7")]
U_ROW = [rnd(b"gh-u0"), L - 1, 0]
M_IN, N_PUB = len(V_ROW), len(U_ROW)
vid = lambda j: 1 + j
uid = lambda i: 2 + M_IN + i
C1, C2 = rnd(b"gh-c1"), rnd(b"gh-c2")


def hint_pool():
    """Every op over its designed values, ops interleaved (so the op-grouped lane
    order differs from the hint order everywhere)."""
    bits = [(op, arg, [(vid(j), 1)]) for arg in (0, 31, 32, 63, 64, 252) for j in range(6)
            for op in (hr.BIT, hr.NOT_BIT)]
    invs = [(op, 0, [(vid(j), 1)]) for j in (0, 1, 6, 2, 5) for op in (hr.INV, hr.IS_ZERO)]
    invs += [(hr.INV, 0, [(vid(5), 1), (vid(7), L - 1)]), (hr.IS_ZERO, 0, [(vid(1), 1), (vid(2), 1)]),  # 1 + (l - 1) = 0
             (hr.INV, 0, []), (hr.IS_ZERO, 0, []), (hr.INV, 0, [(0, 2), (vid(6), L - 1)])]                # 2 - v_6 = 0
    vals = [(hr.VALUE, 0, t) for t in (
        [(vid(5), 1)], [(vid(5), L - 1)], [(vid(5), C1)], [(uid(0), 1)], [(uid(0), L - 1)], [(uid(0), C2)],
        [], [(0, 1)], [(0, L - 1)], [(0, C1)], [(vid(2), L - 1)], [(vid(3), C1), (vid(4), C2)],
        [(0, C2), (vid(2), 1), (vid(5), C1), (vid(7), L - 1), (uid(0), C2), (uid(1), 1), (uid(2), C1)])]
    vals += [(hr.BIT, 252, [(uid(1), 1)]), (hr.NOT_BIT, 0, [(uid(2), 1)]), (hr.BIT, 100, [(vid(5), C1), (uid(0), 1)])]
    pool, lists = [], [bits, invs, vals]
    while any(lists):
        for l in lists:
            if l:
                pool.append(l.pop(0))
            if l is bits and l:  # (bits are most of the pool)
                pool.append(l.pop(0))
    return pool


POOL = hint_pool()


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n_aux", [1, 63, 64, 65, 256, 257])
def test_hint_kernel_against_reference(ctx, n_aux, P):
    """bpp_debug_circuit_hints (the device kernel alone) equals the reference on
    the first n_aux hints of the pool (cycled, starting at another hint for each
    size, so every size sees every op): one lane, a wave less one, a wave, a
    wave and one, a block, a block and one.  Proof p's inputs are the designed
    values rotated by p.  Nothing secret is left behind."""
    import bpperm
    assert len(POOL) >= 100 and {h[0] for h in POOL} == {0, 1, 2, 3, 4}
    start = {1: 2, 63: 0, 64: 11, 65: 40, 256: 0, 257: 7}[n_aux]
    hints = [POOL[(start + t) % len(POOL)] for t in range(n_aux)]
    desc = hr.hand_built(M_IN, N_PUB, hints)
    c = bpperm.Circuit(desc)
    assert c.has_hints and c.n_aux == n_aux
    # (the BIT / INV inputs v_0..v_6 rotate among themselves, v_7 stays random)
    vs = [[V_ROW[(j + p) % 7] for j in range(7)] + [V_ROW[7] + p] for p in range(P)]
    us = [[U_ROW[(i + p) % N_PUB] for i in range(N_PUB)] for p in range(P)]
    got = ctx.circuit_hints(c, enc(vs), enc(us))
    for p in range(P):
        want = hr.hint_eval(desc, vs[p], us[p])
        assert [int.from_bytes(a, "little") for a in got[p]] == want, p
        assert got[p] == c.hint_eval(enc([vs[p]])[0], enc([us[p]])[0])
    assert ctx.secret_residue() == 0


def test_hint_kernel_covers_the_designed_values():
    """The pool really holds the cases the kernel test is about."""
    bit_args = {(h[1], h[2][0][0]) for h in POOL if h[0] in (hr.BIT, hr.NOT_BIT) and len(h[2]) == 1 and h[2][0][0] <= 6}
    assert bit_args == {(a, vid(j)) for a in (0, 31, 32, 63, 64, 252) for j in range(6)}
    for op in (hr.INV, hr.IS_ZERO):
        assert {h[2][0][0] for h in POOL if h[0] == op and len(h[2]) == 1} == {vid(j) for j in (0, 1, 6, 2, 5)}
    assert any(h[0] == hr.VALUE and not h[2] for h in POOL)


# ------------------------------------------- bytes against the reference prover

SMALL = {"not_equal": (gd.not_equal(), [[5, 9], [0, L - 1], [2**252, 1]]),
         "less_than3": (gd.less_than(3), [[0, 7], [6, 7], [2, 5]]),
         "ascending2_2": (gd.ascending(2, 2), [[0, 1], [2, 3], [0, 3]])}


@pytest.mark.parametrize("with_gammas", [False, True], ids=["drawn", "supplied"])
@pytest.mark.parametrize("name", list(SMALL))
def test_hinted_bytes_vs_reference_prover(gens, name, with_gammas):
    """prove_batch(v) with no aux: V and proof bytes equal the reference prover's
    over aux_of(v), three proofs a call; the three verifiers accept."""
    import bpperm
    desc, vs = SMALL[name]
    seeds = [cr.seed32(b"gh-%s-%d" % (name.encode(), i)) for i in range(3)]
    gam = None
    if with_gammas:
        gam = [[cr.rand_scalar(b"ghg-%s-%d-%d" % (name.encode(), i, j)) for j in range(desc.m_in)] for i in range(3)]
        gam[1][0], gam[2][-1] = 0, L - 1
    pr = bpperm.CircuitProver(gens, desc)
    assert pr.circuit.has_hints
    proofs, Vs = pr.prove_batch(enc(vs), None, b"".join(seeds), enc(gam) if gam else None)
    for i in range(3):
        want = cr.prove_circuit(desc, vs[i], desc.aux_of(vs[i]), seeds[i], gam[i] if gam else None)
        assert Vs[i] == b"".join(want.V), i
        assert proofs[i] == want.to_bytes(), i
        assert pr.verify(proofs[i], Vs[i])
    assert pr.verify_batch(proofs, Vs)
    assert pr.verify_batch_each(proofs, Vs) == [True] * 3


# ------------------------------------------------- hinted against supplied aux

def _hands(name):
    """desc and five satisfied instances (the values at the range's edges among them)."""
    if name == "in_range32":
        return gd.in_range(32), [[0], [2**32 - 1], [1], [2**31], [rnd(b"ir32") % 2**32]]
    if name == "distinct5":
        return gd.distinct(5), [[1, 2, 3, 4, 5], [0, L - 1, 1, L - 2, 2**252]] + [
            [rnd(b"d5-%d-%d" % (p, j)) for j in range(5)] for p in range(3)]
    if name == "ascending5_6":
        return gd.ascending(5, 6), [[0, 1, 2, 3, 4], [59, 60, 61, 62, 63], [0, 31, 32, 33, 63], [3, 9, 27, 40, 52],
                                    [1, 2, 4, 8, 16]]
    if name == "in_range_many3_11":
        return gd.in_range_many(3, 11), [[0, 2047, 1024], [1, 2, 3], [2047, 2047, 2047], [1023, 0, 5], [7, 77, 777]]
    raise KeyError(name)


def _both_ways(pr, desc, vs, tag, pub=None):
    seeds = b"".join(cr.seed32(b"%s-%d" % (tag, i)) for i in range(len(vs)))
    hinted = pr.prove_batch(enc(vs), None, seeds, pub=pub)
    supplied = pr.prove_batch(enc(vs), enc([desc.aux_of(v) for v in vs]), seeds, pub=pub)
    return hinted, supplied


@pytest.mark.parametrize("name", ["in_range32", "distinct5", "ascending5_6", "in_range_many3_11"])
def test_hinted_equals_supplied(gens, name):
    """prove_batch(v) equals prove_batch(v, aux_of(v)) byte for byte under the
    same seeds (the supplied-aux path is existing code), and verifies."""
    import bpperm
    desc, vs = _hands(name)
    pr = bpperm.CircuitProver(gens, desc)
    hinted, supplied = _both_ways(pr, desc, vs, b"hs-" + name.encode())
    assert hinted == supplied
    assert pr.verify_batch(*hinted)


def test_hinted_equals_supplied_tiled(gens):
    """BPP_CIRCUIT_TILED: k_witness_program_wide reads the derived array."""
    import bpperm
    desc, vs = _hands("ascending5_6")
    pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, tiled=True))
    assert pr.circuit.has_hints
    hinted, supplied = _both_ways(pr, desc, vs, b"hs-tiled")
    assert hinted == supplied and pr.verify_batch(*hinted)
    assert hinted == _both_ways(bpperm.CircuitProver(gens, desc), desc, vs, b"hs-tiled")[0]


def test_hinted_equals_supplied_global_witness(ctx):
    """A program too large to stage in LDS beside its wires (in_range(252), 252
    gates, 757 asserts): k_witness_program_global reads the derived array."""
    import bpperm
    g = bpperm.Gens(ctx, 256)
    try:
        desc = gd.in_range(252)
        vs = [[2**252 - 1], [0], [rnd(b"ir252") % 2**252]]
        pr = bpperm.CircuitProver(g, desc)
        hinted, supplied = _both_ways(pr, desc, vs, b"hs-global")
        assert hinted == supplied and pr.verify_batch(*hinted)
    finally:
        g.close()


def test_hinted_equals_supplied_streams3(gens, monkeypatch):
    """BPP_PROVE_STREAMS=3: every sub-batch derives its own rows."""
    import bpperm
    desc, vs = _hands("distinct5")
    pr = bpperm.CircuitProver(gens, desc)
    want = _both_ways(pr, desc, vs, b"hs-st")[1]
    monkeypatch.setenv("BPP_PROVE_STREAMS", "3")
    hinted, supplied = _both_ways(pr, desc, vs, b"hs-st")
    assert hinted == supplied == want


def test_hinted_equals_supplied_host_witness(gens, monkeypatch):
    """BPP_CIRCUIT_HOST_WITNESS=1: the host witness over the host hints."""
    import bpperm
    desc, vs = _hands("ascending5_6")
    pr = bpperm.CircuitProver(gens, desc)
    want = _both_ways(pr, desc, vs, b"hs-hw")[0]
    monkeypatch.setenv("BPP_CIRCUIT_HOST_WITNESS", "1")
    hinted, supplied = _both_ways(pr, desc, vs, b"hs-hw")
    assert hinted == supplied == want
    assert pr.ctx.secret_residue() == 0


def above_public(nbits=4):
    """0 < v_0 - u_0 <= 2^nbits and v_1 != u_1: hints over public inputs."""
    b = gd.CircuitBuilder()
    v, u = b.inputs(2), b.publics(2)
    gd._range_bits(b, v[0] - u[0] - 1, nbits)
    b.assert_zero(b.mul(v[1] - u[1], b.hint(gd.HINT_INV, v[1] - u[1]))[2] - 1)
    return b.build()


def test_hinted_equals_supplied_public_inputs(gens):
    """A circuit whose hints read u_i, three proofs with different public
    inputs; the supplied aux is the host hints' (bpp_circuit_hint_eval)."""
    import bpperm
    desc = above_public()
    assert desc.hints is not None and desc.n_pub == 2
    pr = bpperm.CircuitProver(gens, desc)
    vs = [[9, 4], [L - 1, 0], [rnd(b"ap-v") + 16, 7]]
    us = [[8, 5], [L - 17, L - 1], [rnd(b"ap-v"), rnd(b"ap-u")]]
    auxs = [pr.circuit.hint_eval(enc([v])[0], enc([u])[0]) for v, u in zip(vs, us)]
    assert [[int.from_bytes(a, "little") for a in row] for row in auxs] == [
        hr.hint_eval(desc, v, u) for v, u in zip(vs, us)]
    seeds = b"".join(cr.seed32(b"hs-pub-%d" % i) for i in range(3))
    hinted = pr.prove_batch(enc(vs), None, seeds, pub=enc(us))
    supplied = pr.prove_batch(enc(vs), auxs, seeds, pub=enc(us))
    assert hinted == supplied
    assert pr.verify_batch(*hinted, pub=enc(us))
    assert not pr.verify_batch(*hinted, pub=enc(us[1:] + us[:1]))


# ------------------------------------------------------- cross-verification

def test_hinted_and_plain_circuits_verify_each_other(gens):
    import bpperm
    desc, vs = _hands("distinct5")
    hinted = bpperm.CircuitProver(gens, desc)
    plain = bpperm.CircuitProver(gens, bpperm.Circuit(desc, hints=False))
    assert hinted.circuit.has_hints and not plain.circuit.has_hints
    seeds = b"".join(cr.seed32(b"xv-%d" % i) for i in range(len(vs)))
    a = hinted.prove_batch(enc(vs), None, seeds)
    b = plain.prove_batch(enc(vs), enc([desc.aux_of(v) for v in vs]), seeds)
    assert a == b
    assert plain.verify_batch(*a) and hinted.verify_batch(*b)
    assert plain.verify_batch_each(*a) == [True] * len(vs) and hinted.verify(b[0][0], b[1][0])
    # a hinted group beside a plain one and a two-half group in one merged MSM
    two = bpperm.PermProver(gens, 3)
    tp, tv = two.prove_batch([1, 2])
    assert bpperm.verify_groups(gens, [(hinted, *a), (two, tp, tv), (plain, *b)])
    bad = (a[0][:1] + a[0][:1] + a[0][2:], a[1])  # proof 1 replaced by proof 0
    assert bpperm.verify_groups(gens, [(two, tp, tv), (hinted, *bad)], each=True) == [
        [True, True], [True, False, True, True, True]]


# --------------------------------------------------------- refusals, residue

@pytest.mark.parametrize("streams", [1, 3])
def test_unsatisfied_hinted_statement_is_refused_by_name(gens, monkeypatch, streams):
    """not_equal with equal cards as proof 1 of 3: the hint is 0, o - 1 != 0.
    BPP_ERR_ARG naming proof 1 and assert 0, the outputs untouched, nothing
    secret left, and the next valid batch gives the supplied path's bytes."""
    import bpperm
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    desc = gd.not_equal()
    pr = bpperm.CircuitProver(gens, desc)
    vs = [[5, 9], [7, 7], [1, 0]]
    seeds = b"".join(cr.seed32(b"uh-%d" % i) for i in range(3))
    pf = ctypes.create_string_buffer(b"\xa5" * (pr.proof_len * 3))
    V = ctypes.create_string_buffer(b"\x5a" * (32 * pr.m * 3))
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc(vs), None, seeds, out=(pf, V))
    assert e.value.code == 1 and "proof 1" in str(e.value) and "assert 0" in str(e.value)
    assert pf.raw[:pr.proof_len * 3] == b"\xa5" * (pr.proof_len * 3) and V.raw[:32 * pr.m * 3] == b"\x5a" * (32 * pr.m * 3)
    assert pr.ctx.secret_residue() == 0
    vs[1] = [7, 8]
    got = pr.prove_batch(enc(vs), None, seeds)
    assert got == pr.prove_batch(enc(vs), enc([desc.aux_of(v) for v in vs]), seeds)
    assert pr.verify_batch(*got)


@pytest.mark.parametrize("streams", [1, 3])
def test_hinted_batch_leaves_no_secret_bytes(ctx, gens, monkeypatch, streams):
    import bpperm
    desc, vs = _hands("ascending5_6")
    pr = bpperm.CircuitProver(gens, desc)
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    bpperm.PermProver(gens, 52).prove_batch([3, 4, 5])  # a test-hook batch leaves its secrets in place
    assert ctx.secret_residue() > 0
    got = pr.prove_batch(enc(vs), None, b"".join(cr.seed32(b"hres-%d" % i) for i in range(len(vs))))
    assert ctx.secret_residue() == 0
    assert pr.verify_batch(*got)


def test_no_aux_without_hints_still_raises(gens):
    """On a circuit without hints, aux=None with n_aux > 0 is refused as before:
    by the binding, and by the library (BPP_ERR_ARG, nothing written)."""
    import bpperm
    desc = gd.in_range(3)
    pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, hints=False))
    with pytest.raises(ValueError):
        pr.prove_batch(enc([[5]]), None)
    pf, V = ctypes.create_string_buffer(b"\xa5" * pr.proof_len), ctypes.create_string_buffer(b"\x5a" * 64)
    rc = pr.ctx.lib.bpp_circuit_prove_batch(pr.ctx.h, gens.h, pr.circuit.h, 1, sb(5), None, None, None, b"x", 1, pf, V)
    assert rc == 1 and pf.raw[:pr.proof_len] == b"\xa5" * pr.proof_len and V.raw[:64] == b"\x5a" * 64
    # and a supplied aux is used as given on a hinted circuit: a wrong one fails its assert
    hp = bpperm.CircuitProver(gens, desc)
    wrong = desc.aux_of([4])
    with pytest.raises(bpperm.BppError) as e:
        hp.prove_batch(enc([[5]]), enc([wrong]))
    assert e.value.code == 1 and "assert 6" in str(e.value)
