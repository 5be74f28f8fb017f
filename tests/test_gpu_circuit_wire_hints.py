"""Hints over wires and x on the GPU: the late witness kernels alone against the
plain-Python reference (tests/circuit_wire_hints_ref.py) on hand-built programs
in the staged, global and wide variants, proofs made without aux byte-exact
against the reference provers (tests/circuit_ref.py, tests/circuit_pub_ref.py)
and against the library's own supplied-aux path under the prover's switches,
verified across wire-hinted and plain circuits and inside verify_groups, with
an unsatisfied statement refused by name and nothing secret left behind."""
import ctypes
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_pub_ref as cpr  # noqa: E402
import circuit_ref as cr  # noqa: E402
import circuit_wire_hints_ref as wr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402

pytestmark = pytest.mark.gpu
L = wr.L
sb = wr.sb


def enc(rows):
    return [[sb(x) for x in row] for row in rows]


def ints(row):
    return [int.from_bytes(a, "little") for a in row]


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


# --------------------------------------------------------- the kernels alone

def _program(name):
    if name == "x_program":
        return wr.x_program()
    if name == "bits_program":
        return wr.bits_program()
    n, kind = name.split("-")
    return wr.kernel_program(int(n), kind == "chain")


# name -> (lanes, the program is staged in LDS beside its wires)
KERNEL_CASES = {"1-flat": (64, True), "63-chain": (64, True), "64-flat": (64, True), "65-chain": (128, True),
                "300-flat": (256, False), "300-chain": (256, False), "bits_program": (64, True),
                "x_program": (64, True)}


def _check_kernels(ctx, c, desc, P):
    vs, us = wr.rows(P)
    xs = [wr.rnd(b"gwh-x"), vs[1 % P][5], L - 1][:P]  # (proof 1: x = its v_5, a zero made of x)
    aL, aR, aO, fail = ctx.circuit_witness(c, enc(vs), [sb(x) for x in xs], enc(us))
    pad = [0] * (c.n_p - desc.n_gates)
    for p in range(P):
        _aux, wL, wR, wO, bad = wr.witness(desc, vs[p], xs[p], us[p])
        assert ints(aL[p]) == wL + pad, p
        assert ints(aR[p]) == wR + pad, p
        assert ints(aO[p]) == wO + pad, p
        assert fail[p] == bad, p
    assert ctx.secret_residue() == 0


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_late_witness_kernels_against_reference(ctx, name, P):
    """bpp_debug_circuit_witness (k_hint_aux, then the witness kernel the
    circuit launches) equals the reference: programs of 1, 63, 64, 65 and 300
    gates (64, 64, 64, 128 and 256 lanes; the flat 300-gate program has a level
    of 292 gates, more than its lanes), every op over wires and over x, the
    designed values under every bit arg, early hints mixed in, an aux index
    feeding two sides, a chain where gate g's hint reads o_{g-1}.  The 300-gate
    programs do not fit LDS beside their wires: the global variant.  Proof p's
    inputs are rotated by p.  Nothing secret is left behind."""
    import bpperm
    desc = _program(name)
    lanes, staged = KERNEL_CASES[name]
    c = bpperm.Circuit(desc)
    assert min(256, max(64, (c.n_p + 63) // 64 * 64)) == lanes
    assert (wr.staged_lds(desc) <= wr.K_LDS_MAX) == staged
    _check_kernels(ctx, c, desc, P)


@pytest.mark.parametrize("name", ["65-chain", "x_program"])
def test_late_witness_kernel_wide(ctx, name):
    """BPP_CIRCUIT_TILED: the wide variant, the wires in global memory."""
    import bpperm
    desc = _program(name)
    _check_kernels(ctx, bpperm.Circuit(desc, tiled=True), desc, 3)


def test_witness_hook_on_early_hints_and_refusals(ctx):
    """The hook runs circuits without late hints too (the kernels of before),
    and refuses a circuit whose aux values have no hints."""
    import bpperm
    desc = gd.ascending(3, 4)
    c = bpperm.Circuit(desc)
    v = [3, 9, 10]
    aL, aR, aO, fail = ctx.circuit_witness(c, enc([v]), [sb(5)])
    want = c.eval(enc([v])[0], enc([desc.aux_of(v)])[0], sb(5))
    assert (aL[0], aR[0], aO[0], fail[0]) == want
    with pytest.raises(bpperm.BppError) as e:
        ctx.circuit_witness(bpperm.Circuit(desc, hints=False), enc([v]), [sb(5)])
    assert e.value.code == 1
    late = bpperm.Circuit(gd.not_among(2))
    with pytest.raises(bpperm.BppError) as e:
        ctx.circuit_hints(late, enc([[1, 2, 3]]))  # (k_hint_aux alone has no x)
    assert e.value.code == 1
    with pytest.raises(bpperm.BppError) as e:
        ctx.circuit_witness(late, enc([[1, 2, 3]]), [L.to_bytes(32, "little")])
    assert e.value.code == 4


# ------------------------------------------ bytes against the reference provers

def inv_of_x():
    """(x - v_0) * (x - v_0)^-1 = 1, the inverse a hint over x: what no caller
    can supply."""
    b = gd.CircuitBuilder()
    v = b.input()
    b.assert_zero(b.mul(b.challenge - v, b.derived(gd.HINT_INV, b.challenge - v))[2] - 1)
    return b.build()


def bj(ranks):
    S = sum(min(r, 10) for r in ranks)
    return S + (10 if 1 in ranks and S <= 11 else 0)


# name -> (description, three satisfied instances, their public inputs or None)
SMALL = {"max_of(2, 2)": (gd.max_of(2, 2), [[0, 3, 3], [2, 1, 2], [3, 3, 3]], None),
         "max_of(3, 3)": (gd.max_of(3, 3), [[1, 7, 3, 7], [0, 0, 0, 0], [6, 2, 5, 6]], None),
         "not_among(2)": (gd.not_among(2), [[5, 9, 4], [0, L - 1, 1], [2**252, 1, 2]], None),
         "blackjack_total(2)": (gd.blackjack_total(2), [[1, 13], [1, 1], [9, 7]], [[21], [12], [16]]),
         "inv_of_x": (inv_of_x(), [[5], [0], [L - 1]], None)}


def ref_x(desc, v, seed, gammas, pub):
    """x_perm of the reference transcript: the digest, the public inputs, then
    V_0..V_{m_in-1} over the reference draws (supplied gammas in their place)."""
    m_in = desc.m_in
    n_p = cr.n_p_of(desc.n_gates)
    g, h = cr.pedersen_gens_default()
    gamma = [cr.indexed_scalar(seed, j) for j in range(m_in)]
    if gammas is not None:
        gamma = [x % L for x in gammas]
    tr = cpr._transcript(desc, n_p, b"bp-perm", pub) if pub is not None else cr._transcript(desc, n_p, b"bp-perm")
    for j in range(m_in):
        tr.append_point(b"V", cr.bp.enc(cr.bp.msm([v[j] % L, gamma[j]], [g, h])))
    return tr.challenge_scalar(b"x_perm")


def ref_prove(desc, v, seed, gammas, pub):
    """The reference prover over the reference-derived aux."""
    aux = wr.hint_eval_x(desc, v, ref_x(desc, v, seed, gammas, pub), pub)
    if pub is not None:
        return aux, cpr.prove_circuit(desc, v, aux, pub, seed, gammas)
    return aux, cr.prove_circuit(desc, v, aux, seed, gammas)


@pytest.mark.parametrize("with_gammas", [False, True], ids=["drawn", "supplied"])
@pytest.mark.parametrize("name", list(SMALL))
def test_wire_hinted_bytes_vs_reference_prover(gens, name, with_gammas):
    """prove_batch(v) with no aux: V and proof bytes equal the reference
    prover's over the reference-derived aux, three proofs a call; the three
    verifiers accept."""
    import bpperm
    desc, vs, pubs = SMALL[name]
    tag = name.encode()
    seeds = [cr.seed32(b"gwh-%s-%d" % (tag, i)) for i in range(3)]
    gam = None
    if with_gammas:
        gam = [[cr.rand_scalar(b"gwhg-%s-%d-%d" % (tag, i, j)) for j in range(desc.m_in)] for i in range(3)]
        gam[1][0], gam[2][-1] = 0, L - 1
    # (max_of(2, 2) has one step, over M_0 = v_0: no late hint, the new entry point all the same)
    pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, wire_hints=True))
    assert pr.circuit.has_hints and (desc.hints.wire or name == "max_of(2, 2)")
    pub = enc(pubs) if pubs else None
    proofs, Vs = pr.prove_batch(enc(vs), None, b"".join(seeds), enc(gam) if gam else None, pub=pub)
    for i in range(3):
        _aux, want = ref_prove(desc, vs[i], seeds[i], gam[i] if gam else None, pubs[i] if pubs else None)
        assert Vs[i] == b"".join(want.V), i
        assert proofs[i] == want.to_bytes(), i
        assert pr.verify(proofs[i], Vs[i], pub=pub[i] if pub else None)
    assert pr.verify_batch(proofs, Vs, pub=pub)
    assert pr.verify_batch_each(proofs, Vs, pub=pub) == [True] * 3


# ------------------------------------------------- derived against supplied aux

def _hands(name):
    """desc, five satisfied instances, their public inputs or None."""
    if name == "max_of(4, 5)":
        return gd.max_of(4, 5), [[0, 0, 0, 0, 0], [31, 30, 29, 28, 31], [1, 2, 3, 4, 4], [7, 31, 7, 0, 31],
                                 [16, 15, 17, 16, 17]], None
    if name == "not_among(6)":
        return gd.not_among(6), [[1, 2, 3, 4, 5, 6, 7], [0, L - 1, 1, L - 2, 2**252, 2, 3]] + [
            [wr.rnd(b"na6-%d-%d" % (p, j)) for j in range(7)] for p in range(3)], None
    if name == "blackjack_total(3)":
        hands = [[1, 1, 1], [1, 10, 13], [1, 5, 5], [9, 9, 3], [13, 12, 11]]
        return gd.blackjack_total(3), hands, [[bj(h)] for h in hands]
    raise KeyError(name)


def _both_ways(pr, desc, vs, pubs, tag):
    """(derived, supplied): the supplied aux is the reference's, at the x of the
    reference transcript under the same seeds."""
    seeds = [cr.seed32(b"%s-%d" % (tag, i)) for i in range(len(vs))]
    pub = enc(pubs) if pubs else None
    derived = pr.prove_batch(enc(vs), None, b"".join(seeds), pub=pub)
    aux = [wr.hint_eval_x(desc, v, ref_x(desc, v, seeds[i], None, pubs[i] if pubs else None), pubs[i] if pubs else None)
           for i, v in enumerate(vs)]
    supplied = pr.prove_batch(enc(vs), enc(aux), b"".join(seeds), pub=pub)
    return derived, supplied


@pytest.mark.parametrize("name", ["max_of(4, 5)", "not_among(6)", "blackjack_total(3)"])
def test_derived_equals_supplied(gens, name):
    """prove_batch(v) equals prove_batch(v, reference aux) byte for byte under
    the same seeds (the supplied-aux path is existing code), and verifies."""
    import bpperm
    desc, vs, pubs = _hands(name)
    pr = bpperm.CircuitProver(gens, desc)
    derived, supplied = _both_ways(pr, desc, vs, pubs, b"ds-" + name.encode())
    assert derived == supplied
    assert pr.verify_batch(*derived, pub=enc(pubs) if pubs else None)


def test_derived_equals_supplied_tiled(gens):
    import bpperm
    desc, vs, pubs = _hands("max_of(4, 5)")
    pr = bpperm.CircuitProver(gens, bpperm.Circuit(desc, tiled=True))
    derived, supplied = _both_ways(pr, desc, vs, pubs, b"ds-tiled")
    assert derived == supplied and pr.verify_batch(*derived)
    assert derived == _both_ways(bpperm.CircuitProver(gens, desc), desc, vs, pubs, b"ds-tiled")[0]


def test_derived_equals_supplied_streams3(gens, monkeypatch):
    """BPP_PROVE_STREAMS=3: every sub-batch derives its own rows."""
    import bpperm
    desc, vs, pubs = _hands("blackjack_total(3)")
    pr = bpperm.CircuitProver(gens, desc)
    want = _both_ways(pr, desc, vs, pubs, b"ds-st")[1]
    monkeypatch.setenv("BPP_PROVE_STREAMS", "3")
    derived, supplied = _both_ways(pr, desc, vs, pubs, b"ds-st")
    assert derived == supplied == want


def test_derived_equals_supplied_host_witness(gens, monkeypatch):
    """BPP_CIRCUIT_HOST_WITNESS=1: the host witness over bpp_circuit_hint_eval_x's
    code, also for a hint over x."""
    import bpperm
    for name in ("max_of(4, 5)", "inv_of_x"):
        desc, vs, pubs = _hands(name) if name != "inv_of_x" else SMALL[name]
        pr = bpperm.CircuitProver(gens, desc)
        monkeypatch.delenv("BPP_CIRCUIT_HOST_WITNESS", raising=False)
        want = _both_ways(pr, desc, vs, pubs, b"ds-hw")[0]
        monkeypatch.setenv("BPP_CIRCUIT_HOST_WITNESS", "1")
        derived, supplied = _both_ways(pr, desc, vs, pubs, b"ds-hw")
        assert derived == supplied == want
        assert pr.ctx.secret_residue() == 0


# ------------------------------------------------------- cross-verification

def test_wire_hinted_and_plain_circuits_verify_each_other(gens):
    import bpperm
    desc, vs, pubs = _hands("not_among(6)")
    hinted = bpperm.CircuitProver(gens, desc)
    plain = bpperm.CircuitProver(gens, bpperm.Circuit(desc, hints=False))
    assert hinted.circuit.has_hints and not plain.circuit.has_hints
    seeds = b"".join(cr.seed32(b"wxv-%d" % i) for i in range(len(vs)))
    a = hinted.prove_batch(enc(vs), None, seeds)
    b = plain.prove_batch(enc(vs), enc([desc.aux_of(v) for v in vs]), seeds)
    assert a == b
    assert plain.verify_batch(*a) and hinted.verify_batch(*b)
    assert plain.verify_batch_each(*a) == [True] * len(vs) and hinted.verify(b[0][0], b[1][0])
    # a wire-hinted group beside a plain one, a public-input one and a two-half group in one merged MSM
    bdesc, bvs, bpubs = _hands("blackjack_total(3)")
    black = bpperm.CircuitProver(gens, bdesc)
    bp_, bv = black.prove_batch(enc(bvs), None, pub=enc(bpubs))
    two = bpperm.PermProver(gens, 3)
    tp, tv = two.prove_batch([1, 2])
    assert bpperm.verify_groups(gens, [(hinted, *a), (two, tp, tv), (black, bp_, bv, enc(bpubs)), (plain, *b)])
    bad = (a[0][:1] + a[0][:1] + a[0][2:], a[1])  # proof 1 replaced by proof 0
    assert bpperm.verify_groups(gens, [(two, tp, tv), (hinted, *bad)], each=True) == [
        [True, True], [True, False, True, True, True]]


# --------------------------------------------------------- refusals, residue

@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("name", ["not_among", "max_of"])
def test_unsatisfied_statement_is_refused_by_name(gens, monkeypatch, name, streams):
    """A repeated card (the product is 0, its inverse hint 0) or a wrong maximum
    as proof 1 of 3: BPP_ERR_ARG naming proof 1 and the assert, the outputs
    untouched, nothing secret left, and the next valid batch verifies."""
    import bpperm
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    if name == "not_among":
        desc, vs, fix, bad = gd.not_among(3), [[5, 9, 1, 2], [7, 1, 7, 2], [1, 0, 2, 3]], [7, 1, 8, 2], 0
    else:
        desc = gd.max_of(3, 3)
        vs, fix, bad = [[1, 7, 3, 7], [4, 2, 6, 5], [0, 0, 0, 0]], [4, 2, 6, 6], desc.n_asserts - 1
    pr = bpperm.CircuitProver(gens, desc)
    seeds = b"".join(cr.seed32(b"wuh-%d" % i) for i in range(3))
    pf = ctypes.create_string_buffer(b"\xa5" * (pr.proof_len * 3))
    V = ctypes.create_string_buffer(b"\x5a" * (32 * pr.m * 3))
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc(vs), None, seeds, out=(pf, V))
    assert e.value.code == 1 and "proof 1" in str(e.value) and "assert %d " % bad in str(e.value)
    assert pf.raw[:pr.proof_len * 3] == b"\xa5" * (pr.proof_len * 3) and V.raw[:32 * pr.m * 3] == b"\x5a" * (32 * pr.m * 3)
    assert pr.ctx.secret_residue() == 0
    vs[1] = fix
    got = pr.prove_batch(enc(vs), None, seeds)
    assert pr.verify_batch(*got)
    assert pr.ctx.secret_residue() == 0


def test_supplied_aux_is_used_as_given(gens):
    """aux != NULL on a wire-hinted circuit: the kernels of before read it, and a
    wrong value fails its assert."""
    import bpperm
    desc = gd.not_among(2)
    pr = bpperm.CircuitProver(gens, desc)
    v = [5, 9, 4]
    with pytest.raises(bpperm.BppError) as e:
        pr.prove_batch(enc([v]), enc([[3]]))
    assert e.value.code == 1 and "assert 0" in str(e.value)
    got = pr.prove_batch(enc([v]), enc([desc.aux_of(v)]))
    assert pr.verify_batch(*got)
