"""Large circuits without a GPU: bpp_circuit_create_ex's flags, refusals and
acceptances, the compiled statement of circuits beyond the one-workgroup LDS
bounds against the reference helpers, and the large-circuit tests' own helper
(tests/circuit_large_ref.py prover_scalars) pinned to circuit_ref.prove_circuit
on small cases."""
import ctypes
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_large_ref as lr  # noqa: E402
import circuit_pub_ref as cpr  # noqa: E402
import circuit_ref as cr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402

L = bp.L
ARG, LEN = 1, 2


def ints(bs):
    return [int.from_bytes(b, "little") for b in bs]


def _code(desc, **kw):
    import bpperm
    with pytest.raises(bpperm.BppError) as e:
        bpperm.Circuit(desc, **kw)
    return e.value.code


def test_old_entry_points_refuse_and_large_accepts():
    """683 gates (the LDS witness kernel's bound) and Q = 1508 (the one-table
    kernels') are BPP_ERR_LEN from bpp_circuit_create and _create_pub, as
    before; with LARGE they compile."""
    import bpperm
    from bpperm import _lib
    lib = _lib.load()
    for desc, want in ((cr.chain_circuit(683), (1024, 2 * 683 + 1)), (lr.q1508_circuit(), (512, 1508))):
        assert _code(desc) == LEN
        u32a = lambda xs: (ctypes.c_uint32 * max(len(xs), 1))(*xs)
        arrs = (u32a(desc.side_aux), u32a(desc.lc_off), u32a(desc.lc_var), b"".join(desc.lc_coef))
        d = bpperm._CircuitDescC(desc.m_in, desc.n_gates, desc.n_aux, desc.n_asserts, *arrs)
        h = ctypes.c_void_p()
        assert lib.bpp_circuit_create_pub(ctypes.byref(d), 0, ctypes.byref(h)) == LEN and not h.value
        assert lib.bpp_circuit_create_ex(ctypes.byref(d), 0, 0, ctypes.byref(h)) == LEN and not h.value
        c = bpperm.Circuit(desc, large=True)
        assert (c.n_p, c.Q) == want
        assert c.digest == cr.circuit_digest(desc) and c.proof_len == cr.proof_len(desc)
        c.close()


def test_flags():
    import bpperm
    small = gd.member_of([3, 7, 9])
    for bad in (4, 8, 0x80000000, 0xFFFFFFFF, 1 | 4):
        assert _code(small, flags=bad) == ARG
    assert _code(cr.chain_circuit(683), flags=0) == LEN
    # 2^16 + 1 gates: beyond kMaxGates whatever the flags
    b = gd.CircuitBuilder()
    v = b.input()
    for _ in range((1 << 16) + 1):
        b.free_mul()
    b.assert_zero(v)
    big = b.build()
    assert _code(big, large=True) == LEN and _code(big, tiled=True) == LEN and _code(big) == LEN
    # flags are no part of the statement: one description created four ways
    four = [bpperm.Circuit(small), bpperm.Circuit(small, flags=0), bpperm.Circuit(small, large=True),
            bpperm.Circuit(small, tiled=True)]
    from bpperm import _lib
    lib = _lib.load()
    first = four[0]
    for c in four[1:]:
        assert (c.digest, c.proof_len, c.n_p, c.Q, c.m, c.n_pub) == (first.digest, first.proof_len, first.n_p,
                                                                      first.Q, first.m, first.n_pub)
        for which in range(6):
            assert c.matrix(which) == first.matrix(which), which
    # ... and with public inputs: _create_pub(.., n_pub) against _create_ex(.., n_pub, flags)
    pub = gd.member_of_public(5)
    p0 = bpperm.Circuit(pub)
    for kw in ({"large": True}, {"tiled": True}):
        c = bpperm.Circuit(pub, **kw)
        assert (c.digest, c.proof_len, c.n_pub) == (p0.digest, p0.proof_len, 5)
        assert all(c.matrix(w) == p0.matrix(w) for w in range(6))
        c.close()
    for c in four + [p0]:
        c.close()
    assert lib.bpp_circuit_create_ex(None, 0, 1, None) == ARG


def _break(name, vs, pubs):
    """An instance that fails an assert: (v, pub) with one value moved."""
    v, pub = list(vs[0]), list(pubs[0]) if pubs else None
    v[-1] = (v[-1] + 1) % L
    return v, pub


@pytest.mark.parametrize("name", ["shuffle416", "rangemany18", "chain683"])
def test_large_circuit_equals_the_helper(name):
    """digest, info, the six matrices and eval of a circuit no old entry point
    accepts, against circuit_pub_ref (which is circuit_ref when n_pub = 0)."""
    import bpperm
    desc, vs, auxs, pubs = lr.large_case(name, 3)
    assert _code(desc) == LEN
    want = cpr.compile_program(desc)
    c = bpperm.Circuit(desc, large=True)
    assert (c.n_p, c.Q, c.m, c.n_pub) == (want.n_p, want.Q, want.m, getattr(desc, "n_pub", 0))
    assert c.n_p == {"shuffle416": 1024, "rangemany18": 2048, "chain683": 1024}[name]
    assert c.digest == cpr.circuit_digest(desc)
    if not c.n_pub:
        assert c.digest == cr.circuit_digest(desc)
    assert c.proof_len == cpr.proof_len(desc)
    for which, W in ((0, want.WL), (1, want.WR), (2, want.WO), (3, want.WV), (5, want.WU)):
        got = [(q, col, int.from_bytes(val, "little")) for q, col, val in c.matrix(which)]
        assert sorted(got) == sorted(W), which
    assert ints(val for _, _, val in c.matrix(4)) == want.c
    pad = [0] * (want.n_p - want.n)
    enc = lambda xs: [cr.sb(a) for a in xs]
    for i in range(3):  # (0 and l - 1 are among the values: circuit_large_ref's instances)
        v, aux, pub = vs[i], auxs[i] if auxs else [], pubs[i] if pubs else []
        x = cr.rand_scalar(b"lhx-%s-%d" % (name.encode(), i))
        aL, aR, aO, bad = c.eval(enc(v), enc(aux), cr.sb(x), enc(pub) if pubs else None)
        wL, wR, wO, wbad = cpr.eval_program(desc, v, aux, pub, x)
        assert (ints(aL), ints(aR), ints(aO), bad) == (wL + pad, wR + pad, wO + pad, wbad) and bad == 0
    assert any(0 in vs[i] or (auxs and 0 in auxs[i]) for i in range(3))
    assert any(L - 1 in vs[i] for i in range(3)) or name == "rangemany18"  # (a 64-bit value is never l - 1)
    # a broken instance names its assert
    v2, pub2 = _break(name, vs, pubs)
    aux2 = auxs[0] if auxs else []
    *_, bad = c.eval(enc(v2), enc(aux2), cr.sb(x), enc(pub2) if pubs else None)
    assert bad == cpr.eval_program(desc, v2, aux2, pub2 or [], x)[3]
    assert (bad != 0) == (name != "chain683")  # (the chain asserts nothing)
    if name == "rangemany18":
        assert bad == desc.n_asserts  # the last value's bit sum, the last assert
    c.close()


def test_in_range_many_is_in_range_per_value():
    """count * nbits free gates; per value in_range's asserts; one value is
    in_range itself, array for array."""
    one, many = gd.in_range(6), gd.in_range_many(1, 6)
    for f in ("m_in", "n_gates", "n_aux", "n_asserts", "side_aux", "lc_off", "lc_var", "lc_coef"):
        assert getattr(one, f) == getattr(many, f), f
    assert many.aux_of([37]) == one.aux_of([37])
    d = gd.in_range_many(18, 64)
    assert (d.m_in, d.n_gates, d.n_aux, d.n_asserts) == (18, 18 * 64, 2 * 18 * 64, 18 * (2 * 64 + 1))
    assert all(a != gd.SIDE_LC for a in d.side_aux)
    v = [(1 << 64) - 1 - 3 * j for j in range(18)]
    assert cr.eval_program(d, v, d.aux_of(v), 5)[3] == 0
    v[7] = 1 << 64  # out of range: its hints are those of 0, so value 7's bit-sum assert fails
    assert cr.eval_program(d, v, d.aux_of(v), 5)[3] == 8 * (2 * 64 + 1)
    with pytest.raises(ValueError):
        gd.in_range_many(0, 8)
    with pytest.raises(ValueError):
        gd.in_range_many(2, 253)


@pytest.mark.parametrize("name", ["range3", "heavy", "wide70", "twohalf3"])
def test_prover_scalars_equal_prove_circuit(name):
    """The helper the GPU tests lean on: from prove_circuit's own V and point
    bytes it reproduces prove_circuit's t_hat, tau_x and mu, drawn and supplied
    blindings."""
    for i, with_gammas in ((0, False), (1, True)):
        desc, v, aux = cr.satisfying(name, i)
        seed = cr.seed32(b"ps-%s-%d" % (name.encode(), i))
        gam = [cr.rand_scalar(b"psg-%s-%d" % (name.encode(), j)) for j in range(desc.m_in)] if with_gammas else None
        want = cr.prove_circuit(desc, v, aux, seed, gam, label=b"pin")
        got = lr.prover_scalars(desc, v, aux, seed, gam, None, b"".join(want.V), want.to_bytes(), label=b"pin")
        assert got == (want.t_hat, want.tau_x, want.mu)
        assert lr.proof_fields(want.to_bytes())[1:] == (want.tau_x, want.mu, want.t_hat)
