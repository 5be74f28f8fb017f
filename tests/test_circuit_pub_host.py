"""bpp_circuit_*_pub without a GPU: create_pub, info, n_pub, matrix (W_U too) and
eval_pub through ctypes against the reference helper (tests/circuit_pub_ref.py)
for every public-input gadget, a heavy and a wide case; the digests' rules; the
refusals and their codes; the entry points' checks that need no device; and the
host C++ (csrc/host/circuit.cpp) with public inputs under ASan + UBSan as a
stand-alone program (tests/c/circuit_pub_check.cpp)."""
import copy
import ctypes
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_pub_ref as cp  # noqa: E402
import circuit_ref as cr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "bulletproof-perm_amd" / "csrc"
L = cp.L
ARG, LEN, NONCANONICAL = 1, 2, 4
CASES = ["opens", "memberpub2", "memberpub13", "sum3", "shufflepub2", "shufflepub3", "shufflepub52", "heavypub",
         "widepub300"]


def ints(bs):
    return [int.from_bytes(b, "little") for b in bs]


def sbs(xs):
    return [cp.sb(x) for x in xs]


@pytest.mark.parametrize("name", CASES)
def test_create_pub_info_matrix_eval_equal_the_helper(name):
    import bpperm
    desc, v, aux, pub = cp.satisfying(name, 0)
    want = cp.compile_program(desc)
    c = bpperm.Circuit(desc)
    assert c.n_pub == desc.n_pub == len(pub) > 0
    assert (c.n_p, c.Q, c.m) == (want.n_p, want.Q, want.m)
    assert c.digest == cp.circuit_digest(desc)
    assert c.proof_len == cp.proof_len(desc)
    for which, W in ((0, want.WL), (1, want.WR), (2, want.WO), (3, want.WV), (5, want.WU)):
        got = [(q, col, int.from_bytes(val, "little")) for q, col, val in c.matrix(which)]
        assert sorted(got) == sorted(W), which
    assert len(want.WU) > 0
    assert [(q, col) for q, col, _ in c.matrix(4)] == [(q, 0) for q in range(want.Q)]
    assert ints(val for _, _, val in c.matrix(4)) == want.c
    pad = [0] * (want.n_p - want.n)
    for i in range(3):  # (0 and l - 1 among the public inputs for i = 1, 2)
        _, v, aux, pub = cp.satisfying(name, i)
        x = cp.rand_scalar(b"hpx-%s-%d" % (name.encode(), i))
        aL, aR, aO, bad = c.eval(sbs(v), sbs(aux), cp.sb(x), pub=sbs(pub))
        wL, wR, wO, wbad = cp.eval_program(desc, v, aux, pub, x)
        assert (ints(aL), ints(aR), ints(aO), bad) == (wL + pad, wR + pad, wO + pad, wbad) and bad == 0
    # a changed public input: the same first failing assert
    bads = []
    for i in {0, len(pub) - 1}:
        for u in (0, L - 1, cp.rand_scalar(b"hpu-%s" % name.encode())):
            if u == pub[i]:
                continue
            pub2 = list(pub)
            pub2[i] = u
            aL, aR, aO, bad = c.eval(sbs(v), sbs(aux), cp.sb(x), pub=sbs(pub2))
            wL, wR, wO, wbad = cp.eval_program(desc, v, aux, pub2, x)
            assert (ints(aL), ints(aR), ints(aO), bad) == (wL + pad, wR + pad, wO + pad, wbad)
            bads.append(bad)
    assert any(bads)  # (not all: a member stays one when another element of its set changes)
    c.close()


def test_heavy_and_wide_are_what_they_say():
    heavy = cp.compile_program(cp.heavy_pub_circuit())
    assert len({i for _, i, _ in heavy.WU}) == 1 and len(heavy.WU) == 13  # 11 defined sides and 2 asserts
    assert sum(1 for q, _, _ in heavy.WU if q >= heavy.Q - 3) == 2
    wide = cp.wide_pub_circuit(300)
    assert (wide.n_pub, wide.n_gates, cp.n_p_of(wide.n_gates)) == (300, 1, 4)
    assert len(cp.compile_program(wide).WU) > 256


def _circuit(desc, n_pub=None):
    import bpperm
    d = copy.copy(desc)
    if n_pub is not None:
        d.n_pub = n_pub
    return bpperm.Circuit(d)


def _code(desc, n_pub=None):
    import bpperm
    with pytest.raises(bpperm.BppError) as e:
        _circuit(desc, n_pub)
    return e.value.code


def test_digests():
    import bpperm
    from bpperm import _lib
    lib = _lib.load()
    b = gd.CircuitBuilder()  # no public term and no wire term: the arrays mean the same under any n_pub
    v = b.input()
    b.mul(v - 3, v - 7)
    b.assert_zero(v * 2 - 6)
    plain = b.build()
    c0 = bpperm.Circuit(plain)
    # create_pub(desc, 0) is create(desc)
    keep = ((ctypes.c_uint32 * len(plain.side_aux))(*plain.side_aux), (ctypes.c_uint32 * len(plain.lc_off))(*plain.lc_off),
            (ctypes.c_uint32 * len(plain.lc_var))(*plain.lc_var), b"".join(plain.lc_coef))
    d = bpperm._CircuitDescC(plain.m_in, plain.n_gates, plain.n_aux, plain.n_asserts, *keep)
    h = ctypes.c_void_p()
    assert lib.bpp_circuit_create_pub(ctypes.byref(d), 0, ctypes.byref(h)) == 0
    dg = ctypes.create_string_buffer(32)
    assert lib.bpp_circuit_info(h, None, None, None, dg) == 0 and lib.bpp_circuit_n_pub(h) == 0
    assert dg.raw == c0.digest == cr.circuit_digest(plain)
    lib.bpp_circuit_destroy(h)
    assert lib.bpp_circuit_n_pub(None) == 0
    c1, c2 = _circuit(plain, 1), _circuit(plain, 2)
    assert (c1.n_pub, c2.n_pub) == (1, 2)
    assert len({c0.digest, c1.digest, c2.digest}) == 3
    for c in (c0, c1, c2):
        assert c.matrix(5) == [] and c.matrix(0) == c0.matrix(0) and c.matrix(3) == c0.matrix(3)


def _set(xs, i, val):
    xs = list(xs)
    xs[i] = val
    return xs


def test_refusals():
    import bpperm
    m = gd.member_of_public(3)  # gate 0 = (v - u_0)(v - u_1), gate 1 = o_0 (v - u_2)
    assert m.lc_var[:2] == [1, 2 + m.m_in] and m.n_pub == 3
    # a public id on a free side
    bad = copy.copy(m)
    bad.side_aux, bad.n_aux = _set(m.side_aux, 0, 0), 1
    assert _code(bad) == ARG
    # wire ids shifted by the wrong n_pub: gate 1's left side then reads its own wire, or an id past the last
    assert _code(m, 2) == ARG
    t = m.lc_off[2]
    assert m.lc_var[t] == 2 + m.m_in + 3 + 2  # o_0
    assert _code(copy.copy(m), 1) == ARG
    far = copy.copy(m)
    far.lc_var = _set(m.lc_var, len(m.lc_var) - 1, 2 + m.m_in + m.n_pub + 3 * m.n_gates)
    assert _code(far) == ARG
    assert _code(m, (1 << 16) + 1) == LEN
    assert _circuit(gd.member_of([3, 7]), 1 << 16).n_pub == 1 << 16
    # the entry points without pub refuse a public circuit
    c = bpperm.Circuit(m)
    with pytest.raises(bpperm.BppError) as e:
        c.eval([cp.sb(1)], [], cp.sb(2))
    assert e.value.code == ARG
    with pytest.raises(bpperm.BppError) as e:  # a non-canonical public input
        c.eval([cp.sb(1)], [], cp.sb(2), pub=[cp.sb(1), L.to_bytes(32, "little"), cp.sb(3)])
    assert e.value.code == NONCANONICAL
    from bpperm import _lib
    lib = _lib.load()
    outs = [ctypes.create_string_buffer(32 * c.n_p) for _ in range(3)]
    ba = ctypes.c_uint32()
    assert lib.bpp_circuit_eval_pub(c.h, cp.sb(1), None, None, cp.sb(2), *outs, ctypes.byref(ba)) == ARG  # pub = NULL
    c.close()


def test_checks_that_need_no_device():
    """Null handles, a missing pub and non-canonical public scalars are refused
    before any device call, and nothing is written."""
    import bpperm
    from bpperm import _lib
    lib = _lib.load()
    desc, v, aux, pub = cp.satisfying("memberpub2", 0)
    c = bpperm.Circuit(desc)
    vb, ub = cp.sb(v[0]), b"".join(sbs(pub))
    pf, V = ctypes.create_string_buffer(b"\xaa" * c.proof_len), ctypes.create_string_buffer(b"\xaa" * 64)
    bad = L.to_bytes(32, "little")

    def prove(ub_):
        return lib.bpp_circuit_prove_batch_pub(None, None, c.h, 1, vb, None, ub_, None, None, b"x", 1, pf, V)

    assert prove(None) == ARG
    assert prove(ub[:32] + bad) == NONCANONICAL
    assert prove(b"\xff" * 32 + ub[32:]) == NONCANONICAL
    assert prove(ub) == ARG  # canonical: now the null context
    assert lib.bpp_circuit_prove_batch(None, None, c.h, 1, vb, None, None, None, b"x", 1, pf, V) == ARG
    assert pf.raw[:c.proof_len] == b"\xaa" * c.proof_len and V.raw[:64] == b"\xaa" * 64
    ok = ctypes.create_string_buffer(b"\x01")
    assert lib.bpp_circuit_verify_pub(None, None, c.h, b"x", 1, pf, c.proof_len, V, ub) == ARG
    assert lib.bpp_circuit_verify_batch_pub(None, None, c.h, 1, b"x", 1, pf, V, ub) == ARG
    assert lib.bpp_circuit_verify_batch_each_pub(None, None, c.h, 1, b"x", 1, pf, V, ub, ok) == ARG and ok.raw[:1] == b"\0"
    assert lib.bpp_circuit_verify_batch_pub(None, None, c.h, 0, b"x", 1, None, None, None) == ARG
    c.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_circuit_pub_host_asan_ubsan(tmp_path):
    exe = tmp_path / "circuit_pub_check"
    srcs = [ROOT / "tests" / "c" / "circuit_pub_check.cpp",
            *(CSRC / "host" / f for f in ("circuit.cpp", "perm_circuit.cpp", "keccak.cpp", "keccak_x8.cpp"))]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-march=x86-64-v3",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC), *map(str, srcs),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, BPP_HOST_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
