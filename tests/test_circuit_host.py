"""bpp_circuit_* without a GPU: create, info, matrix and eval through ctypes
against the reference helper (tests/circuit_ref.py) for every gadget, every
refusal of bpp_circuit_create and its code, the prover's checks that need no
device, and the host C++ (csrc/host/circuit.cpp) under ASan + UBSan as a
stand-alone program (tests/c/circuit_check.cpp)."""
import copy
import ctypes
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_ref as cr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "bulletproof-perm_amd" / "csrc"
L = bp.L
ARG, LEN, NONCANONICAL = 1, 2, 4
CASES = ["member2", "member13", "twohalf2", "twohalf3", "twohalf52", "range3", "range6", "multiset4", "heavy",
         "wide70", "chain300"]


def ints(bs):
    return [int.from_bytes(b, "little") for b in bs]


@pytest.mark.parametrize("name", CASES)
def test_create_info_matrix_eval_equal_the_helper(name):
    import bpperm
    desc, v, aux = cr.satisfying(name, 0)
    want = cr.compile_program(desc)
    c = bpperm.Circuit(desc)
    assert (c.n_p, c.Q, c.m) == (want.n_p, want.Q, want.m)
    assert c.digest == cr.circuit_digest(desc)
    assert c.proof_len == cr.proof_len(desc)
    for which, W in enumerate((want.WL, want.WR, want.WO, want.WV)):
        got = [(q, col, int.from_bytes(val, "little")) for q, col, val in c.matrix(which)]
        assert sorted(got) == sorted(W), which
    assert [(q, col) for q, col, _ in c.matrix(4)] == [(q, 0) for q in range(want.Q)]
    assert ints(val for _, _, val in c.matrix(4)) == want.c
    for i in range(2):
        _, v, aux = cr.satisfying(name, i)
        x = cr.rand_scalar(b"hx-%s-%d" % (name.encode(), i))
        aL, aR, aO, bad = c.eval([cr.sb(a) for a in v], [cr.sb(a) for a in aux], cr.sb(x))
        wL, wR, wO, wbad = cr.eval_program(desc, v, aux, x)
        pad = [0] * (want.n_p - want.n)
        assert (ints(aL), ints(aR), ints(aO), bad) == (wL + pad, wR + pad, wO + pad, wbad) and bad == 0
    # an unsatisfied instance: the same first failing assert
    v2 = [(v[0] + 2) % L] + list(v[1:])
    *_, bad = c.eval([cr.sb(a) for a in v2], [cr.sb(a) for a in aux], cr.sb(x))
    assert bad == cr.eval_program(desc, v2, aux, x)[3]
    assert (bad != 0) == (name != "chain300")  # (the chain asserts nothing)
    c.close()


def _variant(desc, **kw):
    d = copy.copy(desc)
    for k, val in kw.items():
        setattr(d, k, val)
    return d


def _set(xs, i, val):
    xs = list(xs)
    xs[i] = val
    return xs


def _code(desc):
    import bpperm
    with pytest.raises(bpperm.BppError) as e:
        bpperm.Circuit(desc)
    return e.value.code


def test_every_refusal_returns_its_code():
    d = gd.in_range(3)           # free sides: LCs 0..5 empty, asserts 6..12
    m = gd.member_of([3, 7, 9])  # two gates with defined sides; gate 1's left reads o_0
    assert _code(_variant(m, m_in=0)) == ARG
    assert _code(_variant(m, n_gates=0)) == ARG
    nvar = 2 + m.m_in + 3 * m.n_gates
    assert _code(_variant(m, lc_var=_set(m.lc_var, len(m.lc_var) - 1, nvar))) == ARG      # id out of range
    assert _code(_variant(d, side_aux=_set(d.side_aux, 0, 6))) == ARG                     # aux out of range
    t = m.lc_off[2]  # gate 1's left side: its one term o_0 -> l_1
    assert m.lc_var[t] == 2 + m.m_in + 2
    assert _code(_variant(m, lc_var=_set(m.lc_var, t, 2 + m.m_in + 3))) == ARG             # reads a wire of gate 1
    assert _code(_variant(m, side_aux=_set(m.side_aux, 0, 0), n_aux=1)) == ARG             # a free side with terms
    assert _code(_variant(m, lc_var=_set(_set(m.lc_var, 0, m.lc_var[1]), 1, m.lc_var[0]))) == ARG  # unsorted
    assert _code(_variant(m, lc_var=_set(m.lc_var, 1, m.lc_var[0]))) == ARG                # duplicate
    assert _code(_variant(m, lc_coef=_set(m.lc_coef, 0, bytes(32)))) == ARG                # zero coefficient
    assert _code(_variant(m, lc_off=_set(m.lc_off, 1, m.lc_off[2] + 1))) == ARG            # non-monotone
    assert _code(_variant(m, lc_coef=_set(m.lc_coef, 0, L.to_bytes(32, "little")))) == NONCANONICAL
    assert _code(_variant(m, lc_coef=_set(m.lc_coef, 0, b"\xff" * 32))) == NONCANONICAL
    # beyond the kernels' LDS: 683 gates (the witness kernel), Q = 1508 (the row tables)
    assert _code(cr.chain_circuit(683)) == LEN
    b = gd.CircuitBuilder()
    v = b.input()
    for _ in range(512):
        b.mul(v, v)
    for _ in range(482):
        b.assert_zero(v)
    import bpperm
    c = bpperm.Circuit(b.build())
    assert (c.Q, c.n_p) == (1507, 512)  # 512 gates with both sides defined fit, to the last row
    b.assert_zero(v)
    assert _code(b.build()) == LEN


def test_prover_checks_need_no_device():
    """Null handles and non-canonical scalars are refused before any device
    call, and nothing is written."""
    import bpperm
    from bpperm import _lib
    lib = _lib.load()
    desc, v, aux = cr.satisfying("range3", 0)
    c = bpperm.Circuit(desc)
    vb, ab = cr.sb(v[0]), b"".join(cr.sb(a) for a in aux)
    pf, V = ctypes.create_string_buffer(b"\xaa" * c.proof_len), ctypes.create_string_buffer(b"\xaa" * 64)

    def prove(cc, vb_, ab_, gb_):
        return lib.bpp_circuit_prove_batch(None, None, cc, 1, vb_, ab_, gb_, None, b"x", 1, pf, V)

    assert prove(None, vb, ab, None) == ARG
    assert prove(c.h, None, ab, None) == ARG
    assert prove(c.h, vb, None, None) == ARG
    bad = L.to_bytes(32, "little")
    assert prove(c.h, bad, ab, None) == NONCANONICAL
    assert prove(c.h, vb, ab[:-32] + bad, None) == NONCANONICAL
    assert prove(c.h, vb, ab, bad) == NONCANONICAL
    assert prove(c.h, vb, ab, None) == ARG  # canonical: now the null context
    assert pf.raw[:c.proof_len] == b"\xaa" * c.proof_len and V.raw[:64] == b"\xaa" * 64
    assert lib.bpp_circuit_verify(None, None, c.h, b"x", 1, pf, c.proof_len, V) == ARG
    assert lib.bpp_circuit_proof_len(None) == 0
    with pytest.raises(bpperm.BppError):
        c.eval([bad], [cr.sb(a) for a in aux], cr.sb(1))
    c.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_circuit_host_asan_ubsan(tmp_path):
    exe = tmp_path / "circuit_check"
    srcs = [ROOT / "tests" / "c" / "circuit_check.cpp",
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
