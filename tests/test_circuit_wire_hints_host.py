"""Hints over wires and x without a GPU: bpp_circuit_hint_eval_x and the host
witness over it against the plain-Python reference (tests/circuit_wire_hints_ref.py)
on the new gadgets and on hand-built programs, blackjack_total(2) over every
hand and total, the asserts that unsatisfied statements name, every refusal of
bpp_circuit_create_wire_hinted, and the statement left untouched."""
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_wire_hints_ref as wr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402

L = wr.L
sb = wr.sb
ARG, NONCANONICAL = 1, 4
XS = [0x1234567, 0, 1, L - 1, 2**252, 2**252 - 1, wr.rnd(b"whh-x")]


def ints(row):
    return [int.from_bytes(a, "little") for a in row]


def host_witness(c, v, x, pub=None):
    """hint_eval_x then eval, as ints: (aux, aL, aR, aO, bad)."""
    vb, ub = [sb(a) for a in v], [sb(u) for u in pub] if pub is not None else None
    aux = c.hint_eval_x(vb, sb(x), ub)
    aL, aR, aO, bad = c.eval(vb, aux, sb(x), pub=ub)
    return ints(aux), ints(aL), ints(aR), ints(aO), bad


def check_against_reference(c, desc, v, x, pub=None):
    aux, aL, aR, aO, bad = host_witness(c, v, x, pub)
    w_aux, wL, wR, wO, w_bad = wr.witness(desc, v, x, pub)
    pad = [0] * (c.n_p - desc.n_gates)
    assert aux == w_aux
    assert (aL, aR, aO) == (wL + pad, wR + pad, wO + pad)
    assert bad == w_bad
    return bad


# ------------------------------------------------------------- the gadgets

GADGETS = [("max_of(2, 2)", gd.max_of(2, 2)), ("max_of(3, 3)", gd.max_of(3, 3)), ("max_of(1, 4)", gd.max_of(1, 4)),
           ("not_among(1)", gd.not_among(1)), ("not_among(2)", gd.not_among(2)), ("not_among(5)", gd.not_among(5)),
           ("blackjack_total(1)", gd.blackjack_total(1)), ("blackjack_total(2)", gd.blackjack_total(2)),
           ("blackjack_total(3)", gd.blackjack_total(3))]


def bj_total(ranks):
    S = sum(min(r, 10) for r in ranks)
    return S + (10 if 1 in ranks and S <= 11 else 0)


def instances(name, desc):
    """(v, pub, the assert expected to fail or None)."""
    last = desc.n_asserts - 1
    if name.startswith("max_of"):
        k = desc.m_in - 1
        nbits = int(name.split(",")[1].strip(" )"))
        top = 2**nbits - 1
        hands = [[0] * k, [top] * k, [(3 * i + 1) % (top + 1) for i in range(k)], [top - i for i in range(k)],
                 list(range(k))]
        out = [(h + [max(h)], None, None) for h in hands]
        if k > 1:
            out += [(hands[2] + [max(hands[2]) + 1], None, last), (hands[3] + [min(hands[3])], None, last)]
        return out
    if name.startswith("not_among"):
        k = desc.m_in - 1
        out = [(list(range(5, 6 + k)), None, None), ([0] + [L - 1 - i for i in range(k)], None, None),
               ([2**252] + [wr.rnd(b"na-%d" % i) for i in range(k)], None, None)]
        out += [([7] + [8 + i for i in range(k - 1)] + [7], None, 0), ([7] * (k + 1), None, 0)]
        return out
    k = desc.m_in
    hands = [[1] * k, [13] * k, [10] * k, [(5 * i) % 13 + 1 for i in range(k)], [1] + [9] * (k - 1), [1] + [10] * (k - 1)]
    out = [(h, [bj_total(h)], None) for h in hands]
    out += [(hands[3], [bj_total(hands[3]) + 1], last), (hands[0], [bj_total(hands[0]) - 10], last)]
    return out


@pytest.mark.parametrize("name,desc", GADGETS, ids=[g[0] for g in GADGETS])
def test_gadgets_host_against_reference(name, desc):
    """hint_eval_x then eval equals the reference, satisfied instances have no
    failing assert, a wrong maximum, a repeated card and a wrong total name the
    expected one; aux_of agrees with both."""
    import bpperm
    c = bpperm.Circuit(desc)
    assert c.has_hints and desc.hints is not None and len(desc.hints.op) == desc.n_aux
    assert desc.hints.wire == any(wr.is_late(desc, t) for t in range(desc.n_aux))
    for v, pub, fails in instances(name, desc):
        bad = check_against_reference(c, desc, v, XS[0], pub)
        assert bad == (0 if fails is None else fails + 1), (name, v)
        assert [a % L for a in desc.aux_of(v)] == wr.hint_eval_x(desc, v, XS[0], pub), (name, v)


def test_gadget_shapes():
    """not_among(k): k - 1 product gates and ONE inverse, of the product wire;
    max_of and blackjack_total mix early and late hints."""
    for k in (2, 5):
        d = gd.not_among(k)
        assert (d.n_gates, d.n_aux, d.n_asserts) == (k, 1, 1)
        assert d.hints.op == [wr.INV] and d.hints.lc_var == [2 + (k + 1) + 3 * (k - 2) + 2] and wr.is_late(d, 0)
    assert not gd.not_among(1).hints.wire  # (one difference: the inverse of v_0 - v_1, an early hint)
    d = gd.max_of(3, 3)
    assert d.n_gates == 3 * 3 + 2 * 5
    late = [wr.is_late(d, t) for t in range(d.n_aux)]
    assert any(late) and not all(late)
    d = gd.blackjack_total(2)
    late = [wr.is_late(d, t) for t in range(d.n_aux)]
    assert sum(late) == 2 * 5 and d.n_pub == 1 and d.n_gates == 2 * 16 + 1 + 5 + 1
    assert gd.blackjack_total(5).n_gates == 5 * 16 + 4 + 7 + 1


def test_blackjack_total_2_every_hand_every_total():
    """All 169 hands of two ranks against every total 0..31: the host witness is
    satisfied exactly for the true total."""
    import bpperm
    desc = gd.blackjack_total(2)
    c = bpperm.Circuit(desc)
    x = sb(XS[0])
    for a in range(1, 14):
        for b in range(1, 14):
            vb = [sb(a), sb(b)]
            want = bj_total([a, b])
            aux = c.hint_eval_x(vb, x, [sb(want)])  # (no hint reads u_0: the same for every total)
            assert ints(aux) == wr.hint_eval_x(desc, [a, b], XS[0], [want])
            ok = [t for t in range(32) if c.eval(vb, aux, x, pub=[sb(t)])[3] == 0]
            assert ok == [want], (a, b)


def test_blackjack_total_enforces_the_rank_range():
    import bpperm
    desc = gd.blackjack_total(2)
    c = bpperm.Circuit(desc)
    for hand in ([0, 5], [14, 5], [5, 16], [5, L - 1]):
        for t in range(32):
            assert host_witness(c, hand, XS[0], [t])[4] != 0, (hand, t)


# ------------------------------------------------------ hand-built programs

PROGRAMS = [("x_program", wr.x_program()), ("bits_program", wr.bits_program()),
            ("kernel_program(1)", wr.kernel_program(1, False)), ("kernel_program(40, chain)", wr.kernel_program(40, True)),
            ("kernel_program(65, flat)", wr.kernel_program(65, False))]


@pytest.mark.parametrize("name,desc", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_hand_built_host_against_reference(name, desc):
    """Every op over a wire and over x, the designed values under every bit arg,
    an aux index feeding two sides, early and late hints mixed, a chain where
    gate g's hint reads o_{g-1}: host against reference, for several x (x = 0,
    1, l - 1, 2^252, 2^252 - 1 among them, and x = v_5: a zero made of x)."""
    import bpperm
    c = bpperm.Circuit(desc)
    vs, us = wr.rows(3)
    for p in range(3):
        for x in XS + [vs[p][5]]:
            check_against_reference(c, desc, vs[p], x, us[p])


def test_hand_built_programs_cover_what_they_claim():
    d = wr.bits_program()
    h = d.hints
    seen = {(h.op[t] & 0xFF, h.op[t] >> 8, h.lc_var[h.lc_off[t]]) for t in range(d.n_aux)
            if h.lc_off[t + 1] - h.lc_off[t] == 1}
    for j in range(5):  # the designed values 0, 1, l - 1, 2^252, 2^252 - 1 are l_0..l_4
        assert {(op, arg, d.w(j, 0)) for op in (wr.BIT, wr.NOT_BIT) for arg in wr.BIT_ARGS} <= seen
        assert {(op, 0, d.w(j, 0)) for op in (wr.INV, wr.IS_ZERO)} <= seen
    assert wr.V_ROW[:5] == [0, 1, L - 1, 2**252, 2**252 - 1]
    d = wr.kernel_program(65, True)
    late = [wr.is_late(d, t) for t in range(d.n_aux)]
    assert any(late) and not all(late)                                   # early and late mixed
    assert any(d.side_aux.count(a) == 2 for a in range(d.n_aux))          # an aux index feeding two sides
    ops = {d.hints.op[t] & 0xFF for t in range(d.n_aux) if late[t]}
    assert ops == {0, 1, 2, 3, 4}
    o_prev = [t for t in range(d.n_aux) if d.hints.lc_var[d.hints.lc_off[t]:d.hints.lc_off[t + 1]] ==
              [d.w(d.side_aux.index(t) // 2 - 1, 2)]]
    assert o_prev                                                         # gate g's hint reads o_{g-1}
    x_ops = {wr.x_program().hints.op[t] & 0xFF for t in range(wr.x_program().n_aux)}
    assert x_ops == {0, 1, 2, 3, 4}


def test_late_hint_that_feeds_no_side_is_never_evaluated():
    """An aux value no side uses, with a late hint: accepted, and 0."""
    import bpperm
    d = wr.Desc(2, 0)
    unused = d.hint(wr.INV, 0, [(d.x, 1)])
    t = d.hint(wr.VALUE, 0, [(d.x, 1)])
    d.gate([(d.v(0), 1)], t)
    c = bpperm.Circuit(d)
    aux = host_witness(c, [3, 4], 9)[0]
    assert aux[unused] == 0 and aux[t] == 9 and aux == wr.hint_eval_x(d, [3, 4], 9)


def test_program_without_a_late_hint_behaves_as_hinted():
    """Through the new entry point a program of early hints gives hint_eval's
    values, from hint_eval and from hint_eval_x alike."""
    import bpperm
    for desc, v in ((gd.in_range(5), [19]), (gd.distinct(4), [1, 2, 3, L - 1]), (gd.ascending(3, 4), [3, 9, 10])):
        a, b = bpperm.Circuit(desc, wire_hints=True), bpperm.Circuit(desc)
        vb = [sb(x) for x in v]
        want = b.hint_eval(vb)
        assert a.hint_eval(vb) == want and a.hint_eval_x(vb, sb(5)) == want and b.hint_eval_x(vb, sb(5)) == want
        assert ints(want) == [x % L for x in desc.aux_of(v)]


def test_hint_eval_without_x_refuses_late_hints():
    """bpp_circuit_hint_eval has no x: BPP_ERR_ARG on a circuit with a late hint;
    bpp_circuit_hint_eval_x checks its arguments."""
    import bpperm
    c = bpperm.Circuit(gd.not_among(2))
    vb = [sb(5), sb(6), sb(7)]
    with pytest.raises(bpperm.BppError) as e:
        c.hint_eval(vb)
    assert e.value.code == ARG
    lib = c.lib
    out = bytearray(32)
    buf = (bpperm._lib.C.c_char * 32).from_buffer(out)
    assert lib.bpp_circuit_hint_eval_x(None, b"".join(vb), None, sb(1), buf) == ARG
    assert lib.bpp_circuit_hint_eval_x(c.h, b"".join(vb), None, None, buf) == ARG
    assert lib.bpp_circuit_hint_eval_x(c.h, b"".join(vb), None, L.to_bytes(32, "little"), buf) == NONCANONICAL
    assert lib.bpp_circuit_hint_eval_x(c.h, L.to_bytes(32, "little") + vb[1] + vb[2], None, sb(1), buf) == NONCANONICAL
    plain = bpperm.Circuit(gd.not_among(2), hints=False)
    assert lib.bpp_circuit_hint_eval_x(plain.h, b"".join(vb), None, sb(1), buf) == ARG


# ----------------------------------------------------------------- the builder

def test_builder_derived():
    """derived() allows x and wires where hint() raises; mul() refuses a derived
    side that reads a wire of its own or a later gate; a description whose
    derived hints read neither is created through the old entry point."""
    import bpperm
    b = gd.CircuitBuilder()
    v = b.inputs(2)
    l0, r0, o0 = b.mul(v[0], b.derived(gd.HINT_INV, b.challenge - v[1]))
    with pytest.raises(ValueError):
        b.hint(gd.HINT_VALUE, o0)
    with pytest.raises(ValueError):
        b.hint(gd.HINT_VALUE, b.challenge)
    with pytest.raises(ValueError):
        b.derived(gd.HINT_INV, o0, 3)
    with pytest.raises(ValueError):
        b.derived(gd.HINT_BIT, o0, 253)
    own = b.derived(gd.HINT_VALUE, b._wires(1)[0])  # a wire of gate 1, the next gate
    with pytest.raises(ValueError):
        b.mul(v[1], own)
    later = b.derived(gd.HINT_VALUE, b._wires(2)[2])
    with pytest.raises(ValueError):
        b.mul(later, v[1])
    b.mul(o0, 1)  # gate 1
    b.mul(own, b.derived(gd.HINT_IS_ZERO, o0 - r0))  # gate 2: `own` reads l_1
    assert len(b.hints) == 4  # (`later` feeds no side: accepted, never evaluated)
    d = b.build()
    assert d.hints is not None and d.hints.wire
    c = bpperm.Circuit(d)
    assert check_against_reference(c, d, [3, 4], 77) == 0
    b2 = gd.CircuitBuilder()
    w = b2.input()
    b2.mul(w, b2.derived(gd.HINT_INV, w))
    assert b2.build().hints.wire is False


# --------------------------------------------------------------------- refusals

def _feeds(var, gate_right=1, second_side=None):
    """Three gates v_0 * aux_g; hint 1 (VALUE over `var`) feeds the right side of
    gate `gate_right` and, with second_side = (gate, side), that side too."""
    d = wr.Desc(2, 1)
    t = [d.hint(wr.VALUE, 0, [(d.v(0), 1)]) for _ in range(3)]
    d.hints.lc_var[1] = var
    for g in range(3):
        left = [(d.v(0), 1)]
        right = t[1] if g == gate_right else t[0] if g < gate_right else t[2]
        if second_side == (g, 0):
            left = t[1]
        if second_side == (g, 1):
            right = t[1]
        d.gate(left, right)
    return d


# m_in = 2, n_pub = 1: x is id 3, u_0 is 4, the wires of gate h are 5 + 3h + {0, 1, 2}, the last wire is 13
W = lambda h, s: 5 + 3 * h + s
LATE_REFUSED = [
    ("a wire of its own gate", _feeds(W(1, 0))),
    ("its own gate's output", _feeds(W(1, 2))),
    ("a wire of a later gate", _feeds(W(2, 1))),
    ("the other side of its own gate", _feeds(W(0, 0), gate_right=0)),
    ("own gate, through a second side", _feeds(W(1, 2), gate_right=2, second_side=(1, 0))),
    ("later gate, through a second side", _feeds(W(1, 0), gate_right=2, second_side=(0, 1))),
    ("an id past the last wire", _feeds(W(2, 2) + 1)),
    ("an id far past the last wire", _feeds(1 << 20)),
]


@pytest.mark.parametrize("what,desc", LATE_REFUSED, ids=[r[0] for r in LATE_REFUSED])
def test_create_wire_hinted_refuses(what, desc):
    import bpperm
    with pytest.raises(bpperm.BppError) as e:
        bpperm.Circuit(desc)
    assert e.value.code == ARG, what
    assert not bpperm.Circuit(desc, hints=False).has_hints  # the description itself is fine


def test_create_wire_hinted_accepts_what_only_the_old_entry_point_refuses():
    import bpperm
    for var in (3, W(0, 0), W(0, 2), W(1, 2)):  # x, wires of earlier gates
        d = _feeds(var, gate_right=2)
        c = bpperm.Circuit(d)
        assert c.has_hints
        check_against_reference(c, d, [6, 7], 11, [13])
        with pytest.raises(bpperm.BppError) as e:
            bpperm.Circuit(d, wire_hints=False)
        assert e.value.code == ARG
    # the last wire, read by a hint that feeds no side
    d = _feeds(W(2, 2), gate_right=2)
    d.side_aux[5] = 0
    assert bpperm.Circuit(d).has_hints


def _one_hint(op_word, var, coef, lc_off=None):
    d = _feeds(1, gate_right=1)
    h = d.hints
    h.op[1] = op_word
    h.lc_var[1:2] = list(var)
    h.lc_coef[1:2] = [c if isinstance(c, bytes) else sb(c) for c in coef]
    h.lc_off = lc_off or [0, 1, 1 + len(var), 2 + len(var)]
    return d


OLD_REFUSED = [
    ("unknown op", _one_hint(5, [1], [1]), ARG),
    ("unknown op byte", _one_hint(0xFF, [1], [1]), ARG),
    ("arg above 252", _one_hint(wr.BIT | 253 << 8, [1], [1]), ARG),
    ("arg above 252, NOT_BIT", _one_hint(wr.NOT_BIT | 0xFFFFFF << 8, [1], [1]), ARG),
    ("arg on VALUE", _one_hint(wr.VALUE | 1 << 8, [1], [1]), ARG),
    ("arg on INV", _one_hint(wr.INV | 7 << 8, [1], [1]), ARG),
    ("arg on IS_ZERO", _one_hint(wr.IS_ZERO | 252 << 8, [1], [1]), ARG),
    ("unsorted ids", _one_hint(wr.VALUE, [2, 1], [1, 1]), ARG),
    ("unsorted ids, wires", _one_hint(wr.VALUE, [W(0, 1), W(0, 0)], [1, 1]), ARG),
    ("duplicate ids", _one_hint(wr.VALUE, [3, 3], [1, 1]), ARG),
    ("zero coefficient", _one_hint(wr.VALUE, [W(0, 0)], [0]), ARG),
    ("non-monotone lc_off", _one_hint(wr.VALUE, [1], [1], lc_off=[0, 2, 1, 3]), ARG),
    ("lc_off[0] not 0", _one_hint(wr.VALUE, [1], [1], lc_off=[1, 1, 2, 3]), ARG),
    ("coefficient = l", _one_hint(wr.VALUE, [3], [L.to_bytes(32, "little")]), NONCANONICAL),
    ("coefficient = 2^256 - 1", _one_hint(wr.VALUE, [W(0, 2)], [b"\xff" * 32]), NONCANONICAL),
]


@pytest.mark.parametrize("what,desc,code", OLD_REFUSED, ids=[r[0] for r in OLD_REFUSED])
def test_create_wire_hinted_keeps_the_old_refusals(what, desc, code):
    import bpperm
    with pytest.raises(bpperm.BppError) as e:
        bpperm.Circuit(desc)
    assert e.value.code == code, what
    assert not bpperm.Circuit(desc, hints=False).has_hints


def test_flags_and_null_arguments():
    """The flags of bpp_circuit_create_ex: unknown bits refused, LARGE and TILED
    accepted; hints == NULL is bpp_circuit_create_ex; null desc or out refused."""
    import ctypes

    import bpperm
    d = gd.not_among(3)
    with pytest.raises(bpperm.BppError) as e:
        bpperm.Circuit(d, flags=4)
    assert e.value.code == ARG
    for kw in ({"large": True}, {"tiled": True}):
        assert bpperm.Circuit(d, **kw).has_hints
    c = bpperm.Circuit(d)
    lib, h = c.lib, ctypes.c_void_p()
    assert lib.bpp_circuit_create_wire_hinted(None, 0, 0, None, ctypes.byref(h)) == ARG
    u32a = lambda xs: (ctypes.c_uint32 * max(len(xs), 1))(*xs)
    keep = (u32a(d.side_aux), u32a(d.lc_off), u32a(d.lc_var), b"".join(d.lc_coef))
    dc = bpperm._CircuitDescC(d.m_in, d.n_gates, d.n_aux, d.n_asserts, *keep)
    assert lib.bpp_circuit_create_wire_hinted(ctypes.byref(dc), 0, 0, None, None) == ARG
    assert lib.bpp_circuit_create_wire_hinted(ctypes.byref(dc), 0, 0, None, ctypes.byref(h)) == 0
    assert lib.bpp_circuit_has_hints(h) == 0
    lib.bpp_circuit_destroy(h)


# ------------------------------------------------------- the statement untouched

@pytest.mark.parametrize("name,desc", GADGETS + PROGRAMS[:2], ids=[g[0] for g in GADGETS + PROGRAMS[:2]])
def test_wire_hints_are_no_part_of_the_statement(name, desc):
    """Digest, matrices, info and proof length are equal across plain and
    wire-hinted creation -- and hinted creation, where the old entry point takes
    the program (no late hint)."""
    import bpperm
    a, b = bpperm.Circuit(desc), bpperm.Circuit(desc, hints=False)
    assert a.has_hints and not b.has_hints
    both = [a, b]
    if not any(wr.is_late(desc, t) for t in range(desc.n_aux)):
        both.append(bpperm.Circuit(desc, wire_hints=False))
        both.append(bpperm.Circuit(desc, wire_hints=True))
    for c in both[1:]:
        assert (a.n_p, a.Q, a.m, a.digest, a.proof_len) == (c.n_p, c.Q, c.m, c.digest, c.proof_len)
        for which in range(6):
            assert a.matrix(which) == c.matrix(which)


def test_prove_without_aux_passes_the_argument_checks():
    """aux == NULL on a wire-hinted circuit passes the argument checks and stops
    at the null context (no GPU here); a non-canonical v is still named first."""
    import ctypes

    import bpperm
    c = bpperm.Circuit(gd.not_among(2))
    vb = sb(5) + sb(6) + sb(7)
    pf, V = ctypes.create_string_buffer(c.proof_len), ctypes.create_string_buffer(32 * c.m)
    assert c.lib.bpp_circuit_prove_batch(None, None, c.h, 1, vb, None, None, None, b"x", 1, pf, V) == ARG
    nc = L.to_bytes(32, "little") + sb(6) + sb(7)
    assert c.lib.bpp_circuit_prove_batch(None, None, c.h, 1, nc, None, None, None, b"x", 1, pf, V) == NONCANONICAL


def test_wire_hints_host_asan_ubsan(tmp_path):
    """tests/c/circuit_wire_hints_check.cpp, a stand-alone program over the host
    sources, under ASan + UBSan."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    root = HERE.parent
    csrc = root / "bulletproof-perm_amd" / "csrc"
    exe = tmp_path / "circuit_wire_hints_check"
    srcs = [root / "tests" / "c" / "circuit_wire_hints_check.cpp",
            *(csrc / "host" / f for f in ("circuit.cpp", "perm_circuit.cpp", "keccak.cpp", "keccak_x8.cpp"))]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-march=x86-64-v3",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(csrc), *map(str, srcs),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, BPP_HOST_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
