"""Device GF(2^255 - 19) arithmetic (fe25519.cuh, fe10_ops.inc) at the limb
bounds its contracts state, through the arithmetic probe: one probe call per
opcode, raw limbs in, raw limbs out, compared with Python integers.

Checked for every case: the output's value is the big-integer result mod p,
and every output limb lies inside the bound the function states."""
import functools

import pytest

import fe10_model as m
from oracle import ristretto as r255
from oracle.merlin import Rng

pytestmark = pytest.mark.gpu
P = m.P
ALL = ("exact", "tight", "add_nc", "sub_nc", "g", "mul_in")


@functools.lru_cache(maxsize=None)
def classes(names=ALL, nrand=512, seed=11):
    return m.field_classes(Rng(seed, b"fe10-cases"), nrand=nrand, names=names)


def pairs(names_a=ALL, names_b=ALL, nrand=512):
    """(labels, a, b): every max x max pair, every one-hot of a against the
    largest b, and the random vectors paired with a shifted copy of b's."""
    ca, cb = classes(names_a, nrand, 11), classes(names_b, nrand, 12)
    maxa = [c for c in ca if c[0].endswith("/max")]
    maxb = [c for c in cb if c[0].endswith("/max")]
    out = [(x, y) for x in maxa for y in maxb]
    out += [(x, maxb[-1]) for x in ca if "onehot" in x[0]] + [(maxa[-1], y) for y in cb if "onehot" in y[0]]
    ra = [c for c in ca if "rand" in c[0]]
    rb = [c for c in cb if "rand" in c[0]]
    out += [(x, rb[(7 * i + 3) % len(rb)]) for i, x in enumerate(ra)]
    return [f"{x[0]} , {y[0]}" for x, y in out], [x[1] for x, _ in out], [y[1] for _, y in out]


def check(labels, outs, want, bound, ins=None):
    for i, (lab, o) in enumerate(zip(labels, outs)):
        limbs = o[:10]
        ctx = f"{lab}: in {ins[i] if ins else ''} out {limbs}"
        assert m.value(limbs) == want[i] % P, ctx
        assert m.within(limbs, bound), ctx


def test_fe_carry_at_its_input_bound():
    """fe_carry: limbs < 2^32 - 2^7 in (limb + carry never wraps 32 bits),
    limb 0 < 2^26 + 19 * 2^7 and exact widths elsewhere out."""
    cs = list(classes())
    cs.append(("carry_in/max", m.all_at(m.CARRY_IN)))
    cs += [(f"carry_in/onehot{k}", x) for k, x in enumerate(m.one_hot(m.CARRY_IN))]
    cs += [(f"carry_in/rand{k}", x) for k, x in enumerate(m.random_under(m.CARRY_IN, Rng(13, b"fe10-cases"), 512))]
    labels, a = [c[0] for c in cs], [c[1] for c in cs]
    out = m.probe().fe("carry", a)
    check(labels, out, [m.raw_value(x) for x in a], m.CARRY_OUT, a)
    # the largest input: every carry at its maximum (63 from even limbs, 127 from odd)
    top = out[labels.index("carry_in/max")]
    assert top[0] == (1 << 26) - 129 + 19 * 127 and top[9] == ((1 << 32) - 129 + 63) & 0x1FFFFFF


def test_fe_add_sub_neg():
    """fe_add on every pair of classes (limb sums far below fe_carry's input
    bound); fe_sub with the minuend up to the multiplier's input bound and
    the subtrahend tight at its maximum, as the point formulas use it
    (F = fe_sub(D, C), D = Z + Z uncarried); fe_neg of tight limbs."""
    labels, a, b = pairs()
    check(labels, m.probe().fe("add", a, b), [m.raw_value(x) + m.raw_value(y) for x, y in zip(a, b)], m.CARRY_OUT)
    labels, a, b = pairs(ALL, ("exact", "tight"))
    check(labels, m.probe().fe("sub", a, b), [m.raw_value(x) - m.raw_value(y) for x, y in zip(a, b)], m.CARRY_OUT)
    cs = classes(("exact", "tight"))
    a = [c[1] for c in cs]
    check([c[0] for c in cs], m.probe().fe("neg", a), [-m.raw_value(x) for x in a], m.CARRY_OUT)


def test_fe_add_nc_sub_nc():
    """The uncarried forms are limb-wise: a + b and a + 2p - b.  Tight
    operands stay under the stated 2^27 + 2^19 and 2^27 + 2^26 + 2^18; the
    sum of those two (the G of the point formulas) stays under 2^27.6."""
    labels, a, b = pairs(("exact", "tight"), ("exact", "tight"))
    out = m.probe().fe("add_nc", a, b)
    for lab, x, y, o in zip(labels, a, b, out):
        assert o[:10] == [u + v for u, v in zip(x, y)], lab
        assert m.within(o[:10], m.ADD_NC), lab
    assert max(max(o[:10]) for o in out) == m.ADD_NC[0] - 2  # (2^26 + 2^18 - 1) twice
    # minuend up to the fe_add_nc bound, subtrahend tight
    labels, a, b = pairs(("exact", "tight", "add_nc"), ("exact", "tight"))
    out = m.probe().fe("sub_nc", a, b)
    for lab, x, y, o in zip(labels, a, b, out):
        assert o[:10] == [u + t - v for u, t, v in zip(x, m.TWO_P, y)], lab
        assert m.value(o[:10]) == (m.raw_value(x) - m.raw_value(y)) % P, lab
        if lab.split("/")[0] in ("exact", "tight"):
            assert m.within(o[:10], m.SUB_NC), lab
    # G = fe_add_nc(fe_add_nc(Z, Z), C) with all three tight at their maximum
    t = m.all_at(m.TIGHT)
    (d,) = m.probe().fe("add_nc", [t], [t])
    (g,) = m.probe().fe("add_nc", [d[:10]], [t])
    assert m.within(g[:10], m.G_BOUND) and m.within(g[:10], m.MUL_IN) and max(g[:10]) == m.G_BOUND[0] - 3


def test_fe_mul_sq_at_input_bound():
    """fe_mul / fe_sq with both operands up to floor(2^27.6) - 1 in every limb
    (the 32-bit 19 b_j and the 64-bit column sums are the binding limits):
    even limbs < 2^26, odd < 2^25, limb 1 < 2^25 + 2^18 out."""
    labels, a, b = pairs()
    assert any(x == m.all_at(m.MUL_IN) and y == m.all_at(m.MUL_IN) for x, y in zip(a, b))
    assert any(x == m.all_at(m.G_BOUND) for x in a) and any(y == m.all_at(m.G_BOUND) for y in b)
    check(labels, m.probe().fe("mul", a, b), [m.raw_value(x) * m.raw_value(y) for x, y in zip(a, b)], m.MUL_OUT)
    check(labels, m.probe().fe("mul", b, a), [m.raw_value(x) * m.raw_value(y) for x, y in zip(a, b)], m.MUL_OUT)
    cs = classes()
    a = [c[1] for c in cs]
    check([c[0] for c in cs], m.probe().fe("sq", a), [m.raw_value(x) ** 2 for x in a], m.MUL_OUT)


def test_fe_mul_small():
    ks = [0, 1, 2, 19, 121666, 2**26 - 1, 2**31 - 1]
    cs = [c for c in classes(nrand=32)] + [("u32/max", [2**32 - 1] * 10)]
    labels, a, b = [], [], []
    for k in ks:
        for lab, x in cs:
            labels.append(f"{lab} * {k}")
            a.append(x)
            b.append([k] + [0] * 9)
    check(labels, m.probe().fe("mul_small", a, b), [m.raw_value(x) * y[0] for x, y in zip(a, b)], m.TIGHT)


def modulus_cases():
    """(label, limbs): the values around p and 2^255 in exact limbs with the
    excess in limb 9, the ripple ladder, and tight limbs at their maximum."""
    cs = [(f"value {v:#x}", m.exact_limbs(v)) for v in m.AROUND_MODULUS]
    cs += [(f"ripple {x[0]:#x}", x) for x in m.ripple_cases()]
    cs += list(classes(("exact", "tight")))
    for v in m.AROUND_MODULUS:  # the same values with every limb as loose as tight allows
        cs += [(f"loose {v:#x} #{k}", x) for k, x in enumerate(m.loose_any(v, m.TIGHT))]
    return cs


def test_fe_canon_and_predicates():
    """fe_canon / fe_store_words give exactly the canonical representative;
    fe_iszero, fe_isneg, fe_eq, fe_abs follow from it."""
    cs = modulus_cases()
    labels, a = [c[0] for c in cs], [c[1] for c in cs]
    want = [m.value(x) for x in a]
    for lab, x, o, w in zip(labels, a, m.probe().fe("canon", a), want):
        assert o[:10] == m.exact_limbs(w), f"{lab}: {x} -> {o[:10]}"
    for lab, o, w in zip(labels, m.probe().fe("store_words", a), want):
        assert o[:8] == m.words8(w), lab
    # fe_eq against a tight representation of the same value, and of value + 1
    same = [m.loose_any(w, m.TIGHT)[-1] for w in want]
    other = [m.loose_any(w + 1, m.TIGHT)[0] for w in want]
    for lab, o, o2, w in zip(labels, m.probe().fe("pred", a, same), m.probe().fe("pred", a, other), want):
        assert o[:3] == [int(w == 0), w & 1, 1], lab
        assert o2[:3] == [int(w == 0), w & 1, 0], lab
    # fe_abs negates, so its operand must be a valid subtrahend (limbs <= 2p's
    # limbs: every tight limb is).  Of the excess-in-limb-9 forms the four
    # values >= 2p - 1 are not (limb 9 = 2^26 - 1 > 0x3fffffe: the limb-wise
    # 2p - a would wrap); they are not tight either, and no device code makes
    # that form (fe_load_words folds bit 255 into limb 0).
    keep = [i for i, x in enumerate(a) if all(v <= t for v, t in zip(x, m.TWO_P))]
    assert [labels[i] for i in range(len(a)) if i not in set(keep)] == \
        [f"value {v:#x}" for v in (2 * P - 1, 2 * P, 2 * P + 1, 2**256 - 1)]
    out = m.probe().fe("abs", [a[i] for i in keep])
    for i, o in zip(keep, out):
        assert m.value(o[:10]) == r255.ct_abs(want[i]), labels[i]
        assert o[:10] == a[i] or m.within(o[:10], m.CARRY_OUT), labels[i]


def test_fe_words():
    rng = Rng(14, b"fe10-cases")
    vals = list(m.AROUND_MODULUS) + [v | (1 << 255) for v in m.AROUND_MODULUS if v < 1 << 255]
    vals += [P - (1 << (32 * i)) for i in range(1, 8)] + [P - 2, P + 2, 2**255 - 20, (1 << 255) - (1 << 32)]
    vals += [int.from_bytes(rng.bytes(32), "little") for _ in range(256)]
    a = [m.words8(v) + [0, 0] for v in vals]
    for v, o in zip(vals, m.probe().fe("load_words", a)):
        lo, top = v & ((1 << 255) - 1), v >> 255
        expect = m.exact_limbs(lo)
        expect[0] += 19 * top
        assert o[:10] == expect and m.value(o[:10]) == (lo + 19 * top) % P, hex(v)
    for v, o in zip(vals, m.probe().fe("words_canonical", a)):
        assert o[0] == int(v < P), hex(v)


def test_fe_invert_pow22523():
    cs = [(f"value {v:#x} #{k}", x) for v in m.AROUND_MODULUS + [2, P - 2, r255.SQRT_M1]
          for k, x in enumerate(m.loose_any(v, m.TIGHT))]
    cs += list(classes(ALL, nrand=64))  # the operand only feeds fe_sq / fe_mul: any multiplier operand
    labels, a = [c[0] for c in cs], [c[1] for c in cs]
    check(labels, m.probe().fe("invert", a), [pow(m.value(x), P - 2, P) for x in a], m.MUL_OUT)
    check(labels, m.probe().fe("pow22523", a), [pow(m.value(x), (P - 5) // 8, P) for x in a], m.MUL_OUT)


def test_fe_sqrt_ratio_m1():
    rng = Rng(15, b"fe10-cases")
    rnd = lambda: int.from_bytes(rng.bytes(32), "little") % P
    uv = [(0, 0), (0, 1), (1, 0), (0, rnd()), (rnd(), 0), (1, 1), (P - 1, 1), (1, P - 1), (r255.SQRT_M1, 1), (2, 1), (1, 2)]
    for _ in range(32):
        x, v = rnd(), rnd()
        uv.append((x * x % P * v % P, v))                    # square ratio
        uv.append((x * x % P * v % P * r255.SQRT_M1 % P, v))  # i * square
        uv.append((rnd(), rnd()))
    labels, a, b, want = [], [], [], []
    # u is negated (a subtrahend: tight); v only feeds multipliers (up to 2^27.6)
    for u, v in uv:
        ureps = m.loose_any(u, m.TIGHT)[::-1]
        vreps = m.loose_any(v, m.TIGHT) + m.loose_any(v, m.MUL_IN)[:1]
        for k, y in enumerate(vreps):
            x = ureps[k % len(ureps)]
            labels.append(f"u {u:#x} v {v:#x} #{k}")
            a.append(x)
            b.append(y)
            want.append(r255.sqrt_ratio_m1(u, v))
    flags = set()
    for lab, o, (sq, r) in zip(labels, m.probe().fe("sqrt_ratio_m1", a, b), want):
        assert o[0] == int(sq) and m.value(o[1:11]) == r, lab
        assert m.within(o[1:11], m.TIGHT), lab
        flags.add(sq)
    assert flags == {True, False}
