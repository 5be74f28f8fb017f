"""Device Edwards25519 / ristretto255 point arithmetic (ge25519.cuh,
msm_kernels.cuh ge_madd_fg, dt_walk.cuh ge_add_quad) through the arithmetic
probe, against oracle.ristretto: the completeness cases of the unified law,
inputs in tight limbs at maximum looseness, outputs inspected limb by limb."""
import functools

import pytest

import fe10_model as m
from oracle import ristretto as r255
from oracle.merlin import Rng

pytestmark = pytest.mark.gpu
P = m.P


def rnd_fe(rng):
    return int.from_bytes(rng.bytes(32), "little") % P


@functools.lru_cache(maxsize=None)
def point_sets():
    """(special, random): identity, basepoint, the eight small-order points
    and the negatives; 16 random points.  Every point gets a random Z != 1."""
    rng = Rng(31, b"ge-cases")
    so = m.small_order_points()
    special = [r255.IDENTITY, r255.BASEPOINT] + so
    special += [r255.ed_neg(p) for p in special[1:]]
    random = [m.affine_point(r255.from_uniform_bytes(rng.bytes(64))) for _ in range(16)]
    sc = lambda p: m.scale(p, rnd_fe(rng) or 2)
    return [sc(p) for p in special], [sc(p) for p in random]


@functools.lru_cache(maxsize=None)
def pair_cases():
    special, random = point_sets()
    every = special + random
    prs = [(p, q) for p in special for q in special]
    prs += [(random[i], random[(3 * i + j + 1) % 16]) for i in range(16) for j in range(4)]
    prs += [(random[i], special[(5 * i + j) % len(special)]) for i in range(16) for j in range(3)]
    prs += [(special[(7 * i + j) % len(special)], random[i]) for i in range(16) for j in range(3)]
    for p in every:
        prs += [(p, p), (p, m.scale(p, 3)), (p, r255.ed_neg(p)), (p, r255.IDENTITY), (r255.IDENTITY, p)]
    return prs


def words(p, k=0):
    """P3 row: tight limbs at maximum looseness, the coordinates as v or v + p."""
    ms = [(k >> j) & 1 for j in range(4)]
    return m.p3_limbs(p, m.TIGHT, ms)


def check_point(row, want, label, bound=m.MUL_OUT):
    X, Y, Z, T = m.p3_point(row)
    Xw, Yw, Zw, _ = want
    assert Z != 0, label
    assert (X * Zw - Xw * Z) % P == 0 and (Y * Zw - Yw * Z) % P == 0, label
    assert (X * Y - Z * T) % P == 0, label
    for k in range(4):
        assert m.within(row[10 * k: 10 * k + 10], bound), (label, k, row[10 * k: 10 * k + 10])


def test_mixed_additions_and_their_variants():
    """ge_madd / ge_msub against ed_add; ge_madd_signed, ge_madd_fg (operand
    fetched and swapped by fetch_entry_sw) and ge_madd_signed_h1 + ge_madd_h2
    agree with them limb for limb."""
    prs = pair_cases()
    p = [words(a, i) for i, (a, _) in enumerate(prs)]
    nl = [m.niels_limbs(m.niels_of(b)) for _, b in prs]
    n = len(prs)
    pr = m.probe()
    add, _ = pr.ge("madd", p, nl=nl)
    sub, _ = pr.ge("msub", p, nl=nl)
    for i, (a, b) in enumerate(prs):
        check_point(add[i], r255.ed_add(a, b), f"madd pair {i}")
        check_point(sub[i], r255.ed_add(a, r255.ed_neg(b)), f"msub pair {i}")
    for op in ("madd_signed", "madd_fg", "madd_h1h2"):
        assert pr.ge(op, p, nl=nl, flag=[0] * n)[0] == add, op
        assert pr.ge(op, p, nl=nl, flag=[1] * n)[0] == sub, op
        mixed = pr.ge(op, p, nl=nl, flag=[i & 1 for i in range(n)])[0]
        assert mixed == [sub[i] if i & 1 else add[i] for i in range(n)], op


def test_full_addition_quad_doubling_negation():
    prs = pair_cases()
    p = [words(a, i) for i, (a, _) in enumerate(prs)]
    q = [words(b, i >> 2) for i, (_, b) in enumerate(prs)]
    pr = m.probe()
    add, _ = pr.ge("add", p, q)
    for i, (a, b) in enumerate(prs):
        check_point(add[i], r255.ed_add(a, b), f"add pair {i}")
    # one addition over the four lanes of a quad: the same limbs
    assert pr.ge("add_quad", p, q)[0] == add
    assert pr.ge("add_quad", p[:5], q[:5])[0] == add[:5]  # a last wave padded with copies of case 0
    special, random = point_sets()
    every = special + random
    rows = [words(a, k) for a in every for k in (0, 5, 15)]
    pts = [a for a in every for _ in range(3)]
    dbl, _ = pr.ge("dbl", rows)
    neg, _ = pr.ge("neg", rows)
    for i, a in enumerate(pts):
        check_point(dbl[i], r255.ed_double(a), f"dbl {i}")
        check_point(neg[i], r255.ed_neg(a), f"neg {i}", m.TIGHT)


def test_niels_conversions():
    special, random = point_sets()
    every = special + random
    pr = m.probe()
    rows = [words(a, i) for i, a in enumerate(every)]
    _, nl = pr.ge("to_niels", rows)
    aff = [words(m.affine_point(a), i) for i, a in enumerate(every)]
    _, nl2 = pr.ge("niels_from_affine", aff)
    for i, a in enumerate(every):
        want = m.niels_of(a)
        for got in (nl[i], nl2[i]):
            assert tuple(m.value(got[10 * k: 10 * k + 10]) for k in range(3)) == want, i
            assert all(m.within(got[10 * k: 10 * k + 10], m.TIGHT) for k in range(3)) and got[30:] == [0, 0], i
    back, _ = pr.ge("from_niels", rows, nl=[m.niels_limbs(m.niels_of(a)) for a in every])
    for i, a in enumerate(every):
        check_point(back[i], a, f"from_niels {i}", m.TIGHT)


def test_closure_of_accumulation_and_doubling():
    """64 successive ge_madd_fg into one accumulator (the bucket accumulation's
    loop) and 64 successive ge_dbl, each output fed back in: the limbs stay
    tight and the value right after every step."""
    special, random = point_sets()
    every = special + random
    pr = m.probe()
    acc_pts = list(every)
    rows = [words(a, i) for i, a in enumerate(acc_pts)]
    n = len(rows)
    nls = [m.niels_limbs(m.niels_of(b)) for b in every]
    for step in range(64):
        idx = [(i + 3 * step + 1) % n for i in range(n)]
        ops = [every[k] for k in idx]
        flag = [(i + step) & 1 for i in range(n)]
        rows, _ = pr.ge("madd_fg", rows, nl=[nls[k] for k in idx], flag=flag)
        acc_pts = [r255.ed_add(a, r255.ed_neg(b) if f else b) for a, b, f in zip(acc_pts, ops, flag)]
        for i in range(n):
            check_point(rows[i], acc_pts[i], f"madd_fg step {step} lane {i}")
    dbl_pts = list(every)
    rows = [words(a, i) for i, a in enumerate(dbl_pts)]
    for step in range(64):
        rows, _ = pr.ge("dbl", rows)
        dbl_pts = [r255.ed_double(a) for a in dbl_pts]
        for i in range(n):
            check_point(rows[i], dbl_pts[i], f"dbl step {step} lane {i}")


def test_ristretto_encode_is_constant_on_a_class():
    """MSM partials travel as raw extended points: every representative
    P + T (T in the 4-torsion), at any Z scaling and limb looseness, must
    encode to the oracle's encode(P)."""
    _, random = point_sets()
    rng = Rng(32, b"ge-cases")
    t4 = m.four_torsion()
    rows, want = [], []
    for a in random + [r255.IDENTITY, r255.BASEPOINT]:
        enc = r255.encode(a)
        for t in t4:
            rep = r255.ed_add(a, t)
            assert r255.encode(rep) == enc
            for k, z in enumerate((1, P - 1, rnd_fe(rng) or 3)):
                rows.append(words(m.scale(m.affine_point(rep), z), 5 * k))
                want.append(enc)
    _, aux = m.probe().ge("encode", rows)
    for i, (a, w) in enumerate(zip(aux, want)):
        assert m.from_words(a[:8]).to_bytes(32, "little") == w, i


def test_ristretto_decode_round_trip_and_eq():
    _, random = point_sets()
    rng = Rng(33, b"ge-cases")
    good = [r255.encode(a) for a in random + [r255.IDENTITY, r255.BASEPOINT]]
    bad = []
    while len(bad) < 24:
        b = bytearray(rng.bytes(32))
        b[31] &= 0x7F
        if len(bad) % 2:
            b[0] &= 0xFE
        bad.append(bytes(b))
    bad += [(P - 1).to_bytes(32, "little"), P.to_bytes(32, "little"), (1).to_bytes(32, "little"), b"\xff" * 32]
    encs = good + bad
    dummy = [words(r255.IDENTITY)] * len(encs)
    nl = [m.words8(int.from_bytes(e, "little")) + [0] * 24 for e in encs]
    pr = m.probe()
    out, aux = pr.ge("decode", dummy, nl=nl)
    oks = []
    for i, e in enumerate(encs):
        try:
            want = r255.decode(e)
        except r255.DecodeError:
            want = None
        assert aux[i][0] == int(want is not None), e.hex()
        if want is not None:
            check_point(out[i], want, f"decode {i}", m.TIGHT)
            oks.append(i)
    assert len(oks) >= len(good) and len(oks) < len(encs)
    _, aux = pr.ge("encode", [out[i] for i in oks])
    assert [m.from_words(a[:8]).to_bytes(32, "little") for a in aux] == [encs[i] for i in oks]
    # equality: true across torsion representatives, false otherwise
    t4 = m.four_torsion()
    pts = random[:8] + [r255.IDENTITY, r255.BASEPOINT]
    a, b, want = [], [], []
    for i, x in enumerate(pts):
        for j, t in enumerate(t4):
            a.append(words(m.scale(x, 7 + i), i))
            b.append(words(m.scale(r255.ed_add(x, t), rnd_fe(rng) or 5), j))
            want.append(1)
        for y in (pts[(i + 1) % len(pts)], r255.ed_neg(x), r255.ed_double(x)):
            a.append(words(x, i))
            b.append(words(m.scale(y, 11), 3))
            want.append(int(r255.equal(x, y)))
    assert 0 in want
    _, aux = pr.ge("eq", a, b)
    assert [x[0] for x in aux] == want


def test_elligator():
    rng = Rng(34, b"ge-cases")
    ts = [0, 1, P - 1, 2, r255.SQRT_M1] + [rnd_fe(rng) for _ in range(59)]
    rows = []
    for t in ts:
        rows.append(m.loose_any(t, m.TIGHT)[-1] + [0] * 30)
    out, _ = m.probe().ge("elligator", rows)
    for t, o in zip(ts, out):
        check_point(o, r255.elligator_map(t), f"elligator {t:#x}")
