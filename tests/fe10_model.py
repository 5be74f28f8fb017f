"""Model of the device arithmetic's number formats, for the tests of
bulletproof-perm_amd/probe/arith_probe.hip (test_gpu_arith_*.py).

Field elements are 10 limbs of radix 2^25.5 (fe25519.cuh): limb i sits at bit
OFF[i] = ceil(25.5 i) and is W[i] = 26 (even i) or 25 (odd i) bits wide when
exact.  The bounds below are the ones the headers state, by name; the case
generators put limbs exactly under them.  Scalars are 8 little-endian 32-bit
words.  `ref_digits` is the signed-window recoding the MSM kernels implement
(W = ceil(254 / c) windows; oracle.ristretto.signed_digits uses ceil(256 / w)).

Randomness: oracle.merlin.Rng with fixed seeds.  `Probe` binds the probe's
C interface (libbpperm_probe.so) and is only constructed by GPU tests.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
from pathlib import Path

from oracle import ristretto as r255
from oracle.merlin import Rng

P = r255.P
L = r255.L
DELTA = L - 2**252
N = 10
W = [26 if i % 2 == 0 else 25 for i in range(N)]
OFF = [math.ceil(25.5 * i) for i in range(N)]
assert OFF == [0, 26, 51, 77, 102, 128, 153, 179, 204, 230] and OFF[9] + W[9] == 255

# ---------------------------------------------------------------- bounds
# (exclusive; per limb).  fe25519.cuh names them:
EXACT = [1 << w for w in W]                      # fe_canon's output
TIGHT = [(1 << w) + (1 << 18) for w in W]        # "tight": limb i < 2^w_i + 2^18
ADD_NC = [(1 << 27) + (1 << 19)] * N             # fe_add_nc of tight operands
SUB_NC = [(1 << 27) + (1 << 26) + (1 << 18)] * N  # fe_sub_nc of tight operands
G_BOUND = [(1 << 27) + (1 << 26) + (1 << 19) + (1 << 18)] * N  # G = fe_add_nc(fe_add_nc(Z, Z), C)
MUL_IN = [int(2 ** 27.6)] * N                    # fe_mul / fe_sq operands: limbs < 2^27.6
CARRY_IN = [(1 << 32) - (1 << 7)] * N            # fe_carry's input (no 32-bit wrap of limb + carry)
CARRY_OUT = [(1 << 26) + 19 * (1 << 7)] + EXACT[1:]  # fe_carry's output: limb 0 < 2^26 + 19 * 2^7
MUL_OUT = [1 << 26, (1 << 25) + (1 << 18)] + EXACT[2:]  # fe10_ops.inc: limb 1 < 2^25 + 2^18
# the limbs of 2p that fe_sub / fe_sub_nc add before subtracting
TWO_P = [0x7FFFFDA] + [0x3FFFFFE if i % 2 else 0x7FFFFFE for i in range(1, N)]
assert sum(v << o for v, o in zip(TWO_P, OFF)) == 2 * P
assert all(t - 1 <= tp for t, tp in zip(TIGHT, TWO_P))  # a tight limb is a valid subtrahend

NAMED_BOUNDS = {"exact": EXACT, "tight": TIGHT, "add_nc": ADD_NC, "sub_nc": SUB_NC, "g": G_BOUND, "mul_in": MUL_IN}


def raw_value(limbs) -> int:
    return sum(int(v) << o for v, o in zip(limbs, OFF))


def value(limbs) -> int:
    return raw_value(limbs) % P


def within(limbs, bound) -> bool:
    return all(0 <= int(v) < b for v, b in zip(limbs, bound))


def exact_limbs(v: int) -> list[int]:
    """v < 2^256 in exact-width limbs, the excess over 2^255 in limb 9."""
    assert 0 <= v < 1 << 256
    out = [(v >> OFF[i]) & ((1 << W[i]) - 1) for i in range(9)]
    out.append(v >> OFF[9])
    return out


def words8(v: int) -> list[int]:
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_words(ws) -> int:
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


# ---------------------------------------------------------------- field cases
def all_at(bound) -> list[int]:
    """Every limb at bound - 1."""
    return [b - 1 for b in bound]


def one_hot(bound) -> list[list[int]]:
    """For each position: that limb at bound - 1 and the rest 0, and the complement."""
    out = []
    for i in range(N):
        out.append([bound[j] - 1 if j == i else 0 for j in range(N)])
        out.append([0 if j == i else bound[j] - 1 for j in range(N)])
    return out


def random_under(bound, rng: Rng, n: int) -> list[list[int]]:
    out = []
    for _ in range(n):
        raw = rng.bytes(8 * N)
        out.append([int.from_bytes(raw[8 * i: 8 * i + 8], "little") % bound[i] for i in range(N)])
    return out


AROUND_MODULUS = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2**255 - 1, 2**255, 2**255 + 18, 2**255 + 19,
                  2**256 - 1]


def ripple_cases() -> list[list[int]]:
    """Limbs 1..9 at their exact maximum, limb 0 stepping through
    2^26 - 20 .. 2^26 + 19 * 128: fe_canon's "cannot ripple further"."""
    top = [b - 1 for b in EXACT[1:]]
    return [[v0] + top for v0 in range((1 << 26) - 20, (1 << 26) + 19 * 128 + 1)]


def loose(v: int, bound, m: int = 0, excess=None):
    """Limbs under `bound` (every bound[i] >= 2^W[i]) whose integer value is
    v + m p, with limb i carrying `excess[i]` above its exact part (default:
    the most the bound allows).  None when v + m p does not fit."""
    v %= P
    if excess is None:
        excess = [b - (1 << w) for b, w in zip(bound, W)]
    rest = v + m * P - raw_value(excess)
    if not 0 <= rest < 1 << 255:
        return None
    out = [e + x for e, x in zip(exact_limbs(rest), excess)]
    assert within(out, bound) and raw_value(out) == v + m * P
    return out


def loose_any(v: int, bound, excess=None) -> list[list[int]]:
    """The representations v + m p (as integers) that fit, for the smallest
    such m's (at most three: v, v + p, v + 2p under a tight bound; a looser
    bound's maximum excess alone exceeds 2p, so its m's start higher)."""
    out = [loose(v, bound, m, excess) for m in range(16)]
    out = [x for x in out if x is not None][:3]
    assert out, "no representation fits"
    return out


def field_classes(rng: Rng, nrand: int = 512, names=("exact", "tight", "add_nc", "sub_nc", "g", "mul_in")):
    """[(label, limbs)]: all-at-bound, one-hot and complement, and `nrand`
    random vectors, for each named bound."""
    out = []
    for name in names:
        b = NAMED_BOUNDS[name]
        out.append((f"{name}/max", all_at(b)))
        out += [(f"{name}/onehot{k}", x) for k, x in enumerate(one_hot(b))]
        out += [(f"{name}/rand{k}", x) for k, x in enumerate(random_under(b, rng, nrand))]
    return out


# ---------------------------------------------------------------- scalars
def sc_edge_values() -> list[int]:
    ones29 = [sum(((1 << 29) - 1) << (29 * i) for i in range(k)) for k in range(1, 10)]
    ones32 = [(1 << (32 * k)) - 1 for k in range(1, 9)]
    vals = [0, 1, 2, L - 2, L - 1, (L - 1) // 2, (L + 1) // 2, 2**252, 2**252 - 1]
    for x in ones29 + ones32:
        x &= (1 << 256) - 1
        while x >= L:  # truncated below l
            x >>= 1
        vals.append(x)
    return sorted(set(vals))


def reduce256_cases() -> list[int]:
    out = []
    for q in range(16):
        for r in (0, 1, q * DELTA - 1, q * DELTA, q * DELTA + 1, 2**252 - 1):
            if 0 <= r < 2**252:
                out.append(q * 2**252 + r)
    out.append(2**256 - 1)
    return out


# ---------------------------------------------------------------- digits
def windows(c: int) -> int:
    return (254 + c - 1) // c


def ref_digits(s: int, c: int) -> list[int]:
    """The device rule (msm_kernels.cuh for_each_digit): v >= 2^(c-1) and not
    the top window -> v - 2^c, carry 1."""
    assert 0 <= s < 1 << 253
    Wn = windows(c)
    half, mask = 1 << (c - 1), (1 << c) - 1
    out, carry = [], 0
    for w in range(Wn):
        v = ((s >> (c * w)) & mask) + carry
        if v >= half and w + 1 < Wn:
            out.append(v - (1 << c))
            carry = 1
        else:
            out.append(v)
            carry = 0
    return out


def ref_K(c: int) -> int:
    """sum_{w < W-1} 2^(c w + c - 1): the closed-form recoding's offset."""
    return sum(1 << (c * w + c - 1) for w in range(windows(c) - 1))


def digit_scalars(c: int, rng: Rng, nrand: int = 64) -> list[int]:
    Wn = windows(c)
    half, top = 1 << (c - 1), (1 << c) - 1
    rep = lambda x: sum(x << (c * w) for w in range(Wn))
    vals = [0, 1, L - 1, L - 2, 2**252, rep(half - 1), rep(half), rep(half + 1), rep(top),
            sum((top if w % 2 == 0 else 0) << (c * w) for w in range(Wn)),
            sum((top if w % 2 == 1 else 0) << (c * w) for w in range(Wn))]
    for w in range(Wn):  # a carry arriving exactly at the threshold
        vals.append(((1 << (c * w)) - 1) + ((half - 1) << (c * w)))
    vals += [rng.scalar() for _ in range(nrand)]
    return [v % L for v in vals]


def dig16(d: int) -> int:
    """k_msm_digits' 16-bit code: 0x7FFF for zero, else sign << 15 | (|d| - 1)."""
    return 0x7FFF if d == 0 else ((abs(d) - 1) | (0x8000 if d < 0 else 0))


# ---------------------------------------------------------------- points
def small_order_points():
    """The eight points of order dividing 8 (extended, Z = 1)."""
    # l times a curve point clears its prime-order part; keep the first result
    # of order exactly 8 and list its multiples
    rng = Rng(8, b"fe10-torsion")
    while True:
        y = int.from_bytes(rng.bytes(32), "little") % P
        # on the curve: x^2 = (y^2 - 1) / (d y^2 + 1)
        ok, x = r255.sqrt_ratio_m1((y * y - 1) % P, (r255.D * y * y + 1) % P)
        if not ok:
            continue
        t8 = r255.ed_mul(L, (x, y, 1, x * y % P))
        pts = [r255.IDENTITY]
        while len(pts) < 8:
            nxt = r255.ed_add(pts[-1], t8)
            if r255.ed_affine(nxt) == (0, 1):
                break
            pts.append(nxt)
        if len(pts) == 8:
            return [affine_point(p) for p in pts]


def affine_point(p):
    x, y = r255.ed_affine(p)
    return (x, y, 1, x * y % P)


def four_torsion():
    """The points T with 4 T = identity (the ristretto class of P is P + T)."""
    return [p for p in small_order_points() if r255.ed_affine(r255.ed_double(r255.ed_double(p))) == (0, 1)]


def scale(p, z: int):
    """The same point with its projective coordinates multiplied by z != 0."""
    return tuple(c * z % P for c in p)


def p3_limbs(p, bound=TIGHT, ms=(0, 0, 0, 0)) -> list[int]:
    """40 words (X, Y, Z, T) with every coordinate at maximum looseness under
    `bound`; coordinate k represented as v + ms[k] p when that fits, else v."""
    out = []
    for v, m in zip(p, ms):
        x = loose(v, bound, m) or loose(v, bound, 0) or loose(v, bound, 1)
        assert x is not None
        out += x
    return out


def p3_point(words) -> tuple:
    return tuple(value(words[10 * k: 10 * k + 10]) for k in range(4))


def niels_of(p) -> tuple:
    x, y = r255.ed_affine(p)
    return ((y + x) % P, (y - x) % P, 2 * r255.D * x * y % P)


def niels_limbs(nl, bound=TIGHT) -> list[int]:
    """32 words: (y+x, y-x, 2dxy) at maximum looseness, two words of padding."""
    out = []
    for v in nl:
        out += loose(v, bound, 0) or loose(v, bound, 1)
    return out + [0, 0]


# ---------------------------------------------------------------- the probe
FE_OPS = ["carry", "add", "sub", "neg", "add_nc", "sub_nc", "mul", "sq", "mul_small", "canon", "pred", "abs", "invert",
          "pow22523", "load_words", "store_words", "words_canonical", "sqrt_ratio_m1"]
SC_OPS = ["add", "sub", "neg", "mont", "mont_cios", "to_mont", "from_mont", "half", "reduce256", "from_wide",
          "wave_sum", "shfl"]
GE_OPS = ["madd", "msub", "madd_signed", "madd_fg", "madd_h1h2", "add", "add_quad", "dbl", "neg", "niels_from_affine",
          "to_niels", "from_niels", "encode", "decode", "eq", "elligator"]
FE_OUT_WORDS = 12
GE_AUX_WORDS = 32


def _u32(vals):
    vals = list(vals)
    return (C.c_uint32 * max(1, len(vals)))(*vals)


class Probe:
    """ctypes binding of bpperm/libbpperm_probe.so (BPP_PROBE_LIB selects
    another build).  Every call is one kernel launch over its cases."""

    def __init__(self):
        default = Path(__file__).resolve().parent.parent / "bulletproof-perm_amd" / "bpperm" / "libbpperm_probe.so"
        self.lib = C.CDLL(os.environ.get("BPP_PROBE_LIB") or str(default))

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: HIP error {rc}")

    def fe(self, op: str, a, b=None) -> list[list[int]]:
        """a, b: lists of 10-limb vectors -> list of FE_OUT_WORDS-word rows."""
        n = len(a)
        b = a if b is None else b
        assert len(b) == n and all(len(x) == N for x in a) and all(len(x) == N for x in b)
        out = (C.c_uint32 * max(1, FE_OUT_WORDS * n))()
        rc = self.lib.bpp_probe_fe(C.c_uint32(FE_OPS.index(op)), _u32(v for x in a for v in x),
                                   _u32(v for x in b for v in x), out, C.c_size_t(n))
        self._check(rc, f"bpp_probe_fe({op})")
        return [list(out[FE_OUT_WORDS * i: FE_OUT_WORDS * (i + 1)]) for i in range(n)]

    def sc(self, op: str, a, b=None) -> list[int]:
        """a, b: integers < 2^256 -> integers."""
        n = len(a)
        b = [0] * n if b is None else b
        assert len(b) == n
        out = (C.c_uint32 * max(1, 8 * n))()
        rc = self.lib.bpp_probe_sc(C.c_uint32(SC_OPS.index(op)), _u32(w for x in a for w in words8(x)),
                                   _u32(w for x in b for w in words8(x)), out, C.c_size_t(n))
        self._check(rc, f"bpp_probe_sc({op})")
        return [from_words(out[8 * i: 8 * i + 8]) for i in range(n)]

    def ge(self, op: str, p, q=None, nl=None, flag=None):
        """p, q: 40-word rows; nl: 32-word rows; flag: ints -> (out rows of 40, aux rows of 32)."""
        n = len(p)
        q = p if q is None else q
        nl = [[0] * 32] * n if nl is None else nl
        flag = [0] * n if flag is None else flag
        assert len(q) == n and len(nl) == n and len(flag) == n
        assert all(len(x) == 40 for x in p) and all(len(x) == 40 for x in q) and all(len(x) == 32 for x in nl)
        out = (C.c_uint32 * max(1, 40 * n))()
        aux = (C.c_uint32 * max(1, GE_AUX_WORDS * n))()
        rc = self.lib.bpp_probe_ge(C.c_uint32(GE_OPS.index(op)), _u32(v for x in p for v in x),
                                   _u32(v for x in q for v in x), _u32(v for x in nl for v in x), _u32(flag), out, aux,
                                   C.c_size_t(n))
        self._check(rc, f"bpp_probe_ge({op})")
        return ([list(out[40 * i: 40 * i + 40]) for i in range(n)],
                [list(aux[GE_AUX_WORDS * i: GE_AUX_WORDS * (i + 1)]) for i in range(n)])

    def geom(self, c: int) -> dict:
        g = (C.c_uint32 * 22)()
        self._check(self.lib.bpp_probe_geom(C.c_uint32(c), g), "bpp_probe_geom")
        return {"W": g[0], "B": g[1], "tfb": g[2], "K": from_words(g[3:11]), "NC": g[11],
                "dt_W": g[12], "dt_H": g[13], "dt_K": from_words(g[14:22])}

    def _scal(self, scalars):
        return _u32(w for s in scalars for w in words8(s))

    def for_each_digit(self, c: int, wb: int, Wn: int, scalars) -> list[list[int]]:
        n = len(scalars)
        out = (C.c_int32 * max(1, n * Wn))()
        rc = self.lib.bpp_probe_for_each_digit(C.c_uint32(c), C.c_uint32(wb), C.c_uint32(Wn), self._scal(scalars),
                                               C.c_size_t(n), out)
        self._check(rc, "bpp_probe_for_each_digit")
        return [list(out[Wn * i: Wn * (i + 1)]) for i in range(n)]

    def msm_digits(self, c: int, wb: int, Wn: int, scalars) -> list[list[int]]:
        """-> per scalar, the Wn 16-bit codes."""
        n = len(scalars)
        out = (C.c_uint16 * max(1, n * Wn))()
        rc = self.lib.bpp_probe_msm_digits(C.c_uint32(c), C.c_uint32(wb), C.c_uint32(Wn), self._scal(scalars),
                                           C.c_size_t(n), out)
        self._check(rc, "bpp_probe_msm_digits")
        return [[out[w * n + i] for w in range(Wn)] for i in range(n)]

    def rsort_digits_count(self, c: int, wb: int, Wn: int, scalars, NC: int):
        """-> (codes per scalar, cntA[w][bin], bins per scalar)."""
        n = len(scalars)
        dig = (C.c_uint16 * max(1, n * Wn))()
        cnt = (C.c_uint32 * max(1, Wn * NC))()
        bins = (C.c_uint32 * max(1, n * Wn))()
        rc = self.lib.bpp_probe_rsort_digits_count(C.c_uint32(c), C.c_uint32(wb), C.c_uint32(Wn), self._scal(scalars),
                                                   C.c_size_t(n), dig, cnt, bins)
        self._check(rc, "bpp_probe_rsort_digits_count")
        return ([[dig[w * n + i] for w in range(Wn)] for i in range(n)],
                [list(cnt[NC * w: NC * (w + 1)]) for w in range(Wn)],
                [[bins[w * n + i] for w in range(Wn)] for i in range(n)])

    def dt_rows(self, c: int, gen: int, scalars) -> list[list[tuple]]:
        n, Wn = len(scalars), windows(c)
        out = (C.c_uint32 * max(1, 3 * n * Wn))()
        rc = self.lib.bpp_probe_dt_rows(C.c_uint32(c), C.c_uint32(gen), self._scal(scalars), C.c_size_t(n), out)
        self._check(rc, "bpp_probe_dt_rows")
        return [[tuple(out[3 * (i * Wn + w): 3 * (i * Wn + w) + 3]) for w in range(Wn)] for i in range(n)]


_probe = None


def probe() -> Probe:
    global _probe
    if _probe is None:
        _probe = Probe()
    return _probe
