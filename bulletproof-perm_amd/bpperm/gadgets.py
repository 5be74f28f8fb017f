"""Caller-defined circuits for bpp_circuit_* (include/bpperm.h): a builder that
writes the description arrays, and the gadgets built on it.  Pure Python: no
library call, no GPU.

    b = CircuitBuilder()
    v = b.input()
    l, r, o = b.mul(v - 3, v - 7)      # defined sides: linear combinations
    b.assert_zero(o)                   # v is 3 or 7
    desc = b.build()                   # -> CircuitDesc (the arrays of bpp_circuit_desc)

A linear combination (LC) is built from b.input(), b.challenge, b.public()
(a per-proof public input, bpp_circuit_create_pub), b.one, wires and integers with +, -, unary - and * by an integer; coefficients are mod l.
A defined side may read wires of EARLIER gates only.  b.free_mul() makes a gate
whose two sides are fed from the per-proof auxiliary values (its two aux
indices are 2t, 2t + 1 for the t-th free gate, left then right).

b.hint(op, lc, arg) makes one free side WITH the rule the prover derives its
value by (bpp_circuit_hints): aux = op(lc mod l), lc over {1, v_j, u_i}.  mul()
takes it on either side.  When every auxiliary value has a hint, build() emits
them (CircuitDesc.hints) and the prover needs no aux from its caller:

    inv = b.hint(HINT_INV, v0 - v1)
    b.assert_zero(b.mul(v0 - v1, inv)[2] - 1)   # v0 != v1

b.derived(op, lc, arg) is hint() over the whole variable space of a defined
side: lc may also read x and wires of EARLIER gates (a late hint,
bpp_circuit_create_wire_hinted).  The prover evaluates it inside the witness
kernel when it reaches the gate, so a free side can depend on a product formed
earlier in the same circuit:

    p = b.mul(v0 - v1, v0 - v2)[2]
    b.assert_zero(b.mul(p, b.derived(HINT_INV, p))[2] - 1)   # v0 is neither v1 nor v2
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Sequence

L = 2**252 + 27742317777372353535851937790883648493
SIDE_LC = 0xFFFFFFFF

_ONE, _V, _X, _U, _W = 0, 1, 2, 3, 4  # variable kinds, in id order (_U: public inputs)

# BPP_HINT_*: aux = w, bit `arg` of w, 1 - that bit, w^-1 (0 for 0), [w = 0]
HINT_VALUE, HINT_BIT, HINT_NOT_BIT, HINT_INV, HINT_IS_ZERO = 0, 1, 2, 3, 4


class LC:
    """A sparse linear combination: {(kind, index, part): coefficient mod l}."""

    __slots__ = ("t",)

    def __init__(self, terms=None):
        self.t = {k: c % L for k, c in (terms or {}).items() if c % L}

    @staticmethod
    def of(x) -> "LC":
        if isinstance(x, LC):
            return x
        if isinstance(x, int):
            return LC({(_ONE, 0, 0): x})
        raise TypeError(f"not a linear combination: {x!r}")

    def __add__(self, o):
        o = LC.of(o)
        t = dict(self.t)
        for k, c in o.t.items():
            t[k] = t.get(k, 0) + c
        return LC(t)

    __radd__ = __add__

    def __neg__(self):
        return LC({k: -c for k, c in self.t.items()})

    def __sub__(self, o):
        return self + (-LC.of(o))

    def __rsub__(self, o):
        return LC.of(o) - self

    def __mul__(self, a):
        if not isinstance(a, int):
            raise TypeError("an LC is scaled by an integer; products are gates (CircuitBuilder.mul)")
        return LC({k: c * a for k, c in self.t.items()})

    __rmul__ = __mul__


@dataclass
class CircuitHints:
    """The arrays of bpp_circuit_hints: one hint per auxiliary value.  op[t] =
    HINT_* | arg << 8; the terms of hint t are lc_var / lc_coef [lc_off[t],
    lc_off[t + 1])."""
    op: list
    lc_off: list
    lc_var: list
    lc_coef: list
    # a hint names x or a wire (CircuitBuilder.derived): bpp_circuit_create_wire_hinted takes these
    wire: bool = False


class Hint:
    """A free gate side with a hint (CircuitBuilder.hint): aux index `index`."""
    __slots__ = ("index",)

    def __init__(self, index: int):
        self.index = index


@dataclass
class CircuitDesc:
    """The arrays of bpp_circuit_desc.  lc_coef: one 32-byte little-endian
    scalar per term."""
    m_in: int
    n_gates: int
    n_aux: int
    n_asserts: int
    side_aux: list
    lc_off: list
    lc_var: list
    lc_coef: list
    # the gadget's hint function: v (m_in ints) -> aux (n_aux ints); None when n_aux = 0
    aux_of: "Callable[[Sequence[int]], list] | None" = field(default=None, compare=False)
    # public inputs u_0..u_{n_pub-1} (bpp_circuit_create_pub's argument, not an array of bpp_circuit_desc)
    n_pub: int = 0
    # the hint program (bpp_circuit_create_hinted), no part of the statement; None: aux is the caller's
    hints: "CircuitHints | None" = field(default=None, compare=False)

    def coef_bytes(self) -> bytes:
        return b"".join(self.lc_coef)


class CircuitBuilder:
    def __init__(self):
        self.m_in = 0
        self.n_pub = 0
        self.n_aux = 0
        self.sides = []    # per gate: [left, right], each an LC (defined) or an aux index (free)
        self.hints = []    # per aux value: (op, arg, LC), or None (the caller's)
        self.asserts = []
        self.one = LC({(_ONE, 0, 0): 1})
        self.challenge = LC({(_X, 0, 0): 1})

    def input(self) -> LC:
        self.m_in += 1
        return LC({(_V, self.m_in - 1, 0): 1})

    def inputs(self, n: int) -> list:
        return [self.input() for _ in range(n)]

    def public(self) -> LC:
        """The next public input u_i: per proof, given to prover and verifier,
        never committed."""
        self.n_pub += 1
        return LC({(_U, self.n_pub - 1, 0): 1})

    def publics(self, n: int) -> list:
        return [self.public() for _ in range(n)]

    def _wires(self, g: int):
        return tuple(LC({(_W, g, s): 1}) for s in range(3))

    def hint(self, op: int, lc, arg: int = 0) -> Hint:
        """A free side whose value the prover derives: aux = op(lc mod l), lc
        over {1, v_j, u_i} (neither x nor a wire: aux exists before x does);
        arg: the bit index of HINT_BIT / HINT_NOT_BIT.  For mul(), either side."""
        lc = LC.of(lc)
        if op not in (HINT_VALUE, HINT_BIT, HINT_NOT_BIT, HINT_INV, HINT_IS_ZERO):
            raise ValueError(f"hint: unknown op {op}")
        if not 0 <= arg <= 252 or (arg and op not in (HINT_BIT, HINT_NOT_BIT)):
            raise ValueError("hint: arg is a bit index <= 252, for HINT_BIT / HINT_NOT_BIT only")
        if any(kind in (_X, _W) for (kind, _i, _s) in lc.t):
            raise ValueError("hint: reads x or a wire")
        self.hints.append((op, arg, lc))
        self.n_aux += 1
        return Hint(self.n_aux - 1)

    def derived(self, op: int, lc, arg: int = 0) -> Hint:
        """hint() over {1, v_j, x, u_i, wires}: a free side whose value the
        prover derives when it reaches the gate (a late hint when lc reads x or
        a wire; bpp_circuit_create_wire_hinted).  The gate it feeds comes after
        every gate whose wire lc reads (mul() checks)."""
        lc = LC.of(lc)
        if op not in (HINT_VALUE, HINT_BIT, HINT_NOT_BIT, HINT_INV, HINT_IS_ZERO):
            raise ValueError(f"derived: unknown op {op}")
        if not 0 <= arg <= 252 or (arg and op not in (HINT_BIT, HINT_NOT_BIT)):
            raise ValueError("derived: arg is a bit index <= 252, for HINT_BIT / HINT_NOT_BIT only")
        self.hints.append((op, arg, lc))
        self.n_aux += 1
        return Hint(self.n_aux - 1)

    def mul(self, left, right):
        """A gate whose sides are defined (linear combinations) or hinted free
        sides (hint(), derived()); returns its wires (l, r, o)."""
        g = len(self.sides)
        sides = [s.index if isinstance(s, Hint) else LC.of(s) for s in (left, right)]
        for side in sides:
            for (kind, h, _s) in (side.t if isinstance(side, LC) else ()):
                if kind == _W and h >= g:
                    raise ValueError(f"gate {g}: a definition reads a wire of gate {h}")
            if not isinstance(side, LC) and side < len(self.hints) and self.hints[side] is not None:
                for (kind, h, _s) in self.hints[side][2].t:
                    if kind == _W and h >= g:
                        raise ValueError(f"gate {g}: a derived side reads a wire of gate {h}")
        self.sides.append(sides)
        return self._wires(g)

    def free_mul(self):
        """A gate with both sides free (aux indices n_aux, n_aux + 1); returns
        its wires (l, r, o)."""
        self.sides.append([self.n_aux, self.n_aux + 1])
        self.n_aux += 2
        self.hints += [None, None]
        return self._wires(len(self.sides) - 1)

    def assert_zero(self, lc):
        self.asserts.append(LC.of(lc))

    def build(self, aux_of=None) -> CircuitDesc:
        m_in, n, n_pub = self.m_in, len(self.sides), self.n_pub
        if not m_in or not n:
            raise ValueError("a circuit needs an input and a gate")

        def var_id(key):
            kind, i, s = key
            return {_ONE: 0, _V: 1 + i, _X: 1 + m_in, _U: 2 + m_in + i, _W: 2 + m_in + n_pub + 3 * i + s}[kind]

        side_aux, lc_off, lc_var, lc_coef = [], [0], [], []

        def emit(lc: LC, lc_off=lc_off, lc_var=lc_var, lc_coef=lc_coef):
            for vid, c in sorted((var_id(k), c) for k, c in lc.t.items()):
                lc_var.append(vid)
                lc_coef.append(c.to_bytes(32, "little"))
            lc_off.append(len(lc_var))

        for sides in self.sides:
            for s in sides:
                if isinstance(s, LC):
                    side_aux.append(SIDE_LC)
                    emit(s)
                else:
                    side_aux.append(s)
                    lc_off.append(len(lc_var))
        for a in self.asserts:
            emit(a)
        hints = None
        if self.n_aux and all(h is not None for h in self.hints):  # every aux value has a hint
            hints = CircuitHints([], [0], [], [])
            for op, arg, lc in self.hints:
                hints.op.append(op | arg << 8)
                emit(lc, hints.lc_off, hints.lc_var, hints.lc_coef)
                hints.wire = hints.wire or any(kind in (_X, _W) for (kind, _i, _s) in lc.t)
        return CircuitDesc(m_in, n, self.n_aux, len(self.asserts), side_aux, lc_off, lc_var, lc_coef, aux_of, n_pub,
                           hints)


# --------------------------------------------------------------------- gadgets

def two_half_shuffle(k: int) -> CircuitDesc:
    """bpp_perm_*'s statement as a program: v_0..v_{k-1} and v_k..v_{2k-1} hold
    the same multiset.  Compiles to exactly the two-half circuit's matrices: two
    product chains prod (v_i - x), a negation gate, a difference gate whose
    output is asserted 0."""
    if k < 2:
        raise ValueError("k >= 2")
    b = CircuitBuilder()
    v = b.inputs(2 * k)
    x = b.challenge
    o = [None] * (2 * k)
    for g in range(k - 1):  # chain A
        o[g] = b.mul(v[0] - x if g == 0 else o[g - 1], v[g + 1] - x)[2]
    for g in range(k - 1, 2 * k - 2):  # chain B
        o[g] = b.mul(v[k] - x if g == k - 1 else o[g - 1], v[g + 2] - x)[2]
    o[2 * k - 2] = b.mul(o[2 * k - 3], -1)[2]
    o[2 * k - 1] = b.mul(o[k - 2] + o[2 * k - 2], 1)[2]
    b.assert_zero(o[2 * k - 1])
    return b.build()


def member_of(values: Sequence[int]) -> CircuitDesc:
    """v_0 is one of `values`: prod (v_0 - s_i) = 0, len(values) - 1 gates (one
    gate for one or two values)."""
    s = [int(a) % L for a in values]
    if not s:
        raise ValueError("member_of: an empty set")
    b = CircuitBuilder()
    v = b.input()
    o = b.mul(v - s[0], v - s[1] if len(s) > 1 else 1)[2]
    for a in s[2:]:
        o = b.mul(o, v - a)[2]
    b.assert_zero(o)
    return b.build()


def _range_bits(b: CircuitBuilder, target: LC, nbits: int):
    """target < 2^nbits (target over {1, v_j, u_i}): a gate per bit with both
    sides free and hinted (l = the bit of target, r = 1 - it), an assert o = 0
    and an assert l + r - 1 = 0; one more assert covers the weighted bit sum."""
    total = LC()
    for i in range(nbits):
        l, r, o = b.mul(b.hint(HINT_BIT, target, i), b.hint(HINT_NOT_BIT, target, i))
        b.assert_zero(o)
        b.assert_zero(l + r - 1)
        total = total + l * (1 << i)
    b.assert_zero(total - target)


def _bits_aux(x: int, nbits: int) -> list:
    """_range_bits' auxiliary values for target = x."""
    out = []
    for i in range(nbits):
        bit = (x % L >> i) & 1
        out += [bit, 1 - bit]
    return out


def in_range(nbits: int) -> CircuitDesc:
    """v_0 < 2^nbits.  Each bit takes a gate with both sides free (l = bit, r =
    1 - bit), an assert o = 0 and an assert l + r - 1 = 0; one more assert
    covers the weighted bit sum.  aux_of(v) gives the 2 nbits hints."""
    if not 1 <= nbits <= 252:
        raise ValueError("1 <= nbits <= 252")
    b = CircuitBuilder()
    v = b.input()
    _range_bits(b, v, nbits)

    def aux_of(vals):
        x = int(vals[0]) % L
        out = []
        for i in range(nbits):
            bit = (x >> i) & 1
            out += [bit, 1 - bit]
        return out

    return b.build(aux_of)


def in_range_many(count: int, nbits: int) -> CircuitDesc:
    """v_0..v_{count-1} are each below 2^nbits, in one proof: in_range's bit
    gates for every value (count * nbits gates with both sides free, each with
    its asserts o = 0 and l + r - 1 = 0) and one weighted-sum assert per value.
    aux_of(v) gives the 2 count nbits hints, value-major.  16 values of 64 bits
    are 1024 gates: a large circuit (Circuit(desc, large=True))."""
    if count < 1:
        raise ValueError("count >= 1")
    if not 1 <= nbits <= 252:
        raise ValueError("1 <= nbits <= 252")
    b = CircuitBuilder()
    vs = b.inputs(count)
    for v in vs:
        _range_bits(b, v, nbits)

    def aux_of(vals):
        out = []
        for j in range(count):
            x = int(vals[j]) % L
            for i in range(nbits):
                bit = (x >> i) & 1
                out += [bit, 1 - bit]
        return out

    return b.build(aux_of)


def not_equal() -> CircuitDesc:
    """v_0 != v_1: (v_0 - v_1) * inv = 1, one gate whose right side is free and
    hinted with the inverse of the difference.  Equal cards: the hint is 0 and
    the assert o - 1 = 0 does not hold."""
    return distinct(2)


def distinct(k: int) -> CircuitDesc:
    """v_0..v_{k-1} are pairwise different ("my hand has no repeated card"):
    not_equal over all pairs i < j in lexicographic order, k (k - 1) / 2 gates,
    one hint and one assert each."""
    if k < 2:
        raise ValueError("k >= 2")
    b = CircuitBuilder()
    v = b.inputs(k)
    pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]
    for i, j in pairs:
        b.assert_zero(b.mul(v[i] - v[j], b.hint(HINT_INV, v[i] - v[j]))[2] - 1)

    def aux_of(vals):
        d = [(int(vals[i]) - int(vals[j])) % L for i, j in pairs]
        return [pow(x, -1, L) if x else 0 for x in d]

    return b.build(aux_of)


def less_than(nbits: int) -> CircuitDesc:
    """v_0 < v_1, both below 2^nbits: v_0, v_1 and v_1 - v_0 - 1 are each below
    2^nbits (in_range's bit gates over each), 3 nbits gates.  nbits <= 250, so
    that no sum of two such values wraps mod l."""
    return ascending(2, nbits)


def ascending(k: int, nbits: int) -> CircuitDesc:
    """v_0 < v_1 < .. < v_{k-1}, all below 2^nbits ("my hand is in ascending
    order"): every v_i, then every v_{i+1} - v_i - 1, below 2^nbits;
    (2k - 1) nbits gates."""
    if k < 2:
        raise ValueError("k >= 2")
    if not 1 <= nbits <= 250:
        raise ValueError("1 <= nbits <= 250")
    b = CircuitBuilder()
    v = b.inputs(k)
    for x in v:
        _range_bits(b, x, nbits)
    for i in range(k - 1):
        _range_bits(b, v[i + 1] - v[i] - 1, nbits)

    def aux_of(vals):
        x = [int(a) % L for a in vals]
        out = []
        for a in x:
            out += _bits_aux(a, nbits)
        for i in range(k - 1):
            out += _bits_aux(x[i + 1] - x[i] - 1, nbits)
        return out

    return b.build(aux_of)


def same_multiset(k: int) -> CircuitDesc:
    """Two hidden hands v_0..v_{k-1} and v_k..v_{2k-1} hold the same multiset:
    prod (v_i - x) over each hand, 2k - 2 gates, one assert on the difference
    of the two products."""
    if k < 2:
        raise ValueError("k >= 2")
    b = CircuitBuilder()
    v = b.inputs(2 * k)
    x = b.challenge
    ends = []
    for base in (0, k):
        o = b.mul(v[base] - x, v[base + 1] - x)[2]
        for i in range(2, k):
            o = b.mul(o, v[base + i] - x)[2]
        ends.append(o)
    b.assert_zero(ends[0] - ends[1])
    return b.build()


# ------------------------------------- gadgets whose hints read earlier wires

def derive_aux(desc: CircuitDesc, vals: Sequence[int]) -> list:
    """The n_aux auxiliary values of a description whose hints read neither x
    nor a public input, from v alone: the hints over {1, v_j} first, then the
    gates in order, each late hint from the wires so far (what the prover's
    witness kernel does).  The aux_of of the gadgets below."""
    h, m_in = desc.hints, desc.m_in
    wbase = 2 + m_in + desc.n_pub
    v = [int(a) % L for a in vals]
    wires = [0] * (3 * desc.n_gates)

    def lc(off, var, coef, i):
        w = 0
        for e in range(off[i], off[i + 1]):
            vid = var[e]
            if vid == 0:
                val = 1
            elif vid <= m_in:
                val = v[vid - 1]
            elif vid < wbase:
                raise ValueError("derive_aux: the combination reads x or a public input")
            else:
                val = wires[vid - wbase]
            w += int.from_bytes(coef[e], "little") * val
        return w % L

    def hint(t):
        w = lc(h.lc_off, h.lc_var, h.lc_coef, t)
        op, arg = h.op[t] & 0xFF, h.op[t] >> 8
        return {HINT_VALUE: w, HINT_BIT: (w >> arg) & 1, HINT_NOT_BIT: 1 - ((w >> arg) & 1),
                HINT_INV: pow(w, L - 2, L), HINT_IS_ZERO: int(w == 0)}[op]

    late = [any(x >= wbase for x in h.lc_var[h.lc_off[t]:h.lc_off[t + 1]]) for t in range(desc.n_aux)]
    aux = [0 if late[t] else hint(t) for t in range(desc.n_aux)]
    for g in range(desc.n_gates):
        for s in range(2):
            a = desc.side_aux[2 * g + s]
            if a != SIDE_LC and late[a]:
                aux[a] = hint(a)
            wires[3 * g + s] = lc(desc.lc_off, desc.lc_var, desc.lc_coef, 2 * g + s) if a == SIDE_LC else aux[a]
        wires[3 * g + 2] = wires[3 * g] * wires[3 * g + 1] % L
    return aux


def _with_derived_aux(b: CircuitBuilder) -> CircuitDesc:
    desc = b.build()
    desc.aux_of = lambda vals: derive_aux(desc, vals)
    return desc


def _derived_bits(b: CircuitBuilder, target: LC, nbits: int):
    """_range_bits with derived() in place of hint(): target may read wires of
    earlier gates.  Returns the (l, r) wires of each bit's gate: the bit and
    1 - the bit."""
    total, out = LC(), []
    for i in range(nbits):
        l, r, o = b.mul(b.derived(HINT_BIT, target, i), b.derived(HINT_NOT_BIT, target, i))
        b.assert_zero(o)
        b.assert_zero(l + r - 1)
        total = total + l * (1 << i)
        out.append((l, r))
    b.assert_zero(total - target)
    return out


def max_of(k: int, nbits: int) -> CircuitDesc:
    """v_0..v_{k-1} are below 2^nbits and v_k is their maximum.  Every v_i takes
    in_range's nbits bit gates.  The running maximum M_0 = v_0, M_i = v_i + o_i:
    step i decomposes d_i = v_i - M_{i-1} - 1 + 2^nbits into nbits + 1 bits, whose
    top bit c_i says v_i > M_{i-1}, and a gate (1 - c_i) (M_{i-1} - v_i) = o_i.
    From step 2 on d_i reads the gate output o_{i-1}: its bits are late hints.
    The last assert is M_{k-1} - v_k = 0.  k nbits + (k - 1)(nbits + 2) gates;
    nbits <= 249."""
    if k < 1:
        raise ValueError("k >= 1")
    if not 1 <= nbits <= 249:
        raise ValueError("1 <= nbits <= 249")
    b = CircuitBuilder()
    v = b.inputs(k + 1)
    for x in v[:k]:
        _range_bits(b, x, nbits)
    m = v[0]
    for i in range(1, k):
        bits = _derived_bits(b, v[i] - m - 1 + (1 << nbits), nbits + 1)
        m = v[i] + b.mul(bits[nbits][1], m - v[i])[2]
    b.assert_zero(m - v[k])
    return _with_derived_aux(b)


def not_among(k: int) -> CircuitDesc:
    """v_0 differs from each of v_1..v_k ("my card is none of those"): the
    product of the k differences over k - 1 gates, then one gate p * p^-1 whose
    free side is the inverse of the product wire (a late hint for k >= 2) and
    one assert o - 1 = 0.  A repeat makes p = 0: the hint is 0 and the assert
    does not hold."""
    if k < 1:
        raise ValueError("k >= 1")
    b = CircuitBuilder()
    v = b.inputs(k + 1)
    p = v[0] - v[1]
    for j in range(2, k + 1):
        p = b.mul(p, v[0] - v[j])[2]
    b.assert_zero(b.mul(p, b.derived(HINT_INV, p))[2] - 1)
    return _with_derived_aux(b)


def blackjack_total(k: int) -> CircuitDesc:
    """The k hidden ranks v_i are in 1..13 and the public u_0 is the hand's
    blackjack total S + 10 soft: S = sum min(v_i, 10), soft = 1 exactly when some
    v_i = 1 and S <= 11.  Per card: v_i - 1 and 13 - v_i in 4 bits (the rank
    range), v_i + 5 in 5 bits whose top bit f_i says v_i >= 11, a gate f_i (v_i -
    10) = q_i (min(v_i, 10) = v_i - q_i), and is-zero of v_i - 1 over two gates
    (w inv = 1 - a_i, w a_i = 0).  Then the chain prod (1 - a_i), the bits of d =
    11 - S + 2^B (late hints: S reads every q_i), whose top bit says S <= 11, a
    gate (1 - prod) * that bit = soft, and the assert u_0 - S - 10 soft = 0."""
    if k < 1:
        raise ValueError("k >= 1")
    b = CircuitBuilder()
    v = b.inputs(k)
    u = b.public()
    S, none = LC(), None
    for x in v:
        _range_bits(b, x - 1, 4)
        _range_bits(b, 13 - x, 4)
        n0 = len(b.sides)
        _range_bits(b, x + 5, 5)
        face = b._wires(n0 + 4)[0]
        S = S + x - b.mul(face, x - 10)[2]
        o1 = b.mul(x - 1, b.hint(HINT_INV, x - 1))[2]
        _l, ace, o2 = b.mul(x - 1, b.hint(HINT_IS_ZERO, x - 1))
        b.assert_zero(o2)
        b.assert_zero(o1 - 1 + ace)
        none = 1 - ace if none is None else b.mul(none, 1 - ace)[2]
    B = max(4, (10 * k - 11).bit_length())  # (2^B > 10 k - 11 >= S - 11: d >= 0, and its bit B says S <= 11)
    low = _derived_bits(b, 11 - S + (1 << B), B + 1)[B][0]
    soft = b.mul(1 - none, low)[2]
    b.assert_zero(u - S - 10 * soft)
    return _with_derived_aux(b)


# ------------------------------------------------- gadgets over public inputs

def opens_to() -> CircuitDesc:
    """V_0 opens to the public value u_0: one gate (v_0 - u_0) * 1 whose output
    is asserted 0.  The prover shows a commitment's value without giving up its
    blinding."""
    b = CircuitBuilder()
    v, u = b.input(), b.public()
    b.assert_zero(b.mul(v - u, 1)[2])
    return b.build()


def member_of_public(n: int) -> CircuitDesc:
    """v_0 is one of the n public values of this proof: prod_{i<n} (v_0 - u_i) =
    0, n - 1 gates (one gate for n = 1 or 2).  member_of with the set given per
    proof: one circuit and one digest for every trick."""
    if n < 1:
        raise ValueError("member_of_public: an empty set")
    b = CircuitBuilder()
    v = b.input()
    u = b.publics(n)
    o = b.mul(v - u[0], v - u[1] if n > 1 else 1)[2]
    for a in u[2:]:
        o = b.mul(o, v - a)[2]
    b.assert_zero(o)
    return b.build()


def sum_equals(k: int) -> CircuitDesc:
    """v_0 + .. + v_{k-1} = u_0, the announced total.  The statement is one
    assert; the one gate v_0 * 1 is there because a circuit has a gate."""
    if k < 1:
        raise ValueError("k >= 1")
    b = CircuitBuilder()
    v = b.inputs(k)
    u = b.public()
    b.mul(v[0], 1)
    total = LC()
    for x in v:
        total = total + x
    b.assert_zero(total - u)
    return b.build()


def shuffle_of_public(k: int) -> CircuitDesc:
    """V_0..V_{k-1} commit to a permutation of this proof's public deck
    u_0..u_{k-1}: a chain prod (v_j - x), a chain prod (u_j - x), and an assert
    on the difference of their ends.  2k - 2 gates, m_in = k, n_pub = k."""
    if k < 2:
        raise ValueError("k >= 2")
    b = CircuitBuilder()
    v = b.inputs(k)
    u = b.publics(k)
    x = b.challenge
    ends = []
    for w in (v, u):
        o = b.mul(w[0] - x, w[1] - x)[2]
        for i in range(2, k):
            o = b.mul(o, w[i] - x)[2]
        ends.append(o)
    b.assert_zero(ends[0] - ends[1])
    return b.build()
