"""Plain-Python reference of hints over wires and x (bpp_circuit_create_wire_hinted),
written from the semantics in include/bpperm.h and from the description arrays
alone: it reads neither a gadget's aux_of nor gadgets.derive_aux.

    ids (those of bpp_circuit_desc.lc_var): 0 = one, 1 + j = v_j, 1 + m_in = x,
    2 + m_in + i = u_i, 2 + m_in + n_pub + 3h + {0, 1, 2} = l_h, r_h, o_h
    aux_t = op_t(w_t), w_t = sum coef * value over the hint's terms, mod l
    VALUE w | BIT bit arg of w | NOT_BIT 1 - it | INV w^-1 (0 for 0) | IS_ZERO [w = 0]
    a hint that names x or a wire is late: evaluated when the gates, taken in
    order, reach a side it feeds, from the wires so far; never, when it feeds none
"""
from __future__ import annotations

from dataclasses import dataclass, field

L = 2**252 + 27742317777372353535851937790883648493
VALUE, BIT, NOT_BIT, INV, IS_ZERO = 0, 1, 2, 3, 4
SIDE_LC = 0xFFFFFFFF
K_LDS_MAX = 64 * 1024


def _op(word: int, w: int) -> int:
    op, arg = word & 0xFF, word >> 8
    if op == VALUE:
        return w
    if op == BIT:
        return (w >> arg) & 1
    if op == NOT_BIT:
        return 1 - ((w >> arg) & 1)
    if op == INV:
        return pow(w, L - 2, L)
    if op == IS_ZERO:
        return 1 if w == 0 else 0
    raise ValueError(f"unknown op {op}")


def is_late(desc, t: int) -> bool:
    h, x_id, wbase = desc.hints, 1 + desc.m_in, 2 + desc.m_in + getattr(desc, "n_pub", 0)
    return any(var == x_id or var >= wbase for var in h.lc_var[h.lc_off[t]:h.lc_off[t + 1]])


def witness(desc, v, x: int, pub=None):
    """-> (aux [n_aux], a_L, a_R, a_O [n each], 1 + the first failing assert or 0)."""
    h, m_in, n = desc.hints, desc.m_in, desc.n_gates
    n_pub = getattr(desc, "n_pub", 0)
    wbase = 2 + m_in + n_pub
    pub = [u % L for u in (pub or [])]
    v = [a % L for a in v]
    wires = [0] * (3 * n)

    def lc(off, var, coef, i):
        w = 0
        for e in range(off[i], off[i + 1]):
            vid = var[e]
            if vid == 0:
                val = 1
            elif vid <= m_in:
                val = v[vid - 1]
            elif vid == 1 + m_in:
                val = x % L
            elif vid < wbase:
                val = pub[vid - 2 - m_in]
            else:
                val = wires[vid - wbase]
            w += int.from_bytes(coef[e], "little") * val
        return w % L

    hint = lambda t: _op(h.op[t], lc(h.lc_off, h.lc_var, h.lc_coef, t))
    late = [is_late(desc, t) for t in range(desc.n_aux)]
    aux = [0 if late[t] else hint(t) for t in range(desc.n_aux)]
    for g in range(n):
        for s in range(2):
            a = desc.side_aux[2 * g + s]
            if a == SIDE_LC:
                wires[3 * g + s] = lc(desc.lc_off, desc.lc_var, desc.lc_coef, 2 * g + s)
            else:
                if late[a]:
                    aux[a] = hint(a)
                wires[3 * g + s] = aux[a]
        wires[3 * g + 2] = wires[3 * g] * wires[3 * g + 1] % L
    bad = 0
    for a in range(desc.n_asserts):
        if lc(desc.lc_off, desc.lc_var, desc.lc_coef, 2 * n + a):
            bad = a + 1
            break
    return aux, wires[0::3], wires[1::3], wires[2::3], bad


def hint_eval_x(desc, v, x: int, pub=None) -> list:
    return witness(desc, v, x, pub)[0]


def staged_lds(desc) -> int:
    """circuit::witness_program_staged_lds restated for a wire-hinted circuit:
    the fail word (32 B), the 3n wires, the m_in + n_pub inputs (32 B each) and
    the device image -- side_aux [2n], lc_off [2n + A + 1], lc_wire [2n + A],
    level_off [levels + 1], level_gate [n], with late hints a record of 3 words
    per side, then the T + T_late flagged ids padded to a multiple of 8 words and
    as many coefficients of 8 words.  T_late: the terms of each late hint that
    feeds a side, once.  Levels count the gates a side's late hint reads."""
    h, m_in, n, A = desc.hints, desc.m_in, desc.n_gates, desc.n_asserts
    wbase = 2 + m_in + getattr(desc, "n_pub", 0)
    late = [is_late(desc, t) for t in range(desc.n_aux)]
    level, fed = [0] * n, set()
    for g in range(n):
        for s in range(2):
            a = desc.side_aux[2 * g + s]
            if a == SIDE_LC:
                ids = desc.lc_var[desc.lc_off[2 * g + s]:desc.lc_off[2 * g + s + 1]]
            elif late[a]:
                ids = h.lc_var[h.lc_off[a]:h.lc_off[a + 1]]
                fed.add(a)
            else:
                ids = []
            for var in ids:
                if var >= wbase:
                    level[g] = max(level[g], level[(var - wbase) // 3] + 1)
    T = desc.lc_off[2 * n + A] + sum(h.lc_off[a + 1] - h.lc_off[a] for a in fed)
    words = 2 * n + (2 * n + A + 1) + (2 * n + A) + (max(level) + 2) + n + (6 * n if any(late) else 0) + T
    words = (words + 7) // 8 * 8 + 8 * T
    return 32 + 96 * n + 32 * (m_in + getattr(desc, "n_pub", 0)) + 4 * words


# ------------------------------------------------------- hand-built programs

@dataclass
class Hints:
    op: list = field(default_factory=list)
    lc_off: list = field(default_factory=lambda: [0])
    lc_var: list = field(default_factory=list)
    lc_coef: list = field(default_factory=list)
    wire: bool = True  # (the binding's switch: bpp_circuit_create_wire_hinted)


@dataclass
class Desc:
    m_in: int
    n_pub: int
    n_gates: int = 0
    n_aux: int = 0
    n_asserts: int = 0
    side_aux: list = field(default_factory=list)
    lc_off: list = field(default_factory=lambda: [0])
    lc_var: list = field(default_factory=list)
    lc_coef: list = field(default_factory=list)
    hints: Hints = field(default_factory=Hints)

    # ids
    def v(self, j):
        return 1 + j

    @property
    def x(self):
        return 1 + self.m_in

    def u(self, i):
        return 2 + self.m_in + i

    def w(self, h, lro):
        return 2 + self.m_in + self.n_pub + 3 * h + lro

    def _emit(self, terms):
        for var, coef in terms:
            self.lc_var.append(var)
            self.lc_coef.append((coef % L).to_bytes(32, "little"))
        self.lc_off.append(len(self.lc_var))

    def hint(self, op, arg, terms) -> int:
        """A new aux value with its hint; terms: [(id, coefficient int)], ids ascending."""
        h = self.hints
        h.op.append(op | arg << 8)
        for var, coef in terms:
            h.lc_var.append(var)
            h.lc_coef.append((coef % L).to_bytes(32, "little"))
        h.lc_off.append(len(h.lc_var))
        self.n_aux += 1
        return self.n_aux - 1

    def gate(self, left, right) -> int:
        """A side is a list of terms (defined) or an aux index (free)."""
        assert self.n_asserts == 0, "gates before asserts"
        for side in (left, right):
            if isinstance(side, int):
                self.side_aux.append(side)
                self.lc_off.append(len(self.lc_var))
            else:
                self.side_aux.append(SIDE_LC)
                self._emit(side)
        self.n_gates += 1
        return self.n_gates - 1

    def assert_zero(self, terms):
        self._emit(terms)
        self.n_asserts += 1


def sb(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


def rnd(tag: bytes) -> int:
    import hashlib
    return int.from_bytes(hashlib.sha512(tag).digest(), "little") % L


# inputs of the hand-built programs: v_0..v_4 the designed values, v_5 and v_7
# random, v_6 = 2; three public inputs
V_ROW = [0, 1, L - 1, 2**252, 2**252 - 1, rnd(b"wh-v5"), 2, rnd(b"wh-v7")]
U_ROW = [rnd(b"wh-u0"), L - 1, 0]
BIT_ARGS = (0, 31, 32, 63, 64, 252)
C1, C2 = rnd(b"wh-c1"), rnd(b"wh-c2")


def kernel_program(n: int, chain: bool) -> Desc:
    """n gates over 8 inputs and 3 public inputs, every right side free.  Gates
    0..7 carry the inputs (l_g = v_g) and take hints over x alone.  Gate g >= 8:
    l_g = (g + 1) + v_{g mod 8} + o_prev, where prev = g - 1 in a chain (one gate
    a level) and a carrier otherwise (one wide level); its hint cycles through
    every op over carrier wires (the designed values, every bit arg in turn),
    over x, over the previous gate's wires, over everything at once, and an early
    hint; every 16th gate takes the previous gate's aux value on its LEFT side
    too (an aux index feeding two sides).  Three asserts: one that holds, one
    over x and the last wires, one that holds."""
    d = Desc(len(V_ROW), len(U_ROW))
    for g in range(n):
        prev = g - 1 if chain or g < 8 else g % 8
        j = (g // 9) % 8  # the carrier whose wire the hint reads
        arg = BIT_ARGS[(g // 9) % 6] if g % 2 else BIT_ARGS[(g // 9 + g // 54) % 6]
        if g < 8:
            kinds = [(INV, 0, [(d.v(1), L - 1), (d.x, 1)]), (BIT, 252, [(d.x, 1)]), (NOT_BIT, 31, [(d.x, C1)]),
                     (IS_ZERO, 0, [(d.v(g), 1), (d.x, L - 1)]), (VALUE, 0, [(0, C2), (d.x, 1), (d.u(0), C1)]),
                     (BIT, 3, [(d.v(5), 1)])]
            t = d.hint(*kinds[g % 6])
            d.gate([(d.v(g), 1)], t)
            continue
        kinds = [(INV, 0, [(d.v(1), L - 1), (d.x, 1)]),
                 (BIT, arg, [(d.w(j, 0), 1)]),
                 (NOT_BIT, arg, [(d.w(j, 0), 1)]),
                 (IS_ZERO, 0, [(d.w((0, 1, 6, 2, 5)[(g // 9) % 5], 0), 1)]),
                 (INV, 0, [(d.w((0, 1, 6, 2, 5)[(g // 9) % 5], 0), 1)]),
                 (VALUE, 0, [(0, C1), (d.v(g % 8), 1), (d.x, C2), (d.u(0), 1), (d.w(prev, 2), L - 1)]),
                 (BIT, g % 64, [(d.v(5), 1), (d.u(1), C1)]),                   # early
                 (IS_ZERO, 0, [(d.w(prev, 0), 1), (d.w(prev, 1), L - 1)]),
                 (INV, 0, [(d.w(prev, 2), 1)])]                                # the hint of gate g reads o_{g-1}
        t = d.hint(*kinds[g % 9])
        if g % 16 == 9:
            d.gate(t - 1, t)  # the previous gate's aux value again: a second side it feeds
        else:
            d.gate([(0, g + 1), (d.v(g % 8), 1), (d.w(prev, 2), 1)], t)
    d.assert_zero([(d.v(0), L - 1), (d.w(0, 0), 1)])
    d.assert_zero([(d.x, 1), (d.w(n - 1, 1), 1), (d.w(n - 1, 2), C1)])
    d.assert_zero([(0, 1), (d.v(1), L - 1)])
    return d


def bits_program() -> Desc:
    """The designed values 0, 1, l - 1, 2^252, 2^252 - 1 (and a random one) as
    wires -- l_j = v_j, and o_j = v_j x over x -- with BIT and NOT_BIT of every
    arg 0, 31, 32, 63, 64, 252 over each l_j, and INV and IS_ZERO over each l_j
    and over l_j - v_j (a zero made of a wire)."""
    d = Desc(len(V_ROW), len(U_ROW))
    for j in range(6):
        d.gate([(d.v(j), 1)], [(d.x, 1)])
    for j in range(6):
        for arg in BIT_ARGS:
            l = d.hint(BIT, arg, [(d.w(j, 0), 1)])
            d.gate(l, d.hint(NOT_BIT, arg, [(d.w(j, 0), 1)]))
    for j in range(6):
        d.gate(d.hint(INV, 0, [(d.w(j, 0), 1)]), d.hint(IS_ZERO, 0, [(d.w(j, 0), 1)]))
        d.gate(d.hint(INV, 0, [(d.v(j), L - 1), (d.w(j, 0), 1)]), d.hint(IS_ZERO, 0, [(d.v(j), L - 1), (d.w(j, 0), 1)]))
    d.assert_zero([(d.v(0), L - 1), (d.w(0, 0), 1)])
    return d


def x_program() -> Desc:
    """Every op over x alone and over x with inputs: 12 gates, no wire read."""
    d = Desc(len(V_ROW), len(U_ROW))
    for arg in BIT_ARGS:
        d.gate(d.hint(BIT, arg, [(d.x, 1)]), d.hint(NOT_BIT, arg, [(d.x, 1)]))
    d.gate(d.hint(INV, 0, [(d.x, 1)]), d.hint(IS_ZERO, 0, [(d.x, 1)]))
    d.gate(d.hint(INV, 0, [(d.v(5), L - 1), (d.x, 1)]), d.hint(IS_ZERO, 0, [(d.v(5), L - 1), (d.x, 1)]))  # 0 when x = v_5
    d.gate(d.hint(VALUE, 0, [(d.x, 1)]), d.hint(VALUE, 0, [(d.x, L - 1)]))
    d.gate(d.hint(VALUE, 0, [(d.x, C1)]), d.hint(VALUE, 0, [(0, 1), (d.v(2), C2), (d.x, 1), (d.u(1), L - 1)]))
    d.gate([(d.x, 1)], d.hint(VALUE, 0, []))
    d.gate([(d.v(0), 1)], d.hint(INV, 0, []))
    d.assert_zero([(d.x, L - 1), (d.w(8, 0), 1)])
    return d


def rows(P: int):
    """Proof p's inputs: the designed values rotated by p."""
    vs = [[V_ROW[(j + p) % 7] for j in range(7)] + [V_ROW[7] + p] for p in range(P)]
    us = [[U_ROW[(i + p) % len(U_ROW)] for i in range(len(U_ROW))] for p in range(P)]
    return vs, us
