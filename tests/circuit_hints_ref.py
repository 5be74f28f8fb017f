"""Plain-Python reference of a circuit's hint program (bpp_circuit_hints), written
from the semantics in include/bpperm.h and from nothing else: it reads the
description's arrays, never a gadget's aux_of.

    aux_t = op_t(w_t),  w_t = sum coef * value over the hint's terms, mod l
    ids: 0 = one, 1 + j = v_j, 2 + m_in + i = u_i
    VALUE w | BIT bit arg of w | NOT_BIT 1 - it | INV w^-1 (0 for 0) | IS_ZERO [w = 0]
"""
from __future__ import annotations

from dataclasses import dataclass, field

L = 2**252 + 27742317777372353535851937790883648493
VALUE, BIT, NOT_BIT, INV, IS_ZERO = 0, 1, 2, 3, 4


def hint_eval(desc, v, pub=None) -> list:
    """desc: anything with m_in, n_aux and hints (op, lc_off, lc_var, lc_coef as
    32-byte little-endian scalars); v: m_in ints; pub: n_pub ints.  -> n_aux ints."""
    h = desc.hints
    pub = list(pub or [])
    out = []
    for t in range(desc.n_aux):
        w = 0
        for e in range(h.lc_off[t], h.lc_off[t + 1]):
            var = h.lc_var[e]
            coef = int.from_bytes(h.lc_coef[e], "little")
            if var == 0:
                val = 1
            elif var <= desc.m_in:
                val = v[var - 1]
            else:
                assert var >= 2 + desc.m_in, "a hint does not read x"
                val = pub[var - 2 - desc.m_in]
            w = (w + coef * val) % L
        op, arg = h.op[t] & 0xFF, h.op[t] >> 8
        if op == VALUE:
            out.append(w)
        elif op == BIT:
            out.append((w >> arg) & 1)
        elif op == NOT_BIT:
            out.append(1 - ((w >> arg) & 1))
        elif op == INV:
            out.append(pow(w, L - 2, L))
        elif op == IS_ZERO:
            out.append(1 if w == 0 else 0)
        else:
            raise ValueError(f"hint {t}: unknown op {op}")
    return out


@dataclass
class Hints:
    op: list = field(default_factory=list)
    lc_off: list = field(default_factory=lambda: [0])
    lc_var: list = field(default_factory=list)
    lc_coef: list = field(default_factory=list)


@dataclass
class Desc:
    """A description for hand-built hint programs: n_aux gates v_0 * aux_t, no
    assert -- the smallest circuit that has the aux values the hints feed."""
    m_in: int
    n_pub: int
    n_aux: int
    hints: Hints
    n_gates: int = 0
    n_asserts: int = 0
    side_aux: list = field(default_factory=list)
    lc_off: list = field(default_factory=list)
    lc_var: list = field(default_factory=list)
    lc_coef: list = field(default_factory=list)


def hand_built(m_in: int, n_pub: int, hints) -> Desc:
    """hints: a list of (op, arg, [(var id, coefficient int), ..]) with ids
    ascending.  Gate t = v_0 (defined) times aux_t (free)."""
    h = Hints()
    for op, arg, terms in hints:
        h.op.append(op | arg << 8)
        for var, coef in terms:
            h.lc_var.append(var)
            h.lc_coef.append((coef % L).to_bytes(32, "little"))
        h.lc_off.append(len(h.lc_var))
    n = len(hints)
    d = Desc(m_in, n_pub, n, h, n_gates=n)
    one = (1).to_bytes(32, "little")
    d.lc_off = [0]
    for t in range(n):
        d.side_aux += [0xFFFFFFFF, t]
        d.lc_var.append(1)
        d.lc_coef.append(one)
        d.lc_off += [len(d.lc_var), len(d.lc_var)]
    return d
