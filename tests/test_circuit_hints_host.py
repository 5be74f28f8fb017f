"""Circuit hints without a GPU: the gadgets' hint programs against their aux_of
and the plain-Python reference (tests/circuit_hints_ref.py), the host witness
over the derived values, the statement left untouched by hints, and every
refusal of bpp_circuit_create_hinted."""
import hashlib
import json
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_hints_ref as hr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402

L = hr.L
X = (0x1234567).to_bytes(32, "little")  # any challenge: no hinted gadget reads x


def sb(x):
    return (x % L).to_bytes(32, "little")


def rnd(tag):
    return int.from_bytes(hashlib.sha512(tag).digest(), "little") % L


def designed(nbits):
    return [0, 1, 2**nbits - 1, L - 1, 2**252, rnd(b"hh-a"), rnd(b"hh-b")]


# (name, description, m_in, nbits of its designed values)
GADGETS = [("in_range(5)", gd.in_range(5), 1, 5), ("in_range(252)", gd.in_range(252), 1, 252),
           ("in_range_many(3, 11)", gd.in_range_many(3, 11), 3, 11), ("not_equal", gd.not_equal(), 2, 6),
           ("distinct(4)", gd.distinct(4), 4, 6), ("less_than(3)", gd.less_than(3), 2, 3),
           ("ascending(3, 4)", gd.ascending(3, 4), 3, 4)]


@pytest.mark.parametrize("name,desc,m_in,nbits", GADGETS, ids=[g[0] for g in GADGETS])
def test_hint_eval_equals_aux_of_and_reference(name, desc, m_in, nbits):
    """Every hinted gadget, over vectors drawn from 0, 1, 2^nbits - 1, l - 1,
    2^252 and random values (each value in every position, and all-equal
    vectors: zero differences, the INV hint's 0): the library's host hints, the
    gadget's aux_of and the reference agree."""
    import bpperm
    assert desc.hints is not None and len(desc.hints.op) == desc.n_aux
    c = bpperm.Circuit(desc)
    assert c.has_hints
    vals = designed(nbits)
    rows = [[vals[(i + j) % len(vals)] for j in range(m_in)] for i in range(len(vals))] + [[a] * m_in for a in vals]
    for v in rows:
        got = [int.from_bytes(a, "little") for a in c.hint_eval([sb(x) for x in v])]
        assert got == [a % L for a in desc.aux_of(v)], (name, v)
        assert got == hr.hint_eval(desc, [x % L for x in v]), (name, v)


# satisfied instances, and unsatisfied ones with the assert that must be named
# (asserts of a range block of nbits bits: 2 per bit, then the bit sum)
SATISFIED = [(gd.in_range(5), [0]), (gd.in_range(5), [31]), (gd.in_range(252), [2**252 - 1]),
             (gd.in_range_many(3, 11), [0, 2047, 1000]), (gd.not_equal(), [5, 9]), (gd.not_equal(), [0, L - 1]),
             (gd.distinct(4), [1, 2, 3, L - 1]), (gd.less_than(3), [0, 7]), (gd.less_than(3), [6, 7]),
             (gd.ascending(3, 4), [0, 1, 15]), (gd.ascending(3, 4), [3, 9, 10])]
UNSATISFIED = [(gd.in_range(5), [32], 10), (gd.in_range(5), [L - 1], 10), (gd.not_equal(), [7, 7], 0),
               (gd.not_equal(), [0, 0], 0), (gd.distinct(4), [1, 2, 3, 2], 4),  # pairs 01 02 03 12 13 23
               (gd.less_than(3), [5, 5], 2 * 7 + 6), (gd.less_than(3), [6, 2], 2 * 7 + 6),
               (gd.less_than(3), [8, 9], 6),  # v_0 itself out of range
               (gd.ascending(3, 4), [1, 9, 4], 4 * 9 + 8), (gd.ascending(3, 4), [9, 9, 10], 3 * 9 + 8)]


def test_host_witness_over_derived_aux():
    """Circuit.eval over hint_eval's values: no failing assert for a satisfied
    instance; for equal cards, a repeated card, a descending or out-of-range
    hand, the expected assert."""
    import bpperm
    for desc, v in SATISFIED:
        c = bpperm.Circuit(desc)
        vb = [sb(x) for x in v]
        assert c.eval(vb, c.hint_eval(vb), X)[3] == 0, v
    for desc, v, a in UNSATISFIED:
        c = bpperm.Circuit(desc)
        vb = [sb(x) for x in v]
        assert c.eval(vb, c.hint_eval(vb), X)[3] == a + 1, v


def test_gate_counts():
    assert gd.not_equal().n_gates == 1 and gd.not_equal().n_aux == 1
    assert gd.distinct(5).n_gates == 10
    assert gd.less_than(6).n_gates == 18
    assert gd.ascending(5, 6).n_gates == 9 * 6


def test_builder_hints():
    """hint() on either side of mul(), mixed with a defined side; build() emits
    hints only when every aux value has one; free_mul() without hints keeps
    working; a hint over x or a wire is refused."""
    import bpperm
    b = gd.CircuitBuilder()
    v, u = b.input(), b.public()
    l, r, o = b.mul(b.hint(gd.HINT_VALUE, 3 * v - u + 5), v)   # free left, defined right
    b.mul(u, b.hint(gd.HINT_IS_ZERO, v - u))                    # defined left, free right
    b.assert_zero(l - 3 * v + u - 5)
    desc = b.build()
    assert desc.hints is not None and desc.side_aux == [0, gd.SIDE_LC, gd.SIDE_LC, 1]
    c = bpperm.Circuit(desc)
    got = c.hint_eval([sb(7)], [sb(7)])
    assert got == [sb(3 * 7 - 7 + 5), sb(1)] and got == [sb(a) for a in hr.hint_eval(desc, [7], [7])]
    assert c.eval([sb(7)], got, X, pub=[sb(7)])[3] == 0
    with pytest.raises(ValueError):
        b.hint(gd.HINT_VALUE, b.challenge)
    with pytest.raises(ValueError):
        b.hint(gd.HINT_VALUE, o)
    with pytest.raises(ValueError):
        b.hint(gd.HINT_INV, v, 3)
    with pytest.raises(ValueError):
        b.hint(gd.HINT_BIT, v, 253)
    b.free_mul()  # two aux values without a hint: the whole description has none
    d2 = b.build()
    assert d2.hints is None and d2.n_aux == 4
    c2 = bpperm.Circuit(d2)
    assert not c2.has_hints
    with pytest.raises(bpperm.BppError) as e:
        c2.hint_eval([sb(7)], [sb(7)])
    assert e.value.code == 1
    assert gd.two_half_shuffle(3).hints is None and gd.member_of([1, 2]).hints is None


@pytest.mark.parametrize("name,desc,m_in,nbits", GADGETS, ids=[g[0] for g in GADGETS])
def test_hints_are_no_part_of_the_statement(name, desc, m_in, nbits):
    import bpperm
    a, b = bpperm.Circuit(desc), bpperm.Circuit(desc, hints=False)
    assert a.has_hints and not b.has_hints
    assert (a.n_p, a.Q, a.m, a.digest, a.proof_len) == (b.n_p, b.Q, b.m, b.digest, b.proof_len)
    for which in range(6):
        assert a.matrix(which) == b.matrix(which)


def test_in_range_digest_is_the_golden_one():
    """in_range's description arrays did not change when it gained hints."""
    import bpperm
    gold = {c["name"]: c for c in json.loads((HERE / "golden" / "circuit.json").read_text())["cases"]}
    assert bpperm.Circuit(gd.in_range(3)).digest.hex() == gold["range3"]["digest"]


def _one_hint(op_word, var, coef, m_in=2, n_pub=1, lc_off=None):
    d = hr.hand_built(m_in, n_pub, [(hr.VALUE, 0, [(1, 1)]), (hr.VALUE, 0, [(1, 1)])])
    h = d.hints
    h.op[1] = op_word
    h.lc_var[1:] = list(var)
    h.lc_coef[1:] = [c if isinstance(c, bytes) else sb(c) for c in coef]
    h.lc_off = lc_off or [0, 1, 1 + len(var)]
    return d


ARG, NONCANONICAL = 1, 4
REFUSED = [
    ("unknown op", _one_hint(5, [1], [1]), ARG),
    ("unknown op byte", _one_hint(0xFF, [1], [1]), ARG),
    ("arg above 252", _one_hint(hr.BIT | 253 << 8, [1], [1]), ARG),
    ("arg above 252, NOT_BIT", _one_hint(hr.NOT_BIT | 0xFFFFFF << 8, [1], [1]), ARG),
    ("arg on VALUE", _one_hint(hr.VALUE | 1 << 8, [1], [1]), ARG),
    ("arg on INV", _one_hint(hr.INV | 7 << 8, [1], [1]), ARG),
    ("arg on IS_ZERO", _one_hint(hr.IS_ZERO | 252 << 8, [1], [1]), ARG),
    ("id out of range", _one_hint(hr.VALUE, [1 << 20], [1]), ARG),
    ("id names x", _one_hint(hr.VALUE, [3], [1]), ARG),          # m_in = 2: x is id 3
    ("id names a wire", _one_hint(hr.VALUE, [5], [1]), ARG),     # n_pub = 1: u_0 is 4, l_0 is 5
    ("id names a later wire", _one_hint(hr.VALUE, [10], [1]), ARG),
    ("unsorted ids", _one_hint(hr.VALUE, [2, 1], [1, 1]), ARG),
    ("duplicate ids", _one_hint(hr.VALUE, [2, 2], [1, 1]), ARG),
    ("zero coefficient", _one_hint(hr.VALUE, [1], [0]), ARG),
    ("non-monotone lc_off", _one_hint(hr.VALUE, [1], [1], lc_off=[0, 2, 1]), ARG),
    ("lc_off[0] not 0", _one_hint(hr.VALUE, [1], [1], lc_off=[1, 1, 2]), ARG),
    ("coefficient = l", _one_hint(hr.VALUE, [1], [L.to_bytes(32, "little")]), NONCANONICAL),
    ("coefficient = 2^256 - 1", _one_hint(hr.VALUE, [1], [b"\xff" * 32]), NONCANONICAL),
]


@pytest.mark.parametrize("what,desc,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_hinted_refusals(what, desc, code):
    import bpperm
    with pytest.raises(bpperm.BppError) as e:
        bpperm.Circuit(desc)
    assert e.value.code == code, what
    assert not bpperm.Circuit(desc, hints=False).has_hints  # the description itself is fine


def test_accepted_edges_and_hint_count():
    """The largest arg, u_i and the constant as variables, the empty combination
    and an empty program are accepted; a hint count different from n_aux is
    refused (by the binding: the C struct's arrays are n_aux long by contract)."""
    import bpperm
    d = hr.hand_built(2, 1, [(hr.BIT, 252, [(0, 5), (2, L - 1), (4, 3)]), (hr.INV, 0, []), (hr.NOT_BIT, 0, [])])
    c = bpperm.Circuit(d)
    got = [int.from_bytes(a, "little") for a in c.hint_eval([sb(1), sb(9)], [sb(2**252)])]
    assert got == hr.hint_eval(d, [1, 9], [2**252]) == [((5 - 9 + 3 * 2**252) % L) >> 252, 0, 1]
    for bad in ("short", "long"):
        d = hr.hand_built(2, 1, [(hr.VALUE, 0, [(1, 1)]), (hr.VALUE, 0, [(2, 1)])])
        if bad == "short":
            d.hints.op.pop()
            d.hints.lc_off.pop()
        else:
            d.hints.op.append(hr.VALUE)
            d.hints.lc_off.append(d.hints.lc_off[-1])
        with pytest.raises(ValueError):
            bpperm.Circuit(d)
    # hints == NULL is bpp_circuit_create_ex; a program for n_aux = 0 is empty
    lib = bpperm._lib.load()
    assert lib.bpp_circuit_has_hints(None) == 0
    assert lib.bpp_circuit_hint_eval(None, None, None, None) == ARG


def test_prove_without_aux_needs_hints():
    """aux == NULL with n_aux > 0 on a circuit without hints stays BPP_ERR_ARG
    (checked before the context: no GPU), and the binding still refuses it."""
    import ctypes

    import bpperm
    plain = bpperm.Circuit(gd.in_range(3), hints=False)
    lib = plain.lib
    vb, pf, V = sb(5), ctypes.create_string_buffer(plain.proof_len), ctypes.create_string_buffer(64)
    assert lib.bpp_circuit_prove_batch(None, None, plain.h, 1, vb, None, None, None, b"x", 1, pf, V) == ARG
    hinted = bpperm.Circuit(gd.in_range(3))
    # with hints the same call passes the argument checks and stops at the null context
    assert lib.bpp_circuit_prove_batch(None, None, hinted.h, 1, vb, None, None, None, b"x", 1, pf, V) == ARG
    nc = L.to_bytes(32, "little")
    assert lib.bpp_circuit_prove_batch(None, None, hinted.h, 1, nc, None, None, None, b"x", 1, pf, V) == NONCANONICAL
    assert lib.bpp_circuit_prove_batch(None, None, plain.h, 1, nc, None, None, None, b"x", 1, pf, V) == ARG
