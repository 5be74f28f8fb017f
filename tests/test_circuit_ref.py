"""Caller-defined circuits without a GPU: the reference helper
(tests/circuit_ref.py) against the oracle -- the two-half program compiles to
bp.perm_circuit, every gadget's witness satisfies its compiled rows, one wrong
input violates exactly the expected assert row, and the helper's own proofs
verify and are rejected under a changed coefficient or label."""
import copy
import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_ref as cr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402

L = bp.L
GOLDEN = Path(__file__).resolve().parent / "golden" / "circuit.json"
CASES = ["member2", "member13", "twohalf2", "twohalf3", "range3", "range6", "multiset4", "heavy", "wide70"]


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8, 9, 52])
def test_two_half_program_is_the_perm_circuit(k):
    got, want = cr.compile_program(gd.two_half_shuffle(k)), bp.perm_circuit(k)
    assert (got.n, got.n_p, got.Q, got.m) == (want.n, want.n_p, want.Q, want.m)
    for w in ("WL", "WR", "WO", "WV"):
        assert sorted(getattr(got, w)) == sorted(getattr(want, w)), w
    assert got.c == want.c


def test_sizes():
    d = gd.in_range(3)
    C = cr.compile_program(d)
    assert (d.m_in, d.n_gates, d.n_aux, d.n_asserts) == (1, 3, 6, 7)
    assert (C.Q, C.m, C.n_p) == (0 + 7 + 1, 2, 4)  # no defined side
    d = gd.member_of([3, 7])
    C = cr.compile_program(d)
    assert (d.n_gates, C.Q, C.n_p) == (1, 2 + 1 + 1, 4)
    assert cr.compile_program(gd.member_of(list(range(13)))).n == 12
    assert cr.compile_program(gd.same_multiset(5)).n == 8
    assert cr.compile_program(cr.heavy_circuit()).n_p == 16
    assert cr.compile_program(cr.chain_circuit(300)).n_p == 512
    assert cr.proof_len(cr.chain_circuit(300)) == 32 * (13 + 18)


@pytest.mark.parametrize("name", CASES)
def test_witness_satisfies_every_row(name):
    for i in range(3):
        desc, v, aux = cr.satisfying(name, i)
        C = cr.compile_program(desc)
        x = cr.rand_scalar(b"x-%s-%d" % (name.encode(), i))
        aL, aR, aO, bad = cr.eval_program(desc, v, aux, x)
        assert bad == 0
        assert bp.check_constraints(C, [a % L for a in v] + [x], aL, aR, aO, x) == []


def _assert_row(desc, a):
    """The compiled row of assert a."""
    return sum(1 for s in desc.side_aux if s == cr.SIDE_LC) + a


@pytest.mark.parametrize("name,wrong,assert_index", [
    ("member2", lambda v, aux: ([(v[0] + 1) % L], aux), 0),
    ("member13", lambda v, aux: ([(v[0] + 1) % L], aux), 0),
    ("twohalf3", lambda v, aux: (v[:-1] + [(v[-1] + 1) % L], aux), 0),
    ("multiset4", lambda v, aux: (v[:-1] + [(v[-1] + 1) % L], aux), 0),
    ("range3", lambda v, aux: ([8], aux), 6),                       # 8 >= 2^3: the bit sum
    ("range3", lambda v, aux: (v, aux[:3] + [aux[3] ^ 1] + aux[4:]), None),  # see the test
    ("wide70", lambda v, aux: (v[:40] + [(v[40] + 1) % L] + v[41:], aux), None),
])
def test_one_wrong_input_violates_the_expected_row(name, wrong, assert_index):
    desc, v, aux = cr.satisfying(name, 0)
    C = cr.compile_program(desc)
    x = cr.rand_scalar(b"xw-" + name.encode())
    v2, aux2 = wrong(list(v), list(aux))
    aL, aR, aO, bad = cr.eval_program(desc, v2, aux2, x)
    rows = bp.check_constraints(C, [a % L for a in v2] + [x], aL, aR, aO, x)
    if name == "range3" and assert_index is None:
        # bit 1's right side flipped: v = 7 has bit 1 set, r = 1 makes o_1 = 1
        # (assert 2) and l + r = 2 (assert 3)
        assert rows == [_assert_row(desc, 2), _assert_row(desc, 3)] and bad == 3
    elif name == "wide70":
        # v_40 bumped: v_40 - v_39 - 1 (assert 37) and v_41 - v_40 - 1 (assert 38)
        assert rows == [_assert_row(desc, 37), _assert_row(desc, 38)] and bad == 38
    else:
        assert rows == [_assert_row(desc, assert_index)] and bad == assert_index + 1


def with_coef(desc, t, delta=2):
    d = copy.copy(desc)
    d.lc_coef = list(desc.lc_coef)
    d.lc_coef[t] = cr.sb(int.from_bytes(desc.lc_coef[t], "little") + delta)
    return d


@pytest.mark.parametrize("name", ["member2", "twohalf2", "range3"])
def test_prove_verify_and_reject(name):
    desc, v, aux = cr.satisfying(name, 1)
    gam = [cr.rand_scalar(b"g-%s-%d" % (name.encode(), j)) for j in range(desc.m_in)]
    pf = cr.prove_circuit(desc, v, aux, cr.seed32(name.encode()), gam)
    assert len(pf.V) == desc.m_in + 1 and len(pf.to_bytes()) == cr.proof_len(desc)
    assert cr.verify_circuit(desc, pf)
    assert not cr.verify_circuit(desc, pf, label=b"another")
    other = with_coef(desc, len(desc.lc_coef) - 1)
    assert cr.circuit_digest(other) != cr.circuit_digest(desc)
    assert not cr.verify_circuit(other, pf)
    # an unsatisfied witness proves to something the verifier rejects
    bad_v = [(v[0] + 2) % L] + list(v[1:])
    bad_aux = desc.aux_of([0]) if name == "range3" else aux
    assert not cr.verify_circuit(desc, cr.prove_circuit(desc, bad_v, bad_aux, cr.seed32(b"bad"), check=False))


def test_two_half_program_and_perm_proofs_do_not_cross():
    """The program restating the two-half circuit has the same matrices but its
    own transcript prefix: neither verifier accepts the other's proof."""
    k = 2
    pf, _perm = bp.ac_prove(k, 7)
    desc = gd.two_half_shuffle(k)
    assert bp.ac_verify(k, pf) and not cr.verify_circuit(desc, pf)
    _, v, _ = cr.satisfying("twohalf2", 0)
    pc = cr.prove_circuit(desc, v, [], cr.seed32(b"cross"))
    assert cr.verify_circuit(desc, pc) and not bp.ac_verify(k, pc)


def golden_cases():
    return json.loads(GOLDEN.read_text())["cases"]


def test_helper_reproduces_the_golden_file():
    cases = golden_cases()
    assert len(cases) == 4
    for case in cases:
        desc, _, _ = cr.satisfying(case["name"], 0)
        assert cr.circuit_digest(desc).hex() == case["digest"]
        for p in range(len(case["v"])):
            v = [int.from_bytes(bytes.fromhex(h), "little") for h in case["v"][p]]
            aux = [int.from_bytes(bytes.fromhex(h), "little") for h in case["aux"][p]]
            gam = [int.from_bytes(bytes.fromhex(h), "little") for h in case["gammas"][p]] if case["gammas"] else None
            pf = cr.prove_circuit(desc, v, aux, bytes.fromhex(case["seeds"][p]), gam, label=case["label"].encode())
            assert pf.to_bytes().hex() == case["proofs"][p]
            assert [e.hex() for e in pf.V] == case["V"][p]
