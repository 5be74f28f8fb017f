"""The reference for circuits with public inputs (tests/circuit_pub_ref.py) on
its own, no library: it proves and verifies each gadget at its smallest size,
and a proof is bound to its public inputs -- a changed u_i or another proof's
public inputs reject it."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_pub_ref as cp  # noqa: E402
import circuit_ref as cr  # noqa: E402
from bpperm import gadgets as gd  # noqa: E402

L = cp.L
SMALLEST = ["opens", "memberpub1", "memberpub2", "sum1", "shufflepub2"]


@pytest.fixture(scope="module")
def proved():
    out = {}
    for name in SMALLEST:
        desc, v, aux, pub = cp.satisfying(name, 0)
        out[name] = (desc, pub, cp.prove_circuit(desc, v, aux, pub, cp.seed32(name.encode())))
    return out


@pytest.mark.parametrize("name", SMALLEST)
def test_reference_proves_and_verifies(proved, name):
    desc, pub, proof = proved[name]
    assert desc.n_pub == len(pub) > 0
    assert len(proof.to_bytes()) == cp.proof_len(desc)
    assert cp.verify_circuit(desc, proof, pub)


@pytest.mark.parametrize("name", SMALLEST)
def test_changed_public_input_rejects(proved, name):
    desc, pub, proof = proved[name]
    for i in {0, len(pub) - 1}:
        other = list(pub)
        other[i] = (other[i] + 1) % L
        assert not cp.verify_circuit(desc, proof, other)


def test_swapped_public_inputs_reject():
    """Two proofs of one circuit, each valid under its own public inputs and
    under no other's."""
    name = "memberpub2"
    inst = [cp.satisfying(name, i) for i in range(2)]
    desc = inst[0][0]
    proofs = [cp.prove_circuit(desc, v, aux, pub, cp.seed32(b"swap-%d" % i)) for i, (_, v, aux, pub) in enumerate(inst)]
    pubs = [x[3] for x in inst]
    assert all(cp.verify_circuit(desc, proofs[i], pubs[i]) for i in range(2))
    assert not cp.verify_circuit(desc, proofs[0], pubs[1]) and not cp.verify_circuit(desc, proofs[1], pubs[0])


def test_unsatisfied_public_assert_is_found_and_its_proof_rejected():
    desc, v, aux, pub = cp.satisfying("opens", 0)
    wrong = [(pub[0] + 5) % L]
    assert cp.eval_program(desc, v, aux, pub, 7)[3] == 0
    assert cp.eval_program(desc, v, aux, wrong, 7)[3] == 1
    proof = cp.prove_circuit(desc, v, aux, wrong, cp.seed32(b"unsat"), check=False)
    assert not cp.verify_circuit(desc, proof, wrong) and not cp.verify_circuit(desc, proof, pub)


def test_without_public_inputs_it_is_the_plain_reference():
    """n_pub = 0: the digest, the compiled rows and the proof bytes of
    tests/circuit_ref.py."""
    desc, v, aux = cr.satisfying("member2", 0)
    assert desc.n_pub == 0 and cp.circuit_digest(desc) == cr.circuit_digest(desc)
    a, b = cp.compile_program(desc), cr.compile_program(desc)
    assert (a.WL, a.WR, a.WO, a.WV, a.c, a.WU) == (b.WL, b.WR, b.WO, b.WV, b.c, [])
    seed = cp.seed32(b"plain")
    assert cp.prove_circuit(desc, v, aux, [], seed).to_bytes() == cr.prove_circuit(desc, v, aux, seed).to_bytes()


def test_digest_depends_on_n_pub():
    import copy
    desc = gd.member_of([3, 7])  # (the digest is over the arrays as given)
    d1, d2 = copy.copy(desc), copy.copy(desc)
    d1.n_pub, d2.n_pub = 1, 2
    assert len({cp.circuit_digest(d) for d in (desc, d1, d2)}) == 3


def test_straddle_counts_come_from_the_formula():
    lo, hi = cp.chain_straddle()
    assert hi == lo + 1 and hi <= 256  # (n_p = 256: one generator set serves both)
    assert cp.witness_program_staged_lds(cp.chain_pub_circuit(lo)) <= cp.K_LDS_MAX
    assert cp.witness_program_staged_lds(cp.chain_pub_circuit(hi)) > cp.K_LDS_MAX
