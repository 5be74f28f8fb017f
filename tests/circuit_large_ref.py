"""Reference for large circuits (a helper module, not a test) with no
elliptic-curve arithmetic: prover_scalars replays a proof's transcript from the
proof's own point bytes (Keccak only) and recomputes the three scalars the
prover derives from the witness -- t_hat, tau_x and mu -- with the formulas of
circuit_ref.prove_circuit (eval_program, indexed_scalar, mat_vec_rows, integers
mod l).  Pure-Python prove_circuit spends minutes in its MSMs at n_p >= 1024;
this takes about a second, and is independent of every kernel: a wrong witness
wire, a wrong row power z^(q+1) or a wrong column sum changes t_hat or tau_x.
The host test pins it to prove_circuit on small cases.

The cases the large-circuit tests share are here too (descriptions, satisfied
instances), so both test files prove the same statements.
"""
from __future__ import annotations

import copy
import hashlib

import circuit_pub_ref as cpr
from oracle import bulletproofs as bp, ristretto as r255
from oracle.merlin import indexed_scalar

L = bp.L
sb, rand_scalar, seed32 = cpr.sb, cpr.rand_scalar, cpr.seed32


def proof_fields(proof: bytes):
    """(points A_I A_O S T1 T3 T4 T5 T6, tau_x, mu, t_hat) of a proof's bytes."""
    pts = [proof[32 * i:32 * i + 32] for i in range(8)]
    tau_x, mu, t_hat = (int.from_bytes(proof[32 * i:32 * i + 32], "little") for i in (8, 9, 10))
    return pts, tau_x, mu, t_hat


def prover_scalars(desc, v, aux, seed, gammas, pub, V, proof: bytes, label: bytes = b"bp-perm"):
    """(t_hat, tau_x, mu) an honest prover of (v, aux, pub) with these draws puts
    into a proof whose commitments are V (m x 32 bytes, or a list) and whose
    points are `proof`'s.  v, aux, pub, gammas: ints (gammas None: drawn)."""
    C = cpr.compile_program(desc)
    m_in, n, n_p, m = desc.m_in, C.n, C.n_p, C.m
    pub = [u % L for u in (pub or [])]
    Vb = V if isinstance(V, (bytes, bytearray)) else b"".join(V)
    assert len(Vb) == 32 * m
    S = [indexed_scalar(seed, j) for j in range(m + 3 + 2 * n_p + 5)]
    gamma = S[:m]
    if gammas is not None:
        gamma[:m_in] = [x % L for x in gammas]
    alpha, beta, rho = S[m], S[m + 1], S[m + 2]
    sL = S[m + 3: m + 3 + n_p]
    sR = S[m + 3 + n_p: m + 3 + 2 * n_p]
    taus = S[m + 3 + 2 * n_p:]
    pts, *_ = proof_fields(proof)

    tr = cpr._transcript(desc, n_p, label, pub)
    for j in range(m_in):
        tr.append_point(b"V", Vb[32 * j:32 * j + 32])
    x_perm = tr.challenge_scalar(b"x_perm")
    tr.append_point(b"V", Vb[32 * m_in:32 * m_in + 32])
    aL, aR, aO, bad = cpr.eval_program(desc, [x % L for x in v], aux or [], pub, x_perm)
    assert not bad, bad
    pad = [0] * (n_p - n)
    aL, aR, aO = aL + pad, aR + pad, aO + pad
    for lab, P in zip((b"A_I", b"A_O", b"S"), pts[:3]):
        tr.append_point(lab, P)
    y = tr.challenge_scalar(b"y")
    z = tr.challenge_scalar(b"z")
    y_n = bp.powers(y, n_p)
    y_inv_n = bp.powers(r255.scalar_inv(y), n_p)
    z_q = bp.powers(z, C.Q + 1)[1:]
    zWL = bp.mat_vec_rows(C.WL, z_q, n_p)
    zWR = bp.mat_vec_rows(C.WR, z_q, n_p)
    zWO = bp.mat_vec_rows(C.WO, z_q, n_p)
    zWV = bp.mat_vec_rows(C.WV, z_q, m)
    l_poly = [[0] * n_p,
              [(aL[i] + y_inv_n[i] * zWR[i]) % L for i in range(n_p)],
              list(aO),
              list(sL)]
    r_poly = [[(zWO[i] - y_n[i]) % L for i in range(n_p)],
              [(y_n[i] * aR[i] + zWL[i]) % L for i in range(n_p)],
              [0] * n_p,
              [y_n[i] * sR[i] % L for i in range(n_p)]]
    for lab, P in zip((b"T1", b"T3", b"T4", b"T5", b"T6"), pts[3:]):
        tr.append_point(lab, P)
    x = tr.challenge_scalar(b"x")
    xp = bp.powers(x, 7)
    tau_x = (sum(tau * xp[i] for tau, i in zip(taus, (1, 3, 4, 5, 6))) + xp[2] * bp.inner(zWV, gamma)) % L
    mu = (alpha * x + beta * xp[2] + rho * xp[3]) % L
    t_hat = bp.inner(bp._vecpoly_eval(l_poly, x), bp._vecpoly_eval(r_poly, x))
    return t_hat, tau_x, mu


# ------------------------------------------------------------------ the cases

def q1508_circuit(extra_asserts: int = 483):
    """512 gates with both sides defined and 483 asserts: Q = 1508, one row past
    the one-table kernels, n = 512 well inside the LDS witness kernel.  Gate g
    is (v_0 + g)(v_1 - x + g); assert a is (a + 2)(v_{2+a} - v_0 - a - 1) = 0
    over an input of its own: a distinct non-unit coefficient on every assert
    row, the rows past 1507 among them."""
    from bpperm.gadgets import CircuitBuilder
    b = CircuitBuilder()
    v = b.inputs(2 + extra_asserts)
    for g in range(512):
        b.mul(v[0] + g, v[1] - b.challenge + g)
    for a in range(extra_asserts):
        b.assert_zero((v[2 + a] - v[0] - (a + 1)) * (a + 2))
    return b.build()


def q1508_instance(i: int):
    a = [rand_scalar(b"q1508-a-%d" % i), 0, L - 1][i % 3]
    bb = [rand_scalar(b"q1508-b-%d" % i), L - 1, 0][i % 3]
    return [a, bb] + [(a + j + 1) % L for j in range(483)]


def seam_circuit(n_asserts: int):
    """300 gates with both sides defined and asserts that bring Q + 1 (the one
    table's length; Q = 601 + n_asserts) to 768 (n_asserts = 166) or 769 (167):
    the split table's hi index steps at e = q + 1 = 256, 512, 768.  Gate g is
    ((g + 2) v_0 + g)((g + 3) v_1 - x): row g (left) and row 300 + g (right)
    carry the distinct non-unit coefficients g + 2 and g + 3, which covers q + 1
    in {255, 256, 257, 511, 512, 513}; assert a (row 600 + a) is (a + 5)(v_{2+a}
    - v_0 - a), covering q + 1 = 767 at 167 asserts.  The last row, q + 1 = 768
    there, is the library's own v_m = x: its W_V entry is 1, its constant the
    proof's -x."""
    from bpperm.gadgets import CircuitBuilder
    b = CircuitBuilder()
    v = b.inputs(2 + n_asserts)
    for g in range(300):
        b.mul(v[0] * (g + 2) + g, v[1] * (g + 3) - b.challenge)
    for a in range(n_asserts):
        b.assert_zero((v[2 + a] - v[0] - a) * (a + 5))
    return b.build()


def seam_instance(n_asserts: int, i: int):
    a = [rand_scalar(b"seam-a-%d" % i), 0, L - 1][i % 3]
    bb = rand_scalar(b"seam-b-%d" % i)
    return [a, bb] + [(a + j) % L for j in range(n_asserts)]


def shuffle_instance(k: int, i: int):
    """(v, pub) of shuffle_of_public(k): proof i's own deck (0 and l - 1 among
    the cards of proof 1) and a permutation of it."""
    deck = [rand_scalar(b"lg-deck-%d-%d" % (i, j)) for j in range(k)]
    if i == 1:
        deck[0], deck[1] = 0, L - 1
    perm = sorted(range(k), key=lambda j: hashlib.sha256(b"lg-perm-%d-%d" % (i, j)).digest())
    return [deck[p] for p in perm], deck


def range_many_instance(desc, count: int, nbits: int, i: int):
    top = (1 << nbits) - 1
    v = [rand_scalar(b"lg-rm-%d-%d" % (i, j)) & top for j in range(count)]
    v[0], v[1] = (0, top) if i % 2 == 0 else (top, 0)
    return v, desc.aux_of(v)


def large_case(name: str, n: int = 3):
    """(desc, vs, auxs, pubs) of n satisfied instances; auxs / pubs are None
    where the circuit has none."""
    from bpperm import gadgets as gd
    import circuit_ref as cr
    if name == "chain683":
        d = cr.chain_circuit(683)
        return d, [[[rand_scalar(b"lg-ch-%d" % i), 0, L - 1][i % 3]] for i in range(n)], None, None
    if name == "q1508":
        return q1508_circuit(), [q1508_instance(i) for i in range(n)], None, None
    if name == "shuffle416":
        d = gd.shuffle_of_public(416)
        got = [shuffle_instance(416, i) for i in range(n)]
        return d, [g[0] for g in got], None, [g[1] for g in got]
    if name.startswith("rangemany"):
        count = int(name[9:])
        d = gd.in_range_many(count, 64)
        got = [range_many_instance(d, count, 64, i) for i in range(n)]
        return d, [g[0] for g in got], [g[1] for g in got], None
    raise KeyError(name)


def changed_coefficient(desc, term: int):
    """desc with coefficient `term` + 2: another statement of the same shape."""
    other = copy.copy(desc)
    other.lc_coef = list(desc.lc_coef)
    other.lc_coef[term] = sb(int.from_bytes(other.lc_coef[term], "little") + 2)
    return other
