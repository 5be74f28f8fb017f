"""Reference for caller-defined circuits with per-proof public inputs,
bpp_circuit_*_pub (a helper module, not a test), out of the oracle's own pieces
the way tests/circuit_ref.py is built, whose conventions it keeps.

Public inputs u_0..u_{n_pub-1} are given per proof to prover and verifier and
never committed.  Variable ids: 0 = one, 1 + j = v_j, 1 + m_in = x, 2 + m_in +
i = u_i, 2 + m_in + n_pub + 3h + {0, 1, 2} = l_h, r_h, o_h.

compile_program: circuit_ref's rows, plus the sparse matrix W_U (Q x n_pub,
C.WU): a term a u_i of a defined side at row q -> W_U(q, i) = +a, of an assert
row -> -a (the signs the constant of the same combination takes).  A proof's
constant vector is c + W_U u.

Digest: n_pub = 0: circuit_ref's.  n_pub > 0: SHAKE256("bpperm-pubcircuit" ||
le32 m_in || le32 n_pub || le32 n_gates || le32 n_aux || le32 n_asserts ||
side_aux || lc_off || lc_var || lc_coef)[0..32].

Transcript: Transcript(label), dom-sep("acp v1", n_p), append_message("circuit",
digest), append_message("pub", u_i) for i < n_pub (32 bytes each),
V_0..V_{m_in-1}, challenge x_perm, V_{m_in}, then as circuit_ref.  The prover
never reads c; the verifier reads it in <z^Q, c> alone.
"""
from __future__ import annotations

import hashlib

from circuit_ref import n_p_of, rand_scalar, sb, seed32  # noqa: F401  (re-exported for the tests)
from oracle import bulletproofs as bp, ristretto as r255
from oracle.merlin import Transcript, bulletproof_gens, indexed_scalar, pedersen_gens_default

L = bp.L
SIDE_LC = 0xFFFFFFFF


def proof_len(desc) -> int:
    lg = n_p_of(desc.n_gates).bit_length() - 1
    return 32 * (13 + 2 * lg)


def _terms(desc, i: int):
    return [(desc.lc_var[t], int.from_bytes(desc.lc_coef[t], "little"))
            for t in range(desc.lc_off[i], desc.lc_off[i + 1])]


def circuit_digest(desc) -> bytes:
    n_pub = getattr(desc, "n_pub", 0)
    if n_pub:
        h = hashlib.shake_256(b"bpperm-pubcircuit")
        head = (desc.m_in, n_pub, desc.n_gates, desc.n_aux, desc.n_asserts)
    else:
        h = hashlib.shake_256(b"bpperm-circuit")
        head = (desc.m_in, desc.n_gates, desc.n_aux, desc.n_asserts)
    for x in head:
        h.update(x.to_bytes(4, "little"))
    for arr in (desc.side_aux, desc.lc_off, desc.lc_var):
        for x in arr:
            h.update(x.to_bytes(4, "little"))
    for c in desc.lc_coef:
        h.update(c)
    return h.digest(32)


def compile_program(desc) -> bp.Circuit:
    """bp.Circuit with one more attribute, WU: the (q, i, val) triplets of W_U."""
    m_in, n, A, n_pub = desc.m_in, desc.n_gates, desc.n_asserts, getattr(desc, "n_pub", 0)
    wbase = 2 + m_in + n_pub
    defined = sum(1 for a in desc.side_aux if a == SIDE_LC)
    Q = defined + A + 1
    C = bp.Circuit(0, n, n_p_of(n), Q, m_in + 1)
    C.c = [0] * Q
    C.WU = []
    W = (C.WL, C.WR, C.WO)

    def emit(q, i, sign):  # sign = +1: a definition's row; -1: an assert's
        for var, a in _terms(desc, i):
            if var == 0:
                C.c[q] = (sign * a) % L
            elif var <= 1 + m_in:
                C.WV.append((q, var - 1, (sign * a) % L))
            elif var < wbase:
                C.WU.append((q, var - 2 - m_in, (sign * a) % L))
            else:
                w = var - wbase
                W[w % 3].append((q, w // 3, (-sign * a) % L))

    q = 0
    for s in range(2):
        for g in range(n):
            if desc.side_aux[2 * g + s] == SIDE_LC:
                W[s].append((q, g, 1))
                emit(q, 2 * g + s, 1)
                q += 1
    for a in range(A):
        emit(q, 2 * n + a, -1)
        q += 1
    C.WV.append((q, m_in, 1))
    assert q == Q - 1
    return C


def constants(C, pub, x_perm: int):
    """The proof's constant vector c + W_U u, with c[Q-1] = -x_perm."""
    c = list(C.c)
    for q, i, val in C.WU:
        c[q] = (c[q] + val * pub[i]) % L
    c[C.Q - 1] = (-x_perm) % L
    return c


def eval_program(desc, v, aux, pub, x: int):
    """(a_L, a_R, a_O) of the n gates, and 1 + the first assert that does not
    hold (0: all hold)."""
    m_in, n, n_pub = desc.m_in, desc.n_gates, getattr(desc, "n_pub", 0)
    wbase = 2 + m_in + n_pub
    w = [[0] * n, [0] * n, [0] * n]

    def lc(i):
        acc = 0
        for var, a in _terms(desc, i):
            if var == 0:
                val = 1
            elif var <= m_in:
                val = v[var - 1]
            elif var == 1 + m_in:
                val = x
            elif var < wbase:
                val = pub[var - 2 - m_in]
            else:
                val = w[(var - wbase) % 3][(var - wbase) // 3]
            acc = (acc + a * val) % L
        return acc

    for g in range(n):
        for s in range(2):
            a = desc.side_aux[2 * g + s]
            w[s][g] = lc(2 * g + s) if a == SIDE_LC else aux[a] % L
        w[2][g] = w[0][g] * w[1][g] % L
    bad = 0
    for a in range(desc.n_asserts):
        if lc(2 * n + a):
            bad = a + 1
            break
    return w[0], w[1], w[2], bad


def check_constraints(C, v, aL, aR, aO, pub, x):
    """Rows of W_L a_L + W_R a_R + W_O a_O = W_V v + c + W_U u that do not hold."""
    lhs = [0] * C.Q
    rhs = constants(C, pub, x)
    for W, a in ((C.WL, aL), (C.WR, aR), (C.WO, aO)):
        for q, col, val in W:
            lhs[q] = (lhs[q] + val * a[col]) % L
    for q, col, val in C.WV:
        rhs[q] = (rhs[q] + val * v[col]) % L
    return [q for q in range(C.Q) if lhs[q] != rhs[q]]


def _transcript(desc, n_p: int, label: bytes, pub) -> Transcript:
    tr = Transcript(label)
    tr.arithmetic_domain_sep(n_p)
    tr.append_message(b"circuit", circuit_digest(desc))
    assert len(pub) == getattr(desc, "n_pub", 0)
    for u in pub:
        tr.append_message(b"pub", sb(u))
    return tr


def prove_circuit(desc, v, aux, pub, seed, gammas=None, gens=None, label: bytes = b"bp-perm",
                  check: bool = True) -> bp.PermProof:
    """circuit_ref.prove_circuit with pub: n_pub ints.  (The prover never reads
    the constant vector: pub enters through the transcript and the witness.)"""
    C = compile_program(desc)
    m_in, n, n_p, m = desc.m_in, C.n, C.n_p, C.m
    pub = [u % L for u in pub]
    assert len(v) == m_in and len(aux or []) == desc.n_aux
    if gens is None:
        gens = bulletproof_gens(n_p)
    G, H = gens[0][:n_p], gens[1][:n_p]
    g, h = pedersen_gens_default()
    S = [indexed_scalar(seed, j) for j in range(m + 3 + 2 * n_p + 5)]
    gamma = S[:m]
    if gammas is not None:
        assert len(gammas) == m_in
        gamma[:m_in] = [x % L for x in gammas]
    alpha, beta, rho = S[m], S[m + 1], S[m + 2]
    sL = S[m + 3: m + 3 + n_p]
    sR = S[m + 3 + n_p: m + 3 + 2 * n_p]
    taus = S[m + 3 + 2 * n_p:]

    tr = _transcript(desc, n_p, label, pub)
    vals = [x % L for x in v]
    V = []
    for j in range(m_in):
        V.append(bp.enc(bp.msm([vals[j], gamma[j]], [g, h])))
        tr.append_point(b"V", V[-1])
    x_perm = tr.challenge_scalar(b"x_perm")
    V.append(bp.enc(bp.msm([x_perm, gamma[m_in]], [g, h])))
    tr.append_point(b"V", V[-1])
    aL, aR, aO, bad = eval_program(desc, vals, aux or [], pub, x_perm)
    if check:
        assert not bad and not check_constraints(C, vals + [x_perm], aL, aR, aO, pub, x_perm)
    pad = [0] * (n_p - n)
    aL, aR, aO = aL + pad, aR + pad, aO + pad

    A_I = bp.enc(bp.msm([alpha] + aL + aR, [h] + G + H))
    A_O = bp.enc(bp.msm([beta] + aO, [h] + G))
    S_ = bp.enc(bp.msm([rho] + sL + sR, [h] + G + H))
    for lab, P in ((b"A_I", A_I), (b"A_O", A_O), (b"S", S_)):
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
    t = [0] * 7
    for i in range(4):
        for j in range(4):
            t[i + j] = (t[i + j] + bp.inner(l_poly[i], r_poly[j])) % L
    T = []
    for lab, idx, tau in zip((b"T1", b"T3", b"T4", b"T5", b"T6"), (1, 3, 4, 5, 6), taus):
        T.append(bp.enc(bp.msm([t[idx], tau], [g, h])))
        tr.append_point(lab, T[-1])
    x = tr.challenge_scalar(b"x")
    xp = bp.powers(x, 7)
    tau_x = (sum(tau * xp[i] for tau, i in zip(taus, (1, 3, 4, 5, 6))) + xp[2] * bp.inner(zWV, gamma)) % L
    mu = (alpha * x + beta * xp[2] + rho * xp[3]) % L
    l = bp._vecpoly_eval(l_poly, x)
    r = bp._vecpoly_eval(r_poly, x)
    t_hat = bp.inner(l, r)
    tr.append_scalar(b"TX", tau_x)
    tr.append_scalar(b"mu", mu)
    tr.append_scalar(b"t", t_hat)
    w = tr.challenge_scalar(b"w")
    Qp = r255.ed_mul(w, g)
    ipa = bp.ipa_create(tr, Qp, [1] * n_p, y_inv_n, G, H, l, r)
    return bp.PermProof(V, A_I, A_O, S_, T, tau_x, mu, t_hat, ipa)


def verify_circuit_msm_terms(desc, proof: bp.PermProof, pub, gens=None, label: bytes = b"bp-perm"):
    """circuit_ref.verify_circuit_msm_terms under the public inputs pub: they are
    absorbed before V_0, and the constant vector is c + W_U pub."""
    C = compile_program(desc)
    m_in, n_p, m = desc.m_in, C.n_p, C.m
    pub = [u % L for u in pub]
    if gens is None:
        gens = bulletproof_gens(n_p)
    G, H = gens[0][:n_p], gens[1][:n_p]
    g, h = pedersen_gens_default()
    if len(proof.V) != m:
        raise ValueError("VerificationError: V count")
    tr = _transcript(desc, n_p, label, pub)
    for j in range(m_in):
        tr.append_point(b"V", proof.V[j])
    x_perm = tr.challenge_scalar(b"x_perm")
    tr.append_point(b"V", proof.V[m_in])
    for lab, P in ((b"A_I", proof.A_I), (b"A_O", proof.A_O), (b"S", proof.S)):
        tr.validate_and_append_point(lab, P)
    y = tr.challenge_scalar(b"y")
    z = tr.challenge_scalar(b"z")
    for lab, P in zip((b"T1", b"T3", b"T4", b"T5", b"T6"), proof.T):
        tr.validate_and_append_point(lab, P)
    x = tr.challenge_scalar(b"x")
    tr.append_scalar(b"TX", proof.tau_x)
    tr.append_scalar(b"mu", proof.mu)
    tr.append_scalar(b"t", proof.t_hat)
    w = tr.challenge_scalar(b"w")
    xp = bp.powers(x, 7)
    y_inv_n = bp.powers(r255.scalar_inv(y), n_p)
    z_q = bp.powers(z, C.Q + 1)[1:]
    zWL = bp.mat_vec_rows(C.WL, z_q, n_p)
    zWR = bp.mat_vec_rows(C.WR, z_q, n_p)
    zWO = bp.mat_vec_rows(C.WO, z_q, n_p)
    zWV = bp.mat_vec_rows(C.WV, z_q, m)
    c = constants(C, pub, x_perm)
    delta = bp.inner([y_inv_n[i] * zWR[i] % L for i in range(n_p)], zWL)
    Vp = [r255.decode(e) for e in proof.V]
    Tp = [r255.decode(e) for e in proof.T]
    t_sc = [(proof.t_hat - xp[2] * (delta + bp.inner(z_q, c))) % L, proof.tau_x]
    t_sc += [(-xp[2] * zWV[j]) % L for j in range(m)]
    t_sc += [(-xp[i]) % L for i in (1, 3, 4, 5, 6)]
    t_pts = [g, h] + Vp + Tp
    Qp = r255.ed_mul(w, g)
    if len(proof.ipa.L) != n_p.bit_length() - 1 or len(proof.ipa.R) != len(proof.ipa.L):
        raise ValueError("VerificationError: IPA rounds")
    ipa_sc, ipa_pts = bp.ipa_verify_msm_terms(proof.ipa, n_p, tr, [1] * n_p, y_inv_n, Qp, G, H)
    Pp_sc = [(-x) % L, (-xp[2]) % L, (-xp[3]) % L, proof.mu, (-proof.t_hat * w) % L]
    Pp_pts = [r255.decode(proof.A_I), r255.decode(proof.A_O), r255.decode(proof.S), h, g]
    Pp_sc += [(-x * y_inv_n[i] * zWR[i]) % L for i in range(n_p)]
    Pp_pts += list(G)
    Pp_sc += [(-(y_inv_n[i] * (x * zWL[i] + zWO[i]) - 1)) % L for i in range(n_p)]
    Pp_pts += list(H)
    return (t_sc, t_pts), (ipa_sc + Pp_sc, ipa_pts + Pp_pts)


def verify_circuit(desc, proof: bp.PermProof, pub, gens=None, label: bytes = b"bp-perm") -> bool:
    try:
        (ts, tp), (is_, ip) = verify_circuit_msm_terms(desc, proof, pub, gens, label)
    except (ValueError, r255.DecodeError):
        return False
    ident = r255.IDENTITY
    return r255.equal(bp.msm(ts, tp), ident) and r255.equal(bp.msm(is_, ip), ident)


# ----------------------------------------------------------- the tests' cases

K_LDS_MAX = 64 * 1024


def witness_program_staged_lds(desc) -> int:
    """circuit::witness_program_staged_lds restated: the fail word (32 B), the
    3n wires, the m_in inputs and n_pub public inputs (32 B each), and the
    program's device image -- side_aux [2n], lc_off [2n + A + 1], lc_wire [2n +
    A], level_off [levels + 1], level_gate [n], T flagged ids padded to a
    multiple of 8 words, then T coefficients of 8 words."""
    m_in, n, A, n_pub = desc.m_in, desc.n_gates, desc.n_asserts, getattr(desc, "n_pub", 0)
    wbase = 2 + m_in + n_pub
    level = [0] * n
    for g in range(n):
        for s in range(2):
            for var, _ in _terms(desc, 2 * g + s):
                if var >= wbase:
                    level[g] = max(level[g], level[(var - wbase) // 3] + 1)
    T = desc.lc_off[2 * n + A]
    words = 2 * n + (2 * n + A + 1) + (2 * n + A) + (max(level) + 2) + n + T
    words = (words + 7) // 8 * 8 + 8 * T
    return 32 + 96 * n + 32 * (m_in + n_pub) + 4 * words


def heavy_pub_circuit():
    """11 gates (n_p = 16) over inputs v_0, v_1, v_2 and ONE public input u_0
    that all 11 right sides and both asserts read -- 13 entries in one column
    of W_U: o_0 = v_0 (v_1 + u_0); gate g = 1..10: ((g + 1) o_0 + g) (v_1 - g -
    x + (g + 1) u_0); asserts o_0 + u_0 - v_2 = 0 and r_0 - v_1 - u_0 = 0."""
    from bpperm.gadgets import CircuitBuilder
    b = CircuitBuilder()
    v0, v1, v2 = b.input(), b.input(), b.input()
    u = b.public()
    _, r0, o0 = b.mul(v0, v1 + u)
    for g in range(1, 11):
        b.mul(o0 * (g + 1) + g, v1 - g - b.challenge + u * (g + 1))
    b.assert_zero(o0 + u - v2)
    b.assert_zero(r0 - v1 - u)
    return b.build()


def wide_pub_circuit(n_pub: int = 300):
    """n_pub = 300 public inputs over one gate (n_p = 4; more entries of W_U
    than the verifier kernel has lanes): an arithmetic progression whose step is
    committed.  o = (v_0 + u_0) v_1; asserts o - v_2 = 0, sum_i (i + 1) u_i -
    v_3 = 0, and u_i - u_{i-1} - v_4 = 0 for i = 1..n_pub - 1."""
    from bpperm.gadgets import LC, CircuitBuilder
    b = CircuitBuilder()
    v = b.inputs(5)
    u = b.publics(n_pub)
    o = b.mul(v[0] + u[0], v[1])[2]
    b.assert_zero(o - v[2])
    total = LC()
    for i, x in enumerate(u):
        total = total + x * (i + 1)
    b.assert_zero(total - v[3])
    for i in range(1, n_pub):
        b.assert_zero(u[i] - u[i - 1] - v[4])
    return b.build()


def chain_pub_circuit(n: int):
    """A public product chain of n gates over one input and n public inputs:
    o_0 = (v - x)(v + u_0), o_g = o_{g-1} (v + u_g); n levels."""
    from bpperm.gadgets import CircuitBuilder
    b = CircuitBuilder()
    v = b.input()
    u = b.publics(n)
    o = b.mul(v - b.challenge, v + u[0])[2]
    for g in range(1, n):
        o = b.mul(o, v + u[g])[2]
    return b.build()


def chain_straddle():
    """(n_lo, n_hi): the last chain_pub_circuit that k_witness_program stages in
    LDS and the first it reads from global memory, from the formula."""
    n = 2
    while witness_program_staged_lds(chain_pub_circuit(n + 1)) <= K_LDS_MAX:
        n += 1
    return n, n + 1


def satisfying(name: str, i: int):
    """(desc, v, aux, pub) of a satisfied instance of the named case; i varies
    it (0 and l - 1 among the values for i = 1, 2 where the case allows)."""
    from bpperm import gadgets as gd
    t = b"%s-%d" % (name.encode(), i)
    rs = lambda tag: rand_scalar(b"pub-" + t + tag)
    if name == "opens":
        a = [rs(b"a"), 0, L - 1][i % 3]
        return gd.opens_to(), [a], [], [a]
    if name.startswith("memberpub"):
        n = int(name[9:])
        s = [rs(b"s%d" % j) for j in range(n)]
        if i % 3 == 1:
            s[0] = 0
        if i % 3 == 2:
            s[-1] = L - 1
        pick = [3 * i + 1, 0, n - 1][i % 3] % n
        return gd.member_of_public(n), [s[pick]], [], s
    if name.startswith("sum"):
        k = int(name[3:])
        v = [rs(b"v%d" % j) for j in range(k)]
        if i % 3 == 1:
            v[0] = L - 1
        return gd.sum_equals(k), v, [], [sum(v) % L]
    if name.startswith("shufflepub"):
        k = int(name[10:])
        deck = [rs(b"d%d" % j) for j in range(k)]
        if i % 3 == 1:
            deck[0], deck[1] = 0, L - 1
        perm = sorted(range(k), key=lambda j: rs(b"p%d" % j))
        return gd.shuffle_of_public(k), [deck[p] for p in perm], [], deck
    if name == "heavypub":
        a, b_ = rs(b"a"), rs(b"b")
        u = [rs(b"u"), 0, L - 1][i % 3]
        return heavy_pub_circuit(), [a, b_, (a * (b_ + u) + u) % L], [], [u]
    if name.startswith("widepub"):
        n = int(name[7:])
        a, d = rs(b"a"), [rs(b"d"), 0, L - 1][i % 3]
        u = [(a + j * d) % L for j in range(n)]
        v0, v1 = rs(b"v0"), rs(b"v1")
        return (wide_pub_circuit(n), [v0, v1, (v0 + u[0]) * v1 % L, sum((j + 1) * x for j, x in enumerate(u)) % L, d],
                [], u)
    if name.startswith("chainpub"):
        n = int(name[8:])
        return chain_pub_circuit(n), [rs(b"v")], [], [rs(b"u%d" % j) for j in range(n)]
    raise KeyError(name)
