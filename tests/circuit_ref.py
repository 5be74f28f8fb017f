"""Reference for caller-defined circuits, bpp_circuit_* (a helper module, not a
test), out of the oracle's own pieces (Transcript, indexed_scalar, msm,
ipa_create, ipa_verify_msm_terms, mat_vec_rows, check_constraints), built the
way tests/deck_ref.py is.

A description (bpperm.gadgets.CircuitDesc, or anything with its fields) is a
gate program: committed inputs v_0..v_{m_in-1}, the challenge x, the wires l_h,
r_h, o_h = l_h r_h of n gates.  A gate side is defined (a sparse combination
over {1, v_j, x, wires of gates h < g}) or free (fed from aux); A assert rows
force a combination to 0.  Variable ids: 0 = one, 1 + j = v_j, 1 + m_in = x,
2 + m_in + 3h + {0, 1, 2} = l_h, r_h, o_h.

compile_program: rows = defined left sides by gate, defined right sides by
gate, the asserts, v_{m_in} = x.  Defined side of gate g at row q: W(q, g) = 1
in its own matrix; a wire term a -> -a in the wire's matrix; a v_j / x term ->
W_V = a; the constant -> c[q] = a.  Assert row: wire terms +a, v / x terms -a,
constant -a.  Q = defined sides + A + 1, m = m_in + 1, n_p = max(4,
next_pow2(n)), proof length 32 (13 + 2 lg).

Transcript: Transcript(label), dom-sep("acp v1", n_p), append_message("circuit",
digest), V_0..V_{m_in-1}, challenge x_perm, V_{m_in}, then as bp.ac_prove.
Draws (indexed_scalar): gamma[m], alpha, beta, rho, s_L[n_p], s_R[n_p], tau[5];
supplied gammas replace draws 0..m_in-1; no pi stream is read.
"""
from __future__ import annotations

import hashlib

from oracle import bulletproofs as bp, ristretto as r255
from oracle.merlin import Transcript, bulletproof_gens, indexed_scalar, pedersen_gens_default

L = bp.L
SIDE_LC = 0xFFFFFFFF


def n_p_of(n: int) -> int:
    n_p = 4
    while n_p < n:
        n_p *= 2
    return n_p


def proof_len(desc) -> int:
    lg = n_p_of(desc.n_gates).bit_length() - 1
    return 32 * (13 + 2 * lg)


def _coef(desc, t: int) -> int:
    return int.from_bytes(desc.lc_coef[t], "little")


def _lc_terms(desc, i: int):
    return [(desc.lc_var[t], _coef(desc, t)) for t in range(desc.lc_off[i], desc.lc_off[i + 1])]


def circuit_digest(desc) -> bytes:
    h = hashlib.shake_256(b"bpperm-circuit")
    for x in (desc.m_in, desc.n_gates, desc.n_aux, desc.n_asserts):
        h.update(x.to_bytes(4, "little"))
    for arr in (desc.side_aux, desc.lc_off, desc.lc_var):
        for x in arr:
            h.update(x.to_bytes(4, "little"))
    for c in desc.lc_coef:
        h.update(c)
    return h.digest(32)


def compile_program(desc) -> bp.Circuit:
    m_in, n, A = desc.m_in, desc.n_gates, desc.n_asserts
    defined = sum(1 for a in desc.side_aux if a == SIDE_LC)
    Q = defined + A + 1
    C = bp.Circuit(0, n, n_p_of(n), Q, m_in + 1)
    C.c = [0] * Q
    W = (C.WL, C.WR, C.WO)

    def emit(q, i, sign):  # sign = +1: a definition's row; -1: an assert's
        for var, a in _lc_terms(desc, i):
            if var == 0:
                C.c[q] = (sign * a) % L
            elif var <= 1 + m_in:
                C.WV.append((q, var - 1, (sign * a) % L))
            else:
                w = var - 2 - m_in
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


def eval_program(desc, v, aux, x: int):
    """(a_L, a_R, a_O) of the n gates, and 1 + the first assert that does not
    hold (0: all hold)."""
    m_in, n = desc.m_in, desc.n_gates
    w = [[0] * n, [0] * n, [0] * n]

    def lc(i):
        acc = 0
        for var, a in _lc_terms(desc, i):
            if var == 0:
                val = 1
            elif var <= m_in:
                val = v[var - 1]
            elif var == 1 + m_in:
                val = x
            else:
                val = w[(var - 2 - m_in) % 3][(var - 2 - m_in) // 3]
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


def _transcript(desc, n_p: int, label: bytes) -> Transcript:
    tr = Transcript(label)
    tr.arithmetic_domain_sep(n_p)
    tr.append_message(b"circuit", circuit_digest(desc))
    return tr


def prove_circuit(desc, v, aux, seed, gammas=None, gens=None, label: bytes = b"bp-perm",
                  check: bool = True) -> bp.PermProof:
    """v: m_in ints; aux: n_aux ints; seed: bytes (32-byte entropy seed) or int;
    gammas: None or m_in ints.  check = False proves an unsatisfied witness too
    (the proof must then be rejected)."""
    C = compile_program(desc)
    m_in, n, n_p, m = desc.m_in, C.n, C.n_p, C.m
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

    tr = _transcript(desc, n_p, label)
    vals = [x % L for x in v]
    V = []
    for j in range(m_in):
        V.append(bp.enc(bp.msm([vals[j], gamma[j]], [g, h])))
        tr.append_point(b"V", V[-1])
    x_perm = tr.challenge_scalar(b"x_perm")
    V.append(bp.enc(bp.msm([x_perm, gamma[m_in]], [g, h])))
    tr.append_point(b"V", V[-1])
    aL, aR, aO, bad = eval_program(desc, vals, aux or [], x_perm)
    if check:
        assert not bad and not bp.check_constraints(C, vals + [x_perm], aL, aR, aO, x_perm)
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


def verify_circuit_msm_terms(desc, proof: bp.PermProof, gens=None, label: bytes = b"bp-perm"):
    """bp.ac_verify_msm_terms over the compiled circuit and this transcript:
    (t_check, ipa_check), each of which must sum to the identity."""
    C = compile_program(desc)
    m_in, n_p, m = desc.m_in, C.n_p, C.m
    if gens is None:
        gens = bulletproof_gens(n_p)
    G, H = gens[0][:n_p], gens[1][:n_p]
    g, h = pedersen_gens_default()
    if len(proof.V) != m:
        raise ValueError("VerificationError: V count")
    tr = _transcript(desc, n_p, label)
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
    c = list(C.c)
    c[C.Q - 1] = (-x_perm) % L
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


def verify_circuit(desc, proof: bp.PermProof, gens=None, label: bytes = b"bp-perm") -> bool:
    try:
        (ts, tp), (is_, ip) = verify_circuit_msm_terms(desc, proof, gens, label)
    except (ValueError, r255.DecodeError):
        return False
    ident = r255.IDENTITY
    return r255.equal(bp.msm(ts, tp), ident) and r255.equal(bp.msm(is_, ip), ident)


# ----------------------------------------------------------- the tests' cases

def sb(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


def rand_scalar(tag: bytes) -> int:
    return int.from_bytes(hashlib.shake_256(b"circuit-ref-sc" + tag).digest(64), "little") % L


def seed32(tag: bytes) -> bytes:
    return hashlib.sha256(b"circuit-ref-seed" + tag).digest()


def heavy_circuit():
    """11 gates (n_p = 16): gate 0's output is read by the 10 later left sides
    and by two asserts, and input v_1 by all 11 right sides -- heavy W_O and
    W_V columns that are not the x column."""
    from bpperm.gadgets import CircuitBuilder
    b = CircuitBuilder()
    v0, v1, v2 = b.input(), b.input(), b.input()
    o0 = b.mul(v0, v1 + 1)[2]
    wires = [b.mul(o0 * (g + 1) + g, v1 - g - b.challenge) for g in range(1, 11)]
    b.assert_zero(o0 - v2)                   # v_2 = v_0 (v_1 + 1)
    b.assert_zero(wires[0][0] - o0 * 2 - 1)  # gate 1's left wire restated: l_1 = 2 o_0 + 1
    return b.build()


def wide_circuit(m_in: int = 70):
    """m_in = 70 inputs and one gate (m >> n_p = 4): the product of the first
    two, every other input bound by an assert v_j - v_{j-1} - 1 = 0."""
    from bpperm.gadgets import CircuitBuilder
    b = CircuitBuilder()
    v = b.inputs(m_in)
    o = b.mul(v[0], v[1])[2]
    for j in range(3, m_in):
        b.assert_zero(v[j] - v[j - 1] - 1)
    b.assert_zero(o - v[2])
    return b.build()


def chain_circuit(n: int = 300):
    """A product chain of n gates over one input: o_0 = (v - x)(v + 1), o_g =
    o_{g-1} (v + g + 1); n levels, n_p = 512 at n = 300."""
    from bpperm.gadgets import CircuitBuilder
    b = CircuitBuilder()
    v = b.input()
    o = b.mul(v - b.challenge, v + 1)[2]
    for g in range(1, n):
        o = b.mul(o, v + (g + 1))[2]
    return b.build()


def satisfying(name: str, i: int):
    """(desc, v, aux) of a satisfied instance of the named case; i varies it."""
    from bpperm import gadgets as gd
    t = b"%s-%d" % (name.encode(), i)
    if name == "member2":
        s = [0, L - 1]
        return gd.member_of(s), [s[i % 2]], []
    if name == "member13":
        s = [rand_scalar(b"m13-%d" % j) for j in range(13)]
        return gd.member_of(s), [s[(5 * i + 3) % 13]], []
    if name.startswith("twohalf"):
        k = int(name[7:])
        cards = [rand_scalar(t + b"-%d" % j) for j in range(k)]
        if i == 1:
            cards[0], cards[1] = 0, L - 1
        perm = sorted(range(k), key=lambda j: rand_scalar(t + b"p%d" % j))
        return gd.two_half_shuffle(k), cards + [cards[p] for p in perm], []
    if name.startswith("range"):
        nb = int(name[5:])
        d = gd.in_range(nb)
        v = [[(1 << nb) - 1, 0, 5 % (1 << nb)][i % 3]]
        return d, v, d.aux_of(v)
    if name.startswith("multiset"):
        k = int(name[8:])
        cards = [rand_scalar(t + b"-%d" % j) for j in range(k)]
        return gd.same_multiset(k), cards + cards[::-1], []
    if name == "heavy":
        a = rand_scalar(t + b"a") if i != 2 else 0
        b_ = rand_scalar(t + b"b") if i != 1 else L - 2
        return heavy_circuit(), [a, b_, a * (b_ + 1) % L], []
    if name == "wide70":
        a = rand_scalar(t + b"a") if i != 1 else 0
        b_ = rand_scalar(t + b"b") if i != 2 else L - 1
        c = a * b_ % L
        return wide_circuit(70), [a, b_] + [(c + j) % L for j in range(68)], []
    if name.startswith("chain"):
        return chain_circuit(int(name[5:])), [rand_scalar(t)], []
    raise KeyError(name)
