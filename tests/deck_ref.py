"""Reference for the public-deck shuffle proof, bpp_deck_prove_batch / bpp_deck_verify*
(a helper module, not a test), out of the oracle's own pieces (Transcript,
indexed_scalar, msm, ipa_create, ipa_verify_msm_terms, mat_vec_rows,
check_constraints).

Statement: V_0..V_{k-1} commit to a permutation of the PUBLIC deck d_0..d_{k-1}
and V_k to the transcript challenge x_perm.  One product chain prod (v_i - x)
inside the proof; the deck's own product D = prod (d_i - x_perm) is a constant
both sides compute (row 2k - 2).  Same convention as bp.perm_circuit:
W_L a_L + W_R a_R + W_O a_O = W_V v + c, v = [d_pi(0) .. d_pi(k-1), x], m = k + 1,
n = k - 1 gates, Q = 2k, n_p = max(4, next_pow2(k - 1)); c[Q - 2] = D and
c[Q - 1] = -x_perm are set per proof.

Transcript: Transcript(label), dom-sep("acp v1", n_p), append_message("deck",
SHAKE256("bpperm-deck" || le32 k || d_0 || .. || d_{k-1})[0..32]), V_0..V_{k-1},
challenge x_perm, V_k, A_I A_O S, ... as bp.ac_prove from there.  Draws
(indexed_scalar): gamma[k + 1], alpha, beta, rho, s_L[n_p], s_R[n_p], tau[5];
supplied gammas replace draws 0..k-1; no pi stream is read.
"""
from __future__ import annotations

import hashlib

from oracle import bulletproofs as bp, ristretto as r255
from oracle.merlin import Transcript, bulletproof_gens, indexed_scalar, pedersen_gens_default

L = bp.L


def deck_n_p(k: int) -> int:
    n_p = 4
    while n_p < k - 1:
        n_p *= 2
    return n_p


def deck_proof_len(k: int) -> int:
    lg = deck_n_p(k).bit_length() - 1
    return 32 * (8 + 3 + 2 * lg + 2)


def deck_circuit(k: int) -> bp.Circuit:
    assert k >= 2
    n = k - 1
    C = bp.Circuit(k, n, deck_n_p(k), 2 * k, k + 1)
    X = k  # column of the committed challenge x in v
    neg1 = L - 1
    C.c = [0] * C.Q  # c[Q-2] = D, c[Q-1] = -x per proof
    for g in range(n):  # a_L rows (q = g)
        C.WL.append((g, g, 1))
        if g == 0:
            C.WV += [(g, 0, 1), (g, X, neg1)]
        else:
            C.WO.append((g, g - 1, neg1))
    for g in range(n):  # a_R rows (q = n + g)
        q = n + g
        C.WR.append((q, g, 1))
        C.WV += [(q, g + 1, 1), (q, X, neg1)]
    C.WO.append((2 * k - 2, k - 2, 1))  # a_O[k-2] = D
    C.WV.append((2 * k - 1, X, 1))      # v_k + c = 0, c = -x
    return C


def deck_product(deck, x: int) -> int:
    D = 1
    for d in deck:
        D = D * ((d - x) % L) % L
    return D


def deck_consts(C: bp.Circuit, deck, x: int):
    c = list(C.c)
    c[C.Q - 2] = deck_product(deck, x)
    c[C.Q - 1] = (-x) % L
    return c


def deck_witness(deck, perm, x: int):
    """v = [deck[perm], x]; gates of the one chain prod (v_i - x)."""
    k = len(deck)
    v = [deck[p] % L for p in perm] + [x % L]
    n = k - 1
    aL, aR, aO = [0] * n, [0] * n, [0] * n
    for g in range(n):
        aL[g] = (v[0] - x) % L if g == 0 else aO[g - 1]
        aR[g] = (v[g + 1] - x) % L
        aO[g] = aL[g] * aR[g] % L
    return v, aL, aR, aO


def check_deck_constraints(C: bp.Circuit, deck, v, aL, aR, aO, x: int):
    """bp.check_constraints with this circuit's second per-proof constant."""
    Cc = bp.Circuit(C.k, C.n, C.n_p, C.Q, C.m)
    Cc.WL, Cc.WR, Cc.WO, Cc.WV = C.WL, C.WR, C.WO, C.WV
    Cc.c = deck_consts(C, deck, x)
    return bp.check_constraints(Cc, v, aL, aR, aO, x)


def deck_digest(deck) -> bytes:
    h = hashlib.shake_256(b"bpperm-deck" + len(deck).to_bytes(4, "little"))
    for d in deck:
        h.update((d % L).to_bytes(32, "little"))
    return h.digest(32)


def _transcript(deck, n_p: int, label: bytes) -> Transcript:
    tr = Transcript(label)
    tr.arithmetic_domain_sep(n_p)
    tr.append_message(b"deck", deck_digest(deck))
    return tr


def default_deck(k: int):
    return list(range(1, k + 1))


def prove_deck(deck, perm, seed, gammas=None, gens=None, label: bytes = b"bp-perm") -> bp.PermProof:
    """deck: k ints < L (None: 1..len(perm)); perm: a bijection on [0, k);
    seed: int (u64 test seed) or bytes (32-byte entropy seed); gammas: None or
    k ints < L."""
    if deck is None:
        deck = default_deck(len(perm))
    k = len(deck)
    assert sorted(perm) == list(range(k))
    C = deck_circuit(k)
    n, n_p, m = C.n, C.n_p, C.m
    if gens is None:
        gens = bulletproof_gens(n_p)
    G, H = gens[0][:n_p], gens[1][:n_p]
    g, h = pedersen_gens_default()
    S = [indexed_scalar(seed, j) for j in range(m + 3 + 2 * n_p + 5)]
    gamma = S[:m]
    if gammas is not None:
        assert len(gammas) == k
        gamma[:k] = [x % L for x in gammas]
    alpha, beta, rho = S[m], S[m + 1], S[m + 2]
    sL = S[m + 3: m + 3 + n_p]
    sR = S[m + 3 + n_p: m + 3 + 2 * n_p]
    taus = S[m + 3 + 2 * n_p:]

    tr = _transcript(deck, n_p, label)
    vals = [deck[p] % L for p in perm]
    V = []
    for j in range(k):
        V.append(bp.enc(bp.msm([vals[j], gamma[j]], [g, h])))
        tr.append_point(b"V", V[-1])
    x_perm = tr.challenge_scalar(b"x_perm")
    V.append(bp.enc(bp.msm([x_perm, gamma[k]], [g, h])))
    tr.append_point(b"V", V[-1])
    v, aL, aR, aO = deck_witness(deck, perm, x_perm)
    assert not check_deck_constraints(C, deck, v, aL, aR, aO, x_perm)
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
    assert t_hat == sum(t[i] * xp[i] for i in range(7)) % L
    tr.append_scalar(b"TX", tau_x)
    tr.append_scalar(b"mu", mu)
    tr.append_scalar(b"t", t_hat)
    w = tr.challenge_scalar(b"w")
    Q = r255.ed_mul(w, g)
    ipa = bp.ipa_create(tr, Q, [1] * n_p, y_inv_n, G, H, l, r)
    return bp.PermProof(V, A_I, A_O, S_, T, tau_x, mu, t_hat, ipa)


def verify_deck_msm_terms(deck, proof: bp.PermProof, gens=None, label: bytes = b"bp-perm"):
    """bp.ac_verify_msm_terms over the deck circuit and transcript: (t_check,
    ipa_check), each of which must sum to the identity."""
    k = len(deck)
    C = deck_circuit(k)
    n_p, m = C.n_p, C.m
    if gens is None:
        gens = bulletproof_gens(n_p)
    G, H = gens[0][:n_p], gens[1][:n_p]
    g, h = pedersen_gens_default()
    if len(proof.V) != m:
        raise ValueError("VerificationError: V count")
    tr = _transcript(deck, n_p, label)
    for j in range(k):
        tr.append_point(b"V", proof.V[j])
    x_perm = tr.challenge_scalar(b"x_perm")
    tr.append_point(b"V", proof.V[k])
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
    c = deck_consts(C, deck, x_perm)
    delta = bp.inner([y_inv_n[i] * zWR[i] % L for i in range(n_p)], zWL)
    Vp = [r255.decode(e) for e in proof.V]
    Tp = [r255.decode(e) for e in proof.T]
    t_sc = [(proof.t_hat - xp[2] * (delta + bp.inner(z_q, c))) % L, proof.tau_x]
    t_sc += [(-xp[2] * zWV[j]) % L for j in range(m)]
    t_sc += [(-xp[i]) % L for i in (1, 3, 4, 5, 6)]
    t_pts = [g, h] + Vp + Tp
    Q = r255.ed_mul(w, g)
    if len(proof.ipa.L) != n_p.bit_length() - 1 or len(proof.ipa.R) != len(proof.ipa.L):
        raise ValueError("VerificationError: IPA rounds")
    ipa_sc, ipa_pts = bp.ipa_verify_msm_terms(proof.ipa, n_p, tr, [1] * n_p, y_inv_n, Q, G, H)
    Pp_sc = [(-x) % L, (-xp[2]) % L, (-xp[3]) % L, proof.mu, (-proof.t_hat * w) % L]
    Pp_pts = [r255.decode(proof.A_I), r255.decode(proof.A_O), r255.decode(proof.S), h, g]
    Pp_sc += [(-x * y_inv_n[i] * zWR[i]) % L for i in range(n_p)]
    Pp_pts += list(G)
    Pp_sc += [(-(y_inv_n[i] * (x * zWL[i] + zWO[i]) - 1)) % L for i in range(n_p)]
    Pp_pts += list(H)
    return (t_sc, t_pts), (ipa_sc + Pp_sc, ipa_pts + Pp_pts)


def verify_deck(deck, proof: bp.PermProof, gens=None, label: bytes = b"bp-perm") -> bool:
    try:
        (ts, tp), (is_, ip) = verify_deck_msm_terms(deck, proof, gens, label)
    except (ValueError, r255.DecodeError):
        return False
    ident = r255.IDENTITY
    return r255.equal(bp.msm(ts, tp), ident) and r255.equal(bp.msm(is_, ip), ident)
