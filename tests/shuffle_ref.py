"""Reference for bpp_perm_prove_shuffle_batch (a helper module, not a test):
oracle/bulletproofs.py ac_prove restated for a caller-supplied witness --
deck, permutation and, optionally, the blindings of V_0..V_2k-1 -- out of the
oracle's own pieces (perm_circuit, indexed_scalar, msm, ipa_create,
Transcript).  Only the witness differs from ac_prove: v = [cards, cards[perm],
x_perm] instead of [1..k, perm + 1, x_perm], no pi stream is read, and supplied
gammas replace draws 0..2k-1 (gamma_2k, alpha, beta, rho, s_L, s_R and tau
stay the indexed draws of the seed).  tests/test_shuffle_ref.py pins it to
ac_prove's exact bytes for cards = 1..k, perm = fisher_yates(seed).
"""
from __future__ import annotations

import hashlib

from oracle import bulletproofs as bp, ristretto as r255
from oracle.merlin import Transcript, bulletproof_gens, indexed_scalar, pedersen_gens_default

L = bp.L


def perm_witness(cards, perm, x: int):
    """bp.perm_witness over an explicit deck: v = [cards, cards[perm], x]."""
    k = len(cards)
    v = [c % L for c in cards] + [cards[p] % L for p in perm] + [x % L]
    n = 2 * k
    aL, aR, aO = [0] * n, [0] * n, [0] * n
    for g in range(k - 1):  # chain A: gates 0..k-2
        aL[g] = (v[0] - x) % L if g == 0 else aO[g - 1]
        aR[g] = (v[g + 1] - x) % L
        aO[g] = aL[g] * aR[g] % L
    for g in range(k - 1, 2 * k - 2):  # chain B: gates k-1..2k-3
        aL[g] = (v[k] - x) % L if g == k - 1 else aO[g - 1]
        aR[g] = (v[g + 2] - x) % L
        aO[g] = aL[g] * aR[g] % L
    g = 2 * k - 2
    aL[g], aR[g] = aO[2 * k - 3], L - 1
    aO[g] = aL[g] * aR[g] % L
    g = 2 * k - 1
    aL[g], aR[g] = (aO[k - 2] + aO[2 * k - 2]) % L, 1
    aO[g] = aL[g] * aR[g] % L
    return v, aL, aR, aO


def prove_shuffle(cards, perm, seed, gammas=None, gens=None, label: bytes = b"bp-perm") -> bp.PermProof:
    """cards: k ints < L; perm: a bijection on [0, k); seed: int (u64 test
    seed) or bytes (32-byte entropy seed); gammas: None or 2k ints < L."""
    k = len(cards)
    assert sorted(perm) == list(range(k))
    C = bp.perm_circuit(k)
    n, n_p, m = C.n, C.n_p, C.m
    if gens is None:
        gens = bulletproof_gens(n_p)
    G, H = gens
    g, h = pedersen_gens_default()
    S = [indexed_scalar(seed, j) for j in range(m + 3 + 2 * n_p + 5)]
    gamma = S[:m]
    if gammas is not None:
        assert len(gammas) == 2 * k
        gamma[:2 * k] = [x % L for x in gammas]
    alpha, beta, rho = S[m], S[m + 1], S[m + 2]
    sL = S[m + 3: m + 3 + n_p]
    sR = S[m + 3 + n_p: m + 3 + 2 * n_p]
    taus = S[m + 3 + 2 * n_p:]

    tr = Transcript(label)
    tr.arithmetic_domain_sep(n_p)
    vals = [c % L for c in cards] + [cards[p] % L for p in perm]
    V = []
    for j in range(2 * k):
        V.append(bp.enc(bp.msm([vals[j], gamma[j]], [g, h])))
        tr.append_point(b"V", V[-1])
    x_perm = tr.challenge_scalar(b"x_perm")
    V.append(bp.enc(bp.msm([x_perm, gamma[2 * k]], [g, h])))
    tr.append_point(b"V", V[-1])
    v, aL, aR, aO = perm_witness(cards, perm, x_perm)
    assert not bp.check_constraints(C, v, aL, aR, aO, x_perm)
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


# ----------------------------------------------------------- shared test data
def scalar_bytes(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


def rand_scalar(tag: bytes) -> int:
    """A deterministic 252-bit scalar (top bit of the 252 set, below l)."""
    x = int.from_bytes(hashlib.shake_256(b"shuffle-ref|" + tag).digest(32), "little") % (1 << 251)
    return x | (1 << 251)


def seed32(tag: bytes) -> bytes:
    return hashlib.sha256(b"shuffle-seed|" + tag).digest()


def rand_perm(k: int, tag: bytes):
    p = list(range(k))
    s = hashlib.shake_256(b"shuffle-perm|" + tag).digest(8 * k)
    for i in range(k - 1, 0, -1):
        j = int.from_bytes(s[8 * i: 8 * i + 8], "little") % (i + 1)
        p[i], p[j] = p[j], p[i]
    return p


def edge_decks(k: int):
    """Three decks of k cards that between them hold 0, l - 1, a repeated
    card and 252-bit random cards (every one of them once k >= 4)."""
    rnd = [rand_scalar(b"card-%d-%d" % (k, i)) for i in range(k)]
    a = list(rnd)
    a[0], a[1] = 0, L - 1
    b = list(reversed(rnd))
    b[k - 1] = b[0]  # a repeated 252-bit card
    c = [7] * k  # every card the same
    c[k // 2] = rand_scalar(b"lone-%d" % k)
    if k > 2:
        c[0] = L - 1
    return [a, b, c]
