"""Reference for the masked re-shuffle proof, bpp_masked_reshuffle_* (a helper
module, not a test): the blind re-shuffle of tests/reshuffle_ref.py widened from
one group element per card to an ElGamal pair under a joint key.  Everything not
stated here is that helper's, reused as it is.  The GPU matches it byte for byte.

Statement.  Public: a key K, input cards (U_j, W_j) and output cards (U'_i,
W'_i), ristretto255 encodings, a card the 64 bytes U | W.  The prover knows a
bijection pi on [0, k) and scalars r_i with U'_i = U_{pi(i)} + r_i B and W'_i =
W_{pi(i)} + r_i K, B the Pedersen value base; perm[i] = pi(i).

Argument, T = Transcript(label), scalars mod l:
  1. append_message("dom-sep", "masked reshuffle v1"); append_u64("k", k); K
     under "K"; every input card as U_j then W_j under "C" (2k messages), every
     output card the same way under "C'".
  2. A_i, x, E_i, y as in the blind re-shuffle.
  3. T_i = t_i B + w_i Bb under "Ti"; T_U = sum_i t_i U'_i - t_R B and T_W =
     sum_i t_i W'_i - t_R K under "T", T_U first; c = challenge_scalar("c").
  4. z_i, om_i, z_R = t_R + c sum_i b_i r_i and the inner proof as there.

Proof bytes, 32 (5k + 4) + the circuit proof's:
  A[k] | E[k] | Ti[k] | T_U | T_W | z[k] | om[k] | z_R | V_k | circuit proof.

The verifier accepts iff (i) z_i B + om_i Bb = T_i + c E_i for every i, (ii-U)
sum_i z_i U'_i - z_R B = T_U + c sum_j e_j U_j, (ii-W) sum_i z_i W'_i - z_R K =
T_W + c sum_j e_j W_j, and (iii) the inner proof verifies.

Draws, the inner seed and the batch weight are the blind re-shuffle's, domain
strings included (a seed serves one proof of either kind, never both).

Merged form of (i), (ii-U), (ii-W) under one weight rho (merged_terms): T_i:
-rho^(i+1); E_i: -rho^(i+1) c; U'_i: rho^(k+1) z_i; W'_i: rho^(k+2) z_i; U_j:
-rho^(k+1) c e_j; W_j: -rho^(k+2) c e_j; T_U: -rho^(k+1); T_W: -rho^(k+2); B:
sum_i rho^(i+1) z_i - rho^(k+1) z_R; Bb: sum_i rho^(i+1) om_i; K: -rho^(k+2)
z_R.  6k + 5 terms whose sum is the identity.
"""
from __future__ import annotations

import hashlib

import circuit_pub_ref as cp
import reshuffle_ref as rr
from oracle import bulletproofs as bp, ristretto as r255
from oracle.merlin import Transcript, pedersen_gens_default

L = rr.L
sb, rand_scalar, seed32, rand_perm = rr.sb, rr.rand_scalar, rr.seed32, rr.rand_perm
desc_of, draws, inner_seed, batch_weight = rr.desc_of, rr.draws, rr.inner_seed, rr.batch_weight
K_MAX, IDENTITY = rr.K_MAX, rr.IDENTITY


def proof_len(k: int) -> int:
    return rr.proof_len(k) + 32


def regions(k: int):
    """(name, first byte, length) of the ten regions of a proof."""
    out, o = [], 0
    for name, n in (("A", k), ("E", k), ("Ti", k), ("TU", 1), ("TW", 1), ("z", k), ("om", k), ("zR", 1), ("Vk", 1)):
        out.append((name, o, 32 * n))
        o += 32 * n
    out.append(("inner", o, cp.proof_len(desc_of(k))))
    return out


def halves(card: bytes):
    assert len(card) == 64
    return card[:32], card[32:]


def _decode(cards):
    """The cards' U points and W points."""
    return [r255.decode(c[:32]) for c in cards], [r255.decode(c[32:]) for c in cards]


def key_of(sk: int) -> bytes:
    """K = sk B, encoded."""
    g, _ = pedersen_gens_default()
    return r255.encode(r255.ed_mul(sk % L, g))


def remask(key: bytes, cards_in, perm, r):
    """(U_perm[i] + r_i B, W_perm[i] + r_i K), encoded."""
    g, _ = pedersen_gens_default()
    Kp = r255.decode(key)
    U, W = _decode(cards_in)
    return [r255.encode(r255.ed_add(U[perm[i]], r255.ed_mul(r[i] % L, g))) +
            r255.encode(r255.ed_add(W[perm[i]], r255.ed_mul(r[i] % L, Kp))) for i in range(len(perm))]


def _start(k: int, label: bytes, key: bytes, cards_in, cards_out) -> Transcript:
    tr = Transcript(label)
    tr.append_message(b"dom-sep", b"masked reshuffle v1")
    tr.append_u64(b"k", k)
    tr.append_message(b"K", key)
    for lab, cards in ((b"C", cards_in), (b"C'", cards_out)):
        for c in cards:
            u, w = halves(c)
            tr.append_message(lab, u)
            tr.append_message(lab, w)
    return tr


def prove(key: bytes, cards_in, perm, seed: bytes, blinds=None, label: bytes = b"bp-perm", cards_out=None,
          force: bool = False):
    """(cards_out, proof) for k = len(cards_in) 64-byte cards under the key,
    perm a bijection on [0, k), seed 32 bytes, blinds None or k ints (the r_i).
    cards_out: None, or the outputs to prove instead of the honest ones (a
    forced proof of a statement that need not hold).  force: perm need not be
    a bijection either, and the inner circuit is proved unchecked."""
    k = len(cards_in)
    assert 2 <= k <= K_MAX and len(perm) == k and (force or sorted(perm) == list(range(k)))
    desc = desc_of(k)
    g, h = pedersen_gens_default()
    Kp = r255.decode(key)
    r, alpha, beta, t, w, t_R = draws(seed, k, blinds)
    if cards_out is None:
        cards_out = remask(key, cards_in, perm, r)
    Uo, Wo = _decode(cards_out)
    tr = _start(k, label, key, cards_in, cards_out)
    A = [rr._commit(perm[i], alpha[i]) for i in range(k)]
    for a in A:
        tr.append_message(b"A", a)
    x = tr.challenge_scalar(b"x")
    e = [pow(x, j + 1, L) for j in range(k)]
    b = [e[perm[i]] for i in range(k)]
    E = [rr._commit(b[i], beta[i]) for i in range(k)]
    for p in E:
        tr.append_message(b"E", p)
    y = tr.challenge_scalar(b"y")
    Ti = [rr._commit(t[i], w[i]) for i in range(k)]
    for p in Ti:
        tr.append_message(b"Ti", p)
    T_U = bp.enc(bp.msm(list(t) + [(-t_R) % L], Uo + [g]))
    T_W = bp.enc(bp.msm(list(t) + [(-t_R) % L], Wo + [Kp]))
    tr.append_message(b"T", T_U)
    tr.append_message(b"T", T_W)
    c = tr.challenge_scalar(b"c")
    z = [(t[i] + c * b[i]) % L for i in range(k)]
    om = [(w[i] + c * beta[i]) % L for i in range(k)]
    R = sum(b[i] * r[i] for i in range(k)) % L
    z_R = (t_R + c * R) % L
    d = [(y * perm[i] + b[i]) % L for i in range(k)]
    delta = [(y * alpha[i] + beta[i]) % L for i in range(k)]
    u = [(y * j + e[j]) % L for j in range(k)]
    inner = cp.prove_circuit(desc, d, [], u, inner_seed(seed), delta, label=label, check=not force)
    proof = b"".join(A) + b"".join(E) + b"".join(Ti) + T_U + T_W + b"".join(sb(s) for s in z)
    proof += b"".join(sb(s) for s in om) + sb(z_R) + inner.V[k] + inner.to_bytes()
    assert len(proof) == proof_len(k)
    return list(cards_out), proof


class Parsed:
    """A proof's fields and its replayed challenges; raises ValueError (a
    scalar >= l, a wrong length) or r255.DecodeError (a point)."""

    def __init__(self, key: bytes, cards_in, cards_out, proof: bytes, label: bytes):
        k = self.k = len(cards_in)
        if len(cards_out) != k or len(proof) != proof_len(k) or any(len(c) != 64 for c in list(cards_in) + list(cards_out)):
            raise ValueError("length")
        f = [proof[32 * i:32 * i + 32] for i in range(5 * k + 4)]
        self.A, self.E, self.Ti, self.T_U, self.T_W = f[:k], f[k:2 * k], f[2 * k:3 * k], f[3 * k], f[3 * k + 1]
        sc = [r255.scalar_from_canonical(s) for s in f[3 * k + 2:5 * k + 3]]
        self.z, self.om, self.z_R = sc[:k], sc[k:2 * k], sc[2 * k]
        self.V_k = f[5 * k + 3]
        self.inner = proof[32 * (5 * k + 4):]
        self.Kp = r255.decode(key)
        self.Up, self.Wp = _decode(cards_in)
        self.UOp, self.WOp = _decode(cards_out)
        self.Ap, self.Ep, self.Tp = ([r255.decode(p) for p in ps] for ps in (self.A, self.E, self.Ti))
        self.TUp, self.TWp = r255.decode(self.T_U), r255.decode(self.T_W)
        tr = _start(k, label, key, cards_in, cards_out)
        for a in self.A:
            tr.append_message(b"A", a)
        self.x = tr.challenge_scalar(b"x")
        for p in self.E:
            tr.append_message(b"E", p)
        self.y = tr.challenge_scalar(b"y")
        for p in self.Ti:
            tr.append_message(b"Ti", p)
        tr.append_message(b"T", self.T_U)
        tr.append_message(b"T", self.T_W)
        self.c = tr.challenge_scalar(b"c")
        self.e = [pow(self.x, j + 1, L) for j in range(k)]
        self.u = [(self.y * j + self.e[j]) % L for j in range(k)]

    def D(self):
        return [r255.encode(r255.ed_add(r255.ed_mul(self.y, a), e)) for a, e in zip(self.Ap, self.Ep)]


def merged_terms(P: Parsed, rho: int):
    """(scalars, points) of checks (i), (ii-U) and (ii-W) under the weight rho:
    6k + 5 terms in the order T_i, E_i, U'_i, W'_i, U_j, W_j, T_U, T_W, B, Bb, K."""
    k, c = P.k, P.c
    g, h = pedersen_gens_default()
    rp = [pow(rho, i + 1, L) for i in range(k + 2)]
    ru, rw = rp[k], rp[k + 1]
    sc = [(-rp[i]) % L for i in range(k)]
    sc += [(-rp[i] * c) % L for i in range(k)]
    sc += [ru * P.z[i] % L for i in range(k)]
    sc += [rw * P.z[i] % L for i in range(k)]
    sc += [(-ru * c * P.e[i]) % L for i in range(k)]
    sc += [(-rw * c * P.e[i]) % L for i in range(k)]
    sc += [(-ru) % L, (-rw) % L]
    sc += [(sum(rp[i] * P.z[i] for i in range(k)) - ru * P.z_R) % L]
    sc += [sum(rp[i] * P.om[i] for i in range(k)) % L]
    sc += [(-rw * P.z_R) % L]
    return sc, P.Tp + P.Ep + P.UOp + P.WOp + P.Up + P.Wp + [P.TUp, P.TWp, g, h, P.Kp]


def verify_parts(key: bytes, cards_in, cards_out, proof: bytes, label: bytes = b"bp-perm"):
    """(i, ii_U, ii_W, inner): one verdict per check, each as stated."""
    try:
        P = Parsed(key, cards_in, cards_out, proof, label)
    except (ValueError, r255.DecodeError):
        return False, False, False, False
    k, c = P.k, P.c
    g, h = pedersen_gens_default()
    one = True
    for i in range(k):
        lhs = bp.msm([P.z[i], P.om[i]], [g, h])
        one &= r255.equal(lhs, r255.ed_add(P.Tp[i], r255.ed_mul(c, P.Ep[i])))

    def two(outs, base, T, ins):
        lhs = bp.msm(P.z + [(-P.z_R) % L], outs + [base])
        return r255.equal(lhs, r255.ed_add(T, r255.ed_mul(c, bp.msm(P.e, ins))))

    inner = cp.verify_circuit(desc_of(k), rr._inner_parse(k, P.D() + [P.V_k], P.inner), P.u, label=label)
    return bool(one), bool(two(P.UOp, g, P.TUp, P.Up)), bool(two(P.WOp, P.Kp, P.TWp, P.Wp)), bool(inner)


def verify(key: bytes, cards_in, cards_out, proof: bytes, label: bytes = b"bp-perm") -> bool:
    return all(verify_parts(key, cards_in, cards_out, proof, label))


def unmask(cards, sk: int):
    """M_i = W_i - sk U_i, encoded: what the key's discrete log opens."""
    U, W = _decode(cards)
    return [r255.encode(r255.ed_add(w, r255.ed_neg(r255.ed_mul(sk % L, u)))) for u, w in zip(U, W)]


# ----------------------------------------------------------- the tests' cases

def rand_point(tag: bytes) -> bytes:
    return rr.rand_cards(1, b"masked-" + tag)[0]


def rand_cards(k: int, tag: bytes):
    """k cards nobody opens: both halves from_uniform_bytes of a hash."""
    pts = rr.rand_cards(2 * k, b"masked-" + tag)
    return [pts[2 * i] + pts[2 * i + 1] for i in range(k)]


def open_deck(M):
    """(identity, M_j): the deck every masked game starts from, no proof needed."""
    return [IDENTITY + m for m in M]


def edge_case(k: int, name: str):
    """(key, cards_in, perm, blinds) of the named edge input at k cards."""
    tag = b"edge-" + name.encode()
    key = rand_point(tag + b"-key")
    cards = rand_cards(k, tag)
    perm = rand_perm(k, tag)
    blinds = None
    if name == "open-deck":
        cards = open_deck([c[32:] for c in cards])
    elif name == "identity-card":
        cards[k - 1] = IDENTITY + IDENTITY
    elif name == "equal-cards":
        cards[1] = cards[0]
    elif name == "zero-blind":
        blinds = [rand_scalar(b"edge-r%d" % i) for i in range(k)]
        blinds[0] = 0
    elif name == "pi-identity":
        perm = list(range(k))
    elif name == "pi-reversal":
        perm = list(range(k))[::-1]
    elif name == "key-identity":
        key = IDENTITY
    else:
        raise KeyError(name)
    return key, cards, perm, blinds


EDGES = ("open-deck", "identity-card", "equal-cards", "zero-blind", "pi-identity", "pi-reversal", "key-identity")
