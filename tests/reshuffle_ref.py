"""Reference for the blind re-shuffle proof, bpp_reshuffle_* (a helper module,
not a test): the written specification, out of the oracle's own pieces
(oracle.ristretto, oracle.merlin) and tests/circuit_pub_ref.py's prover and
verifier for the inner proof.  The GPU matches it byte for byte.

Statement.  Public: input cards C_0..C_{k-1} and output cards C'_0..C'_{k-1},
ristretto255 encodings.  The prover knows a bijection pi on [0, k) and scalars
r_i with C'_i = C_{pi(i)} + r_i Bb, Bb = B_blinding; perm[i] = pi(i).  It opens
none of the cards.

Argument, T = Transcript(label), scalars mod l:
  1. append_message("dom-sep", "reshuffle v1"); append_u64("k", k); every C_j
     under "C", every C'_i under "C'".
  2. A_i = pi(i) B + alpha_i Bb under "A"; x = challenge_scalar("x").
  3. e_j = x^(j+1), b_i = e_pi(i); E_i = b_i B + beta_i Bb under "E";
     y = challenge_scalar("y").
  4. T_i = t_i B + w_i Bb under "Ti"; T_S = sum_i t_i C'_i - t_R Bb under "T";
     c = challenge_scalar("c").
  5. z_i = t_i + c b_i; om_i = w_i + c beta_i; z_R = t_R + c sum_i b_i r_i.
  6. D_i = y A_i + E_i commits to d_i = y pi(i) + b_i under delta_i = y alpha_i
     + beta_i: the shuffle_of_public(k) circuit proved with v = d, gammas =
     delta, pub u_j = y j + e_j under the caller's label.  Its V_0..V_{k-1} are
     the D_i byte for byte; V_k and the circuit proof go into the proof.

Proof bytes, 32 (5k + 3) + the circuit proof's:
  A[k] | E[k] | Ti[k] | T_S | z[k] | om[k] | z_R | V_k | inner circuit proof.

The verifier accepts iff (i) z_i B + om_i Bb = T_i + c E_i for every i, (ii)
sum_i z_i C'_i - z_R Bb = T_S + c sum_j e_j C_j, and (iii) the inner proof
verifies for V = (D_0..D_{k-1}, V_k) with D_i = y A_i + E_i formed by the
verifier, and pub = u.

Draws: scalar j = from_wide(SHAKE256("bpperm-reshuffle-sc" || seed32 || le32
j)[0..64]) in the order r[k], alpha[k], beta[k], t[k], w[k], t_R; supplied
blinds replace draws 0..k-1.  The inner prover's seed is
SHAKE256("bpperm-reshuffle-inner" || seed32)[0..32].

Merged form of (i) and (ii) under one weight rho (merged_terms): T_i: -rho^(i+1);
E_i: -rho^(i+1) c; C'_i: rho^(k+1) z_i; C_i: -rho^(k+1) c e_i; T_S: -rho^(k+1);
B: sum_i rho^(i+1) z_i; Bb: sum_i rho^(i+1) om_i - rho^(k+1) z_R.  4k + 3 terms
whose sum is the identity.  A batch derives rho_p = from_wide(SHAKE256(
"bpperm-reshuffle-wt" || seed || le64 p || c_p)[0..64]) and sums the B and Bb
scalars over its proofs.
"""
from __future__ import annotations

import hashlib
import struct

import circuit_pub_ref as cp
from oracle import bulletproofs as bp, ristretto as r255
from oracle.merlin import Transcript, indexed_scalar, pedersen_gens_default

L = bp.L
sb, rand_scalar, seed32 = cp.sb, cp.rand_scalar, cp.seed32
K_MAX = 342  # 2k - 2 gates within the plain circuit bound of 682

_DESC = {}


def desc_of(k: int):
    """shuffle_of_public(k), built once per k."""
    if k not in _DESC:
        from bpperm import gadgets as gd
        _DESC[k] = gd.shuffle_of_public(k)
    return _DESC[k]


def proof_len(k: int) -> int:
    return 32 * (5 * k + 3) + cp.proof_len(desc_of(k))


def regions(k: int):
    """(name, first byte, length) of the nine regions of a proof."""
    out, o = [], 0
    for name, n in (("A", k), ("E", k), ("Ti", k), ("T", 1), ("z", k), ("om", k), ("zR", 1), ("Vk", 1)):
        out.append((name, o, 32 * n))
        o += 32 * n
    out.append(("inner", o, cp.proof_len(desc_of(k))))
    return out


def draws(seed: bytes, k: int, blinds=None):
    """(r, alpha, beta, t, w, t_R) of a proof's seed."""
    S = [indexed_scalar(seed, j, b"bpperm-reshuffle-sc") for j in range(5 * k + 1)]
    if blinds is not None:
        assert len(blinds) == k
        S[:k] = [x % L for x in blinds]
    return S[:k], S[k:2 * k], S[2 * k:3 * k], S[3 * k:4 * k], S[4 * k:5 * k], S[5 * k]


def inner_seed(seed: bytes) -> bytes:
    return hashlib.shake_256(b"bpperm-reshuffle-inner" + seed).digest(32)


def reblind(cards_in, perm, r):
    """C'_i = C_perm[i] + r_i Bb, encoded."""
    _, h = pedersen_gens_default()
    pts = [r255.decode(c) for c in cards_in]
    return [r255.encode(r255.ed_add(pts[perm[i]], r255.ed_mul(r[i] % L, h))) for i in range(len(perm))]


def _start(k: int, label: bytes, cards_in, cards_out) -> Transcript:
    tr = Transcript(label)
    tr.append_message(b"dom-sep", b"reshuffle v1")
    tr.append_u64(b"k", k)
    for c in cards_in:
        tr.append_message(b"C", c)
    for c in cards_out:
        tr.append_message(b"C'", c)
    return tr


def _commit(v: int, g_: int) -> bytes:
    g, h = pedersen_gens_default()
    return bp.enc(bp.msm([v % L, g_ % L], [g, h]))


def _inner_bytes(pf: bp.PermProof) -> bytes:
    return pf.to_bytes()


def _inner_parse(k: int, V, raw: bytes) -> bp.PermProof:
    lg = cp.n_p_of(desc_of(k).n_gates).bit_length() - 1
    f = [raw[32 * i:32 * i + 32] for i in range(len(raw) // 32)]
    num = lambda b: int.from_bytes(b, "little")
    ipa = bp.IPAProof([f[11 + 2 * j] for j in range(lg)], [f[12 + 2 * j] for j in range(lg)], num(f[11 + 2 * lg]),
                      num(f[12 + 2 * lg]))
    return bp.PermProof(list(V), f[0], f[1], f[2], f[3:8], num(f[8]), num(f[9]), num(f[10]), ipa)


def prove(cards_in, perm, seed: bytes, blinds=None, label: bytes = b"bp-perm", cards_out=None, force: bool = False):
    """(cards_out, proof) for k = len(cards_in) encodings, perm a bijection on
    [0, k), seed 32 bytes, blinds None or k ints (the r_i).  cards_out: None,
    or the outputs to prove instead of the honest ones (a forced proof of a
    statement that need not hold).  force: perm need not be a bijection either,
    and the inner circuit is proved unchecked."""
    k = len(cards_in)
    assert 2 <= k <= K_MAX and len(perm) == k and (force or sorted(perm) == list(range(k)))
    desc = desc_of(k)
    g, h = pedersen_gens_default()
    r, alpha, beta, t, w, t_R = draws(seed, k, blinds)
    if cards_out is None:
        cards_out = reblind(cards_in, perm, r)
    out_pts = [r255.decode(c) for c in cards_out]
    tr = _start(k, label, cards_in, cards_out)
    A = [_commit(perm[i], alpha[i]) for i in range(k)]
    for a in A:
        tr.append_message(b"A", a)
    x = tr.challenge_scalar(b"x")
    e = [pow(x, j + 1, L) for j in range(k)]
    b = [e[perm[i]] for i in range(k)]
    E = [_commit(b[i], beta[i]) for i in range(k)]
    for p in E:
        tr.append_message(b"E", p)
    y = tr.challenge_scalar(b"y")
    Ti = [_commit(t[i], w[i]) for i in range(k)]
    for p in Ti:
        tr.append_message(b"Ti", p)
    T_S = bp.enc(bp.msm(list(t) + [(-t_R) % L], out_pts + [h]))
    tr.append_message(b"T", T_S)
    c = tr.challenge_scalar(b"c")
    z = [(t[i] + c * b[i]) % L for i in range(k)]
    om = [(w[i] + c * beta[i]) % L for i in range(k)]
    R = sum(b[i] * r[i] for i in range(k)) % L
    z_R = (t_R + c * R) % L
    d = [(y * perm[i] + b[i]) % L for i in range(k)]
    delta = [(y * alpha[i] + beta[i]) % L for i in range(k)]
    u = [(y * j + e[j]) % L for j in range(k)]
    inner = cp.prove_circuit(desc, d, [], u, inner_seed(seed), delta, label=label, check=not force)
    proof = b"".join(A) + b"".join(E) + b"".join(Ti) + T_S + b"".join(sb(s) for s in z) + b"".join(sb(s) for s in om)
    proof += sb(z_R) + inner.V[k] + _inner_bytes(inner)
    assert len(proof) == proof_len(k)
    return list(cards_out), proof


class Parsed:
    """A proof's fields and its replayed challenges; raises ValueError (a
    scalar >= l, a wrong length) or r255.DecodeError (a point)."""

    def __init__(self, cards_in, cards_out, proof: bytes, label: bytes):
        k = self.k = len(cards_in)
        if len(cards_out) != k or len(proof) != proof_len(k):
            raise ValueError("length")
        f = [proof[32 * i:32 * i + 32] for i in range(5 * k + 3)]
        self.A, self.E, self.Ti, self.T_S = f[:k], f[k:2 * k], f[2 * k:3 * k], f[3 * k]
        sc = [r255.scalar_from_canonical(s) for s in f[3 * k + 1:5 * k + 2]]
        self.z, self.om, self.z_R = sc[:k], sc[k:2 * k], sc[2 * k]
        self.V_k = f[5 * k + 2]
        self.inner = proof[32 * (5 * k + 3):]
        self.Cp = [r255.decode(c) for c in cards_in]
        self.Op = [r255.decode(c) for c in cards_out]
        self.Ap, self.Ep, self.Tp = ([r255.decode(p) for p in ps] for ps in (self.A, self.E, self.Ti))
        self.TSp = r255.decode(self.T_S)
        tr = _start(k, label, cards_in, cards_out)
        for a in self.A:
            tr.append_message(b"A", a)
        self.x = tr.challenge_scalar(b"x")
        for p in self.E:
            tr.append_message(b"E", p)
        self.y = tr.challenge_scalar(b"y")
        for p in self.Ti:
            tr.append_message(b"Ti", p)
        tr.append_message(b"T", self.T_S)
        self.c = tr.challenge_scalar(b"c")
        self.e = [pow(self.x, j + 1, L) for j in range(k)]
        self.u = [(self.y * j + self.e[j]) % L for j in range(k)]

    def D(self):
        return [r255.encode(r255.ed_add(r255.ed_mul(self.y, a), e)) for a, e in zip(self.Ap, self.Ep)]


def merged_terms(P: Parsed, rho: int):
    """(scalars, points) of checks (i) and (ii) under the weight rho: 4k + 3
    terms in the order T_i, E_i, C'_i, C_i, T_S, B, Bb."""
    k, c = P.k, P.c
    g, h = pedersen_gens_default()
    rp = [pow(rho, i + 1, L) for i in range(k + 1)]
    sc = [(-rp[i]) % L for i in range(k)]
    sc += [(-rp[i] * c) % L for i in range(k)]
    sc += [rp[k] * P.z[i] % L for i in range(k)]
    sc += [(-rp[k] * c * P.e[i]) % L for i in range(k)]
    sc += [(-rp[k]) % L]
    sc += [sum(rp[i] * P.z[i] for i in range(k)) % L]
    sc += [(sum(rp[i] * P.om[i] for i in range(k)) - rp[k] * P.z_R) % L]
    return sc, P.Tp + P.Ep + P.Op + P.Cp + [P.TSp, g, h]


def batch_weight(seed: bytes, p: int, c: int) -> int:
    return r255.scalar_from_wide(hashlib.shake_256(b"bpperm-reshuffle-wt" + seed + struct.pack("<Q", p) + sb(c)).digest(64))


def verify_parts(cards_in, cards_out, proof: bytes, label: bytes = b"bp-perm"):
    """(sigma, inner): checks (i) and (ii) as stated, and check (iii)."""
    try:
        P = Parsed(cards_in, cards_out, proof, label)
    except (ValueError, r255.DecodeError):
        return False, False
    k, c = P.k, P.c
    g, h = pedersen_gens_default()
    ok = True
    for i in range(k):
        lhs = bp.msm([P.z[i], P.om[i]], [g, h])
        ok &= r255.equal(lhs, r255.ed_add(P.Tp[i], r255.ed_mul(c, P.Ep[i])))
    lhs = bp.msm(P.z + [(-P.z_R) % L], P.Op + [h])
    rhs = r255.ed_add(P.TSp, r255.ed_mul(c, bp.msm(P.e, P.Cp)))
    ok &= r255.equal(lhs, rhs)
    inner = cp.verify_circuit(desc_of(k), _inner_parse(k, P.D() + [P.V_k], P.inner), P.u, label=label)
    return bool(ok), bool(inner)


def verify(cards_in, cards_out, proof: bytes, label: bytes = b"bp-perm") -> bool:
    return all(verify_parts(cards_in, cards_out, proof, label))


# ----------------------------------------------------------- the tests' cases

def commit_cards(values, gammas):
    """Pedersen commitments v B + gamma Bb, encoded: a first committer's deck."""
    return [_commit(v, g_) for v, g_ in zip(values, gammas)]


def rand_perm(k: int, tag: bytes):
    return sorted(range(k), key=lambda i: hashlib.sha256(b"reshuffle-perm" + tag + b"%d" % i).digest())


def rand_cards(k: int, tag: bytes):
    """k cards nobody opens: from_uniform_bytes of a hash."""
    return [r255.encode(r255.from_uniform_bytes(hashlib.shake_256(b"reshuffle-card" + tag + b"%d" % i).digest(64)))
            for i in range(k)]


IDENTITY = bytes(32)


def edge_case(k: int, name: str):
    """(cards_in, perm, blinds) of the named edge input at k cards."""
    cards = rand_cards(k, b"edge-" + name.encode())
    perm = rand_perm(k, b"edge-" + name.encode())
    blinds = None
    if name == "identity-card":
        cards[k - 1] = IDENTITY
    elif name == "equal-cards":
        cards[1] = cards[0]
    elif name == "zero-blind":
        blinds = [rand_scalar(b"edge-r%d" % i) for i in range(k)]
        blinds[0] = 0
    elif name == "pi-identity":
        perm = list(range(k))
    elif name == "pi-reversal":
        perm = list(range(k))[::-1]
    else:
        raise KeyError(name)
    return cards, perm, blinds


EDGES = ("identity-card", "equal-cards", "zero-blind", "pi-identity", "pi-reversal")
