"""bpp_perm_prove_shuffle_batch on the GPU: proofs of caller-supplied shuffles
(own deck, own permutation, own blindings) byte-exact against the reference
helper (tests/shuffle_ref.py, pinned to the oracle's ac_prove by
tests/test_shuffle_ref.py), anchored to the seeded prover's bytes, accepted and
rejected by the unchanged verifiers, on the large-k witness paths, and with the
batch's secrets wiped."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import shuffle_ref as sr  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402
from oracle.merlin import Rng  # noqa: E402

pytestmark = pytest.mark.gpu
L = bp.L


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens2048(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 2048)
    yield g
    g.close()


def deck_bytes(deck):
    return [sr.scalar_bytes(c) for c in deck]


def case(k, with_gammas):
    """Three shuffles of k cards: decks with 0, l - 1, a repeated card and
    252-bit cards, three different perms, 32-byte seeds."""
    decks = sr.edge_decks(k)
    perms = [sr.rand_perm(k, b"gpu-%d-%d" % (k, i)) for i in range(3)]
    seeds = [sr.seed32(b"gpu-%d-%d" % (k, i)) for i in range(3)]
    gam = None
    if with_gammas:
        gam = [[sr.rand_scalar(b"gam-%d-%d-%d" % (k, i, j)) for j in range(2 * k)] for i in range(3)]
        gam[1][0], gam[1][1] = 0, L - 1  # edge blindings too
    return decks, perms, seeds, gam


@pytest.mark.parametrize("with_gammas", [False, True], ids=["drawn", "supplied"])
@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_shuffle_bit_exact_vs_helper(gens, k, with_gammas):
    """k = 2: the shortest chains; 5: padded gates; 8: 2k = n_p, no padding.
    V and proof bytes equal the helper's, bpp_perm_verify and the oracle's
    ac_verify accept, and a second identical call returns the same bytes."""
    import bpperm
    decks, perms, seeds, gam = case(k, with_gammas)
    pr = bpperm.PermProver(gens, k)
    args = ([deck_bytes(d) for d in decks], perms, b"".join(seeds),
            [deck_bytes(g) for g in gam] if gam else None)
    proofs, Vs = pr.prove_shuffle_batch(*args)
    for i in range(3):
        want = sr.prove_shuffle(decks[i], perms[i], seeds[i], gam[i] if gam else None)
        assert Vs[i] == b"".join(want.V), i
        assert proofs[i] == want.to_bytes(), i
        assert pr.verify(proofs[i], Vs[i])
        assert bp.ac_verify(k, want)
    again, Vagain = pr.prove_shuffle_batch(*args)
    assert again == proofs and Vagain == Vs


def test_shuffle_anchored_to_seeded_prover(gens):
    """cards = 1..k, perms = the permutations the seeded prover derives from
    the same 32-byte seeds, no gammas: the bytes of
    bpp_perm_prove_batch_entropy.  52 cards, 9 proofs (a lockstep group of 8
    and a tail of 1).  The 32-byte-seed prover returns no permutation, so the
    perms are the oracle's Fisher-Yates over the same stream -- which is what
    PermProver.prove returns for its u64 seeds (checked first)."""
    import bpperm
    k, n = 52, 9
    pr = bpperm.PermProver(gens, k)
    _, _, dev_perm = pr.prove(77)
    assert dev_perm == bp.fisher_yates(k, Rng(77, b"bpperm-prove"))
    seeds = [sr.seed32(b"anchor-%d" % i) for i in range(n)]
    perms = [bp.fisher_yates(k, Rng(s, b"bpperm-prove")) for s in seeds]
    assert len({tuple(p) for p in perms}) == n
    want, wantV = pr.prove_batch_entropy(n, b"".join(seeds))
    cards = [deck_bytes(range(1, k + 1))] * n
    got, gotV = pr.prove_shuffle_batch(cards, perms, b"".join(seeds))
    assert gotV == wantV
    assert got == want


def test_shuffle_verification_accepts_and_rejects(gens):
    """The unchanged batch verifier takes new and seeded proofs together, and
    rejects two swapped output commitments, one proof's V under another's
    proof, and a flipped proof byte."""
    import bpperm
    k = 5
    decks, perms, seeds, gam = case(k, True)
    pr = bpperm.PermProver(gens, k)
    new, newV = pr.prove_shuffle_batch([deck_bytes(d) for d in decks], perms, b"".join(seeds),
                                       [deck_bytes(g) for g in gam])
    old, oldV = pr.prove_batch([51, 52, 53])
    proofs, Vs = [new[0], old[0], new[1], old[1], new[2], old[2]], [newV[0], oldV[0], newV[1], oldV[1], newV[2], oldV[2]]
    assert pr.verify_batch(proofs, Vs)
    # output commitments k and k + 1 of the first new proof swapped
    v = Vs[0]
    a, b = v[32 * k: 32 * k + 32], v[32 * (k + 1): 32 * (k + 2)]
    assert a != b
    sw = v[:32 * k] + b + a + v[32 * (k + 2):]
    assert not pr.verify_batch(proofs, [sw] + Vs[1:])
    assert not pr.verify(proofs[0], sw)
    # proof 0's V under proof 2 and the reverse
    assert not pr.verify_batch(proofs, [Vs[2], Vs[1], Vs[0]] + Vs[3:])
    bad = bytearray(proofs[4])
    bad[37] ^= 1
    assert not pr.verify_batch(proofs[:4] + [bytes(bad)] + proofs[5:], Vs)
    assert pr.verify_batch(proofs, Vs)


def big_case(k, n, tag):
    decks = [[sr.rand_scalar(b"%s-%d-%d-%d" % (tag, k, p, i)) for i in range(k)] for p in range(n)]
    perms = [sr.rand_perm(k, b"%s-%d-%d" % (tag, k, p)) for p in range(n)]
    return [deck_bytes(d) for d in decks], perms


@pytest.mark.parametrize("k", [600, 769])
def test_shuffle_large_k(ctx, gens2048, k):
    """k = 600: the device witness on 128 lanes with several elements per
    lane; k = 769: the host witness.  252-bit cards; the verifier accepts and
    nothing of the batch's secrets is left."""
    import bpperm
    pr = bpperm.PermProver(gens2048, k)
    cards, perms = big_case(k, 2, b"big")
    proofs, Vs = pr.prove_shuffle_batch(cards, perms)
    assert ctx.secret_residue() == 0
    assert pr.verify_batch(proofs, Vs)
    # the same shuffles under supplied blindings
    gam = [[sr.scalar_bytes(sr.rand_scalar(b"bg-%d-%d-%d" % (k, p, j))) for j in range(2 * k)] for p in range(2)]
    proofs2, Vs2 = pr.prove_shuffle_batch(cards, perms, gammas=gam)
    assert ctx.secret_residue() == 0
    assert pr.verify_batch(proofs2, Vs2)
    assert Vs2 != Vs


@pytest.mark.parametrize("streams", [1, 3])
def test_shuffle_leaves_no_secret_bytes(ctx, gens, monkeypatch, streams):
    """52 cards on one stream and on three sub-batch streams
    (BPP_PROVE_STREAMS): the same bytes either way for fixed seeds, the
    verifier accepts, and every span that held cards, perms, gammas, draws or
    witness reads back as zero -- after a test-hook batch had left its own."""
    import bpperm
    k, n = 52, 7
    pr = bpperm.PermProver(gens, k)
    cards, perms = big_case(k, n, b"res")
    seeds = b"".join(sr.seed32(b"res-%d" % i) for i in range(n))
    gam = [[sr.scalar_bytes(sr.rand_scalar(b"rg-%d-%d" % (p, j))) for j in range(2 * k)] for p in range(n)]
    monkeypatch.setenv("BPP_PROVE_STREAMS", "1")
    want, wantV = pr.prove_shuffle_batch(cards, perms, seeds, gam)
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    pr.prove_batch([3, 4, 5])  # a test-hook batch leaves its secrets in place
    assert ctx.secret_residue() > 0
    got, gotV = pr.prove_shuffle_batch(cards, perms, seeds, gam)
    assert ctx.secret_residue() == 0
    assert got == want and gotV == wantV
    assert pr.verify_batch(got, gotV)


def test_seeded_prover_unchanged_after_a_shuffle_batch(gens):
    """The same context and thread prove the 52-card u64-seed batch to the
    same bytes before and after a shuffle batch (its wipe, its larger input
    workspace and its full-width V tables leave nothing behind)."""
    import bpperm
    k = 52
    pr = bpperm.PermProver(gens, k)
    seeds = [11, 12, 13, 14, 15]
    before, vb = pr.prove_batch(seeds)
    cards, perms = big_case(k, 3, b"mid")
    s, sv = pr.prove_shuffle_batch(cards, perms)
    after, va = pr.prove_batch(seeds)
    assert before == after and vb == va
    assert pr.verify_batch(s + after, sv + va)
