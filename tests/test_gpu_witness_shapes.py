"""The chain witness's prefix-product scan at the shapes where it changes
path, through the public API only.  One scan serves the seeded prover
(k_witness), the caller's shuffle (k_witness_cards) and the deck circuit
(k_witness_deck).  With C = ceil(k / lanes) elements per lane and nch =
ceil(k / C) active lanes:

  k = 256        C = 1, every lane active, a full 8-step scan
  k = 257        C = 2, nch = 129, the last chunk of one element
  k = 512 / 513  the two-chain kernels' switch from 256 to 128 lanes; 513 has
                 C = 5 and a ragged tail
  k = 768        the last two-chain device witness, every one of 128 lanes full

Two proofs per batch on a 2048-generator set."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import shuffle_ref as sr  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402
from oracle.merlin import Rng  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gens2048(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 2048)
    yield g
    g.close()


def sb(xs):
    return [sr.scalar_bytes(x) for x in xs]


@pytest.mark.parametrize("k", [257, 513])
def test_seeded_matches_c_prover(gens2048, k):
    """The seeded prover's bytes against the serial C prover (oracle/c/
    perm_cpu.c), as test_prove_batch_matches_c_prover_52_card at 52 cards."""
    import bpperm
    from oracle import cport
    pr = bpperm.PermProver(gens2048, k)
    seeds = [k, 7 * k + 1]
    proofs, Vs = pr.prove_batch(seeds)
    for s, pf, V in zip(seeds, proofs, Vs):
        cpf, cV = cport.cpu_prove(k, s)
        assert pf == cpf and V == b"".join(cV)
    assert pr.verify_batch(proofs, Vs)


@pytest.mark.parametrize("k", [256, 257, 512, 513, 768])
def test_shuffle_anchored_to_seeded_prover(ctx, gens2048, k):
    """cards = 1..k and the oracle's Fisher-Yates perms over the seeds' own
    streams: the bytes of bpp_perm_prove_batch_entropy (test_gpu_shuffle's
    anchor at 52 cards), which the verifier accepts.  Then random 252-bit cards
    under random perms: accepted, and nothing of the batch's secrets left."""
    import bpperm
    n = 2
    pr = bpperm.PermProver(gens2048, k)
    seeds = [sr.seed32(b"scan-%d-%d" % (k, i)) for i in range(n)]
    perms = [bp.fisher_yates(k, Rng(s, b"bpperm-prove")) for s in seeds]
    want, wantV = pr.prove_batch_entropy(n, b"".join(seeds))
    got, gotV = pr.prove_shuffle_batch([sb(range(1, k + 1))] * n, perms, b"".join(seeds))
    assert gotV == wantV
    assert got == want
    assert pr.verify_batch(want, wantV)
    cards = [sb(sr.rand_scalar(b"scan-%d-%d-%d" % (k, p, i)) for i in range(k)) for p in range(n)]
    perms = [sr.rand_perm(k, b"scan-%d-%d" % (k, p)) for p in range(n)]
    proofs, Vs = pr.prove_shuffle_batch(cards, perms)
    assert ctx.secret_residue() == 0
    assert pr.verify_batch(proofs, Vs)


@pytest.mark.parametrize("k", [256, 257])
def test_deck_device_witness_matches_host(gens2048, monkeypatch, k):
    """The deck circuit's device witness byte for byte against the host
    witness (BPP_DECK_HOST_WITNESS=1) of the same batch, as
    test_deck_witness_paths at k = 1536."""
    import bpperm
    deck = [sr.rand_scalar(b"scan-deck-%d-%d" % (k, i)) for i in range(k)]
    perms = [sr.rand_perm(k, b"scan-deck-%d-%d" % (k, p)) for p in range(2)]
    seeds = b"".join(sr.seed32(b"scan-deck-%d-%d" % (k, p)) for p in range(2))
    pr = bpperm.DeckProver(gens2048, k, sb(deck))
    proofs, Vs = pr.prove_batch(perms, seeds)
    assert pr.verify_batch(proofs, Vs)
    monkeypatch.setenv("BPP_DECK_HOST_WITNESS", "1")
    host, hostV = pr.prove_batch(perms, seeds)
    monkeypatch.delenv("BPP_DECK_HOST_WITNESS")
    assert host == proofs and hostV == Vs
