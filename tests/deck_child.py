"""Child process of tests/test_gpu_deck.py (a helper, not a test): proves the
fixed deck batch of deck_case() under whatever BPP_* switches the parent put in
the environment and prints the proofs and V as one hex line each."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import shuffle_ref as sr  # noqa: E402


def deck_case(k=6, n=5):
    deck = sr.edge_decks(k)[0]
    perms = [sr.rand_perm(k, b"deck-child-%d" % i) for i in range(n)]
    seeds = b"".join(sr.seed32(b"deck-child-%d" % i) for i in range(n))
    gam = [[sr.scalar_bytes(sr.rand_scalar(b"deck-child-g-%d-%d" % (i, j))) for j in range(k)] for i in range(n)]
    return k, [sr.scalar_bytes(c) for c in deck], perms, seeds, gam


def prove(ctx=None):
    import bpperm
    k, deck, perms, seeds, gam = deck_case()
    own = ctx is None
    if own:
        ctx = bpperm.Context(0)
    g = bpperm.Gens(ctx, 8)
    try:
        return bpperm.DeckProver(g, k, deck).prove_batch(perms, seeds, gam, raw=True)
    finally:
        g.close()
        if own:
            ctx.close()


if __name__ == "__main__":
    p, v = prove()
    print("PROOFS", p.hex())
    print("V", v.hex())
