"""Child process of tests/test_gpu_circuit_pub.py (a helper, not a test): proves
the fixed public-input batch of circuit_case() under whatever BPP_* switches the
parent put in the environment and prints the proofs and V as one hex line each."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_pub_ref as cp  # noqa: E402


def circuit_case(n=5):
    """shuffle_of_public(3): five proofs over five decks, supplied blindings."""
    got = [cp.satisfying("shufflepub3", i) for i in range(n)]
    desc = got[0][0]
    seeds = b"".join(cp.seed32(b"circuit-pub-child-%d" % i) for i in range(n))
    gam = [[cp.rand_scalar(b"circuit-pub-child-g-%d-%d" % (i, j)) for j in range(desc.m_in)] for i in range(n)]
    return desc, [g[1] for g in got], [g[3] for g in got], seeds, gam


def prove(ctx=None):
    import bpperm
    desc, v, pub, seeds, gam = circuit_case()
    own = ctx is None
    if own:
        ctx = bpperm.Context(0)
    g = bpperm.Gens(ctx, 8)
    try:
        enc = lambda rows: [[cp.sb(x) for x in row] for row in rows]
        return bpperm.CircuitProver(g, desc).prove_batch(enc(v), None, seeds, enc(gam), raw=True, pub=enc(pub))
    finally:
        g.close()
        if own:
            ctx.close()


if __name__ == "__main__":
    p, v = prove()
    print("PROOFS", p.hex())
    print("V", v.hex())
