"""Child process of tests/test_gpu_circuit.py (a helper, not a test): proves the
fixed circuit batch of circuit_case() under whatever BPP_* switches the parent
put in the environment and prints the proofs and V as one hex line each."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_ref as cr  # noqa: E402


def circuit_case(n=5):
    """in_range(3): free sides, aux and supplied blindings in one batch."""
    desc = cr.satisfying("range3", 0)[0]
    v = [[(3 * i + 1) % 8] for i in range(n)]
    aux = [desc.aux_of(x) for x in v]
    seeds = b"".join(cr.seed32(b"circuit-child-%d" % i) for i in range(n))
    gam = [[cr.rand_scalar(b"circuit-child-g-%d" % i)] for i in range(n)]
    return desc, v, aux, seeds, gam


def prove(ctx=None):
    import bpperm
    desc, v, aux, seeds, gam = circuit_case()
    own = ctx is None
    if own:
        ctx = bpperm.Context(0)
    g = bpperm.Gens(ctx, 8)
    try:
        enc = lambda rows: [[cr.sb(x) for x in row] for row in rows]
        return bpperm.CircuitProver(g, desc).prove_batch(enc(v), enc(aux), seeds, enc(gam), raw=True)
    finally:
        g.close()
        if own:
            ctx.close()


if __name__ == "__main__":
    p, v = prove()
    print("PROOFS", p.hex())
    print("V", v.hex())
