"""Generate tests/golden/deck.json from the public-deck reference
(tests/deck_ref.py, built from the CPU oracle's pieces).

    python tests/golden/make_deck_golden.py

Two cases, each one call of bpp_deck_prove_batch: 2 proofs at k = 52 over the
default deck 1..52 with drawn blindings, and 1 proof at k = 9 over an edge deck
(0, l - 1, 252-bit cards) with supplied blindings.  Every proof is verified by
the reference before it is written.  k = 52 takes minutes in pure Python, which
is why the tests read the file instead.
"""
import json
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import deck_ref as dr  # noqa: E402
import shuffle_ref as sr  # noqa: E402


def case(k, deck, nproofs, with_gammas, tag):
    label = b"bp-perm"
    d = deck if deck is not None else dr.default_deck(k)
    perms = [sr.rand_perm(k, b"deck-golden-%s-%d" % (tag, i)) for i in range(nproofs)]
    seeds = [sr.seed32(b"deck-golden-%s-%d" % (tag, i)) for i in range(nproofs)]
    gammas = None
    if with_gammas:
        gammas = [[sr.rand_scalar(b"deck-golden-g-%s-%d-%d" % (tag, i, j)) for j in range(k)] for i in range(nproofs)]
    proofs, Vs = [], []
    for i in range(nproofs):
        pf = dr.prove_deck(d, perms[i], seeds[i], gammas[i] if gammas else None, label=label)
        assert dr.verify_deck(d, pf, label=label)
        proofs.append(pf.to_bytes().hex())
        Vs.append([v.hex() for v in pf.V])
    return {"k": k, "label": label.decode(),
            "deck": None if deck is None else [sr.scalar_bytes(c).hex() for c in deck],
            "perms": perms, "seeds": [s.hex() for s in seeds],
            "gammas": None if gammas is None else [[sr.scalar_bytes(g).hex() for g in row] for row in gammas],
            "proofs": proofs, "V": Vs}


if __name__ == "__main__":
    t = time.time()
    cases = [case(52, None, 2, False, b"k52"), case(9, sr.edge_decks(9)[0], 1, True, b"k9")]
    out = {"generator": "tests/golden/make_deck_golden.py", "cases": cases, "oracle_seconds": time.time() - t}
    (HERE / "deck.json").write_text(json.dumps(out, indent=1))
    print("wrote", HERE / "deck.json", out["oracle_seconds"])
