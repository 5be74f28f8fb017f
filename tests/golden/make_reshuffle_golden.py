"""Writes tests/golden/reshuffle.json from the reference helper
(tests/reshuffle_ref.py): input cards, permutation, seed, blinds, output cards
and proof of blind re-shuffles at k = 2, 3, 5 (supplied blinds at k = 3, the
identity among the cards at k = 5) and one at k = 52.  No GPU.

    python tests/golden/make_reshuffle_golden.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import reshuffle_ref as rr  # noqa: E402

# (k, label)
CASES = [(2, "bp-perm"), (3, "golden-reshuffle"), (5, "bp-perm"), (52, "bp-perm")]


def main():
    cases = []
    for k, label in CASES:
        tag = b"golden-%d" % k
        cards = rr.rand_cards(k, tag)
        if k == 5:
            cards[2] = rr.IDENTITY
        perm = {2: [1, 0], 3: [2, 0, 1]}.get(k) or rr.rand_perm(k, tag)  # (never the identity: pi and its inverse differ at k >= 3)
        assert perm != list(range(k))
        blinds = None
        if k == 3:
            blinds = [rr.rand_scalar(tag + b"-r%d" % i) for i in range(k)]
            blinds[1] = rr.L - 1
        seed = rr.seed32(tag)
        out, proof = rr.prove(cards, perm, seed, blinds, label.encode())
        assert rr.verify(cards, out, proof, label.encode())
        cases.append({"k": k, "label": label, "seed": seed.hex(), "perm": perm,
                      "blinds": [rr.sb(b).hex() for b in blinds] if blinds else None,
                      "cards_in": [c.hex() for c in cards], "cards_out": [c.hex() for c in out],
                      "proof": proof.hex()})
    path = Path(__file__).resolve().parent / "reshuffle.json"
    path.write_text(json.dumps({"cases": cases}, indent=1) + "\n")
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
