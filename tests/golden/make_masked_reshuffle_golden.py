"""Writes tests/golden/masked_reshuffle.json from the reference helper
(tests/masked_reshuffle_ref.py): key, input cards, permutation, seed, blinds,
output cards and proof of masked re-shuffles at k = 3 (supplied blinds, the open
deck) and k = 52.  No GPU.

    python tests/golden/make_masked_reshuffle_golden.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import masked_reshuffle_ref as mr  # noqa: E402

# (k, label)
CASES = [(3, "golden-masked"), (52, "bp-perm")]


def main():
    cases = []
    for k, label in CASES:
        tag = b"golden-%d" % k
        key = mr.key_of(mr.rand_scalar(tag + b"-sk"))
        cards = mr.rand_cards(k, tag)
        perm = {3: [2, 0, 1]}.get(k) or mr.rand_perm(k, tag)
        assert perm != list(range(k))
        blinds = None
        if k == 3:
            cards = mr.open_deck([c[32:] for c in cards])
            blinds = [mr.rand_scalar(tag + b"-r%d" % i) for i in range(k)]
            blinds[1] = mr.L - 1
        seed = mr.seed32(tag)
        out, proof = mr.prove(key, cards, perm, seed, blinds, label.encode())
        assert mr.verify(key, cards, out, proof, label.encode())
        cases.append({"k": k, "label": label, "key": key.hex(), "seed": seed.hex(), "perm": perm,
                      "blinds": [mr.sb(b).hex() for b in blinds] if blinds else None,
                      "cards_in": [c.hex() for c in cards], "cards_out": [c.hex() for c in out],
                      "proof": proof.hex()})
    path = Path(__file__).resolve().parent / "masked_reshuffle.json"
    path.write_text(json.dumps({"cases": cases}, indent=1) + "\n")
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
