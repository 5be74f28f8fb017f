"""Writes tests/golden/circuit_pub.json from the reference helper
(tests/circuit_pub_ref.py): inputs, public inputs, proofs and V of three
circuits with public inputs -- opens_to, member_of_public(13) and
shuffle_of_public(5) -- two proofs each, fixed seeds, supplied blindings.  No GPU.

    python tests/golden/make_circuit_pub_golden.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import circuit_pub_ref as cp  # noqa: E402

# (case of circuit_pub_ref.satisfying, label)
CASES = [("opens", "bp-perm"), ("memberpub13", "golden-circuit-pub"), ("shufflepub5", "bp-perm")]


def main():
    cases = []
    for name, label in CASES:
        desc = cp.satisfying(name, 0)[0]
        case = {"name": name, "label": label, "digest": cp.circuit_digest(desc).hex(), "v": [], "pub": [],
                "gammas": [], "seeds": [], "proofs": [], "V": []}
        for p in range(2):
            _, v, aux, pub = cp.satisfying(name, p)
            assert not aux
            gam = [cp.rand_scalar(b"golden-pub-g-%s-%d-%d" % (name.encode(), p, j)) for j in range(desc.m_in)]
            if p == 1:
                gam[0] = cp.L - 1
            seed = cp.seed32(b"golden-pub-%s-%d" % (name.encode(), p))
            pf = cp.prove_circuit(desc, v, aux, pub, seed, gam, label=label.encode())
            assert cp.verify_circuit(desc, pf, pub, label=label.encode())
            case["v"].append([cp.sb(x).hex() for x in v])
            case["pub"].append([cp.sb(x).hex() for x in pub])
            case["gammas"].append([cp.sb(g).hex() for g in gam])
            case["seeds"].append(seed.hex())
            case["proofs"].append(pf.to_bytes().hex())
            case["V"].append([e.hex() for e in pf.V])
        cases.append(case)
    out = ROOT / "tests" / "golden" / "circuit_pub.json"
    out.write_text(json.dumps({"cases": cases}, indent=1) + "\n")
    print(out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
