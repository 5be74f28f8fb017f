"""Writes tests/golden/circuit.json from the reference helper
(tests/circuit_ref.py): inputs, proofs and V of four small caller-defined
circuits, two proofs each.  No GPU.

    python tools/gen_circuit_golden.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import circuit_ref as cr  # noqa: E402

# (case of circuit_ref.satisfying, supplied blindings?, label)
CASES = [("member2", False, "bp-perm"), ("twohalf2", True, "bp-perm"), ("range3", True, "golden-circuit"),
         ("heavy", False, "bp-perm")]


def main():
    cases = []
    for name, with_gammas, label in CASES:
        desc = cr.satisfying(name, 0)[0]
        case = {"name": name, "label": label, "digest": cr.circuit_digest(desc).hex(), "v": [], "aux": [],
                "gammas": [] if with_gammas else None, "seeds": [], "proofs": [], "V": []}
        for p in range(2):
            _, v, aux = cr.satisfying(name, p)
            gam = None
            if with_gammas:
                gam = [cr.rand_scalar(b"golden-g-%s-%d-%d" % (name.encode(), p, j)) for j in range(desc.m_in)]
                if p == 1:
                    gam[0] = cr.L - 1
                case["gammas"].append([cr.sb(g).hex() for g in gam])
            seed = cr.seed32(b"golden-%s-%d" % (name.encode(), p))
            pf = cr.prove_circuit(desc, v, aux, seed, gam, label=label.encode())
            assert cr.verify_circuit(desc, pf, label=label.encode())
            case["v"].append([cr.sb(x).hex() for x in v])
            case["aux"].append([cr.sb(x).hex() for x in aux])
            case["seeds"].append(seed.hex())
            case["proofs"].append(pf.to_bytes().hex())
            case["V"].append([e.hex() for e in pf.V])
        cases.append(case)
    out = ROOT / "tests" / "golden" / "circuit.json"
    out.write_text(json.dumps({"cases": cases}, indent=1) + "\n")
    print(out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
