"""Cost of the circuit hints (bpp_circuit_create_hinted): what deriving a proof's
auxiliary values on the GPU costs against handing them over, and that the
feature costs the existing entry points nothing.

    python tools/circuit_hints_cost.py [--windows 7] [--parent-lib PATH] [--out profiles/circuit_hints_cost_ab.json]

(a) Hinted against supplied: in_range_many(16, 64) (BPP_CIRCUIT_LARGE, 1024
    gates, n_aux = 2048: 64 KB of hints per proof) and in_range(64) (64 gates,
    n_aux = 128), proved in 64-proof batches by one circuit handle -- aux == NULL
    (k_hint_aux derives the values) and aux = aux_of(v) prepared before any clock
    starts -- one process, one context, interleaved windows (hinted, supplied,
    hinted, ...).  proofs/s with medians and window spread; the "hint_aux" and
    "witness_program" stage times of one more batch each way (Context.profile);
    the bytes a batch stages and uploads ("prove_stage_bytes").  Reported, no
    threshold: nothing here had been measured before.
(b) What exists, against the parent commit's library (--parent-lib), in fresh
    child processes that alternate between the two libraries: part (c) of
    tools/circuit_large_cost.py, run as it stands -- bpp_perm_verify_batch,
    bpp_circuit_prove_batch with supplied inputs (two_half_shuffle(52)) and
    bpp_circuit_verify_batch_pub (shuffle_of_public(52)).  within_parent_spread:
    this library's median lies inside the min..max of the parent's own windows
    (or above it).

A tool, not part of bench.py; recorded, not gated.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_large_cost as clc  # noqa: E402  (stats, window, and part (c)'s child processes)

BATCH = 64


class Case:
    """One hinted circuit's marshalled inputs: BATCH proofs' v and aux_of(v),
    made before any clock starts; prove(hinted) is the raw C-ABI call."""

    def __init__(self, ctx, gens, circ, desc, rows, label=b"bp-perm"):
        import bpperm
        self.ctx, self.gens, self.circ, self.label = ctx, gens, circ, label
        self.lib, self.check = ctx.lib, bpperm.check
        sb = lambda x: x.to_bytes(32, "little")
        self.v = C.c_char_p(b"".join(sb(x) for v in rows for x in v))
        self.aux = C.c_char_p(b"".join(sb(x) for v in rows for x in desc.aux_of(v)))
        self.pf = C.create_string_buffer(circ.proof_len * BATCH)
        self.V = C.create_string_buffer(32 * circ.m * BATCH)

    def prove(self, hinted: bool):
        self.check(self.lib.bpp_circuit_prove_batch(self.ctx.h, self.gens.h, self.circ.h, BATCH, self.v,
                                                    None if hinted else self.aux, None, None, self.label,
                                                    len(self.label), self.pf, self.V),
                   "bpp_circuit_prove_batch", self.ctx.h)

    def one_batch(self, hinted: bool):
        """stage times (ms) and staged bytes of one profiled batch"""
        import bpperm
        self.ctx.profile(True)
        self.ctx.profile_reset()
        self.ctx.work_reset()
        self.prove(hinted)
        out = {}
        for s in ("hint_aux", "witness_program"):
            try:
                out[s + "_ms"] = round(self.ctx.profile_get(s)[0], 4)
            except bpperm.BppError:
                pass
        self.ctx.profile(False)
        v = C.c_uint64()
        self.check(self.lib.bpp_ctx_work_get(self.ctx.h, b"prove_stage_bytes", C.byref(v)), "bpp_ctx_work_get")
        out["staged_bytes"] = v.value
        return out


def hinted_vs_supplied(a, ctx, gens):
    import bpperm
    from bpperm import gadgets
    rnd = random.Random(6416)
    out = {"unit": "proofs/s", "shape": {"batch": BATCH, "batches_per_window": a.batches, "windows": a.windows},
           "order": "hinted, supplied, hinted, ... in one process on one context"}
    for name, desc, count, large in (("in_range_many(16, 64)", gadgets.in_range_many(16, 64), 16, True),
                                     ("in_range(64)", gadgets.in_range(64), 1, False)):
        rows = [[rnd.randrange(1 << 64) for _ in range(count)] for _ in range(BATCH)]
        circ = bpperm.Circuit(desc, large=large)
        assert circ.has_hints
        c = Case(ctx, gens, circ, desc, rows)
        for _ in range(3):
            c.prove(True)
            c.prove(False)
        runs = {"hinted": [], "supplied": []}
        for _ in range(a.windows):
            for side in runs:
                runs[side].append(clc.window(lambda: c.prove(side == "hinted"), a.batches, BATCH))
        h, s = clc.stats(runs["hinted"]), clc.stats(runs["supplied"])
        out[name] = {"n_gates": desc.n_gates, "n_aux": desc.n_aux, "n_p": circ.n_p, "Q": circ.Q,
                     "aux_bytes_per_proof": 32 * desc.n_aux, "hinted": h, "supplied": s,
                     "ratio": h["median"] / s["median"],
                     "hinted_spread": (h["max"] - h["min"]) / h["median"],
                     "supplied_spread": (s["max"] - s["min"]) / s["median"],
                     "one_batch": {"hinted": c.one_batch(True), "supplied": c.one_batch(False)}}
        circ.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batches", type=int, default=40, help="64-proof batches per window of part a")
    ap.add_argument("--prove-batches", type=int, default=100, help="384-proof batches per proving window of part b")
    ap.add_argument("--verify-calls", type=int, default=100, help="4096-proof calls per verifying window of part b")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libbpperm.so (part b; skipped without it)")
    ap.add_argument("--ab-rounds", type=int, default=2, help="processes per library in part b")
    ap.add_argument("--ab-windows", type=int, default=5, help="windows per process in part b")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: a, b")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    out = {}
    if "a" not in skip:
        import bpperm
        ctx = bpperm.Context(0)
        gens = bpperm.Gens(ctx, 1024)
        out["hinted_vs_supplied"] = hinted_vs_supplied(a, ctx, gens)
        gens.close()
        ctx.close()
    if a.parent_lib and "b" not in skip:
        b = argparse.Namespace(**vars(a))
        b.windows = a.ab_windows
        out["existing"] = clc.existing(b)
    brief = {}
    if "hinted_vs_supplied" in out:
        brief["hinted_vs_supplied"] = {
            n: {"hinted": round(v["hinted"]["median"], 1), "supplied": round(v["supplied"]["median"], 1),
                "ratio": round(v["ratio"], 3), "one_batch": v["one_batch"]}
            for n, v in out["hinted_vs_supplied"].items() if isinstance(v, dict) and "hinted" in v}
    if "existing" in out:
        brief["existing"] = {k: {q: out["existing"][k][q] for q in ("ratio", "parent_spread", "this_spread",
                                                                      "within_parent_spread")}
                             for k in ("verify", "prove", "verify_pub")}
    print(json.dumps(brief))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
