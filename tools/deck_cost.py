"""Cost of the public-deck shuffle proof (bpp_deck_*) against the statement it
replaces for a first shuffle, the two-half proof of a caller's shuffle
(bpp_perm_prove_shuffle_batch / bpp_perm_verify_batch), at 52 cards.

    python tools/deck_cost.py [--windows 5] [--out profiles/deck_cost_ab.json]

One process, one context, both sides through the C ABI with buffers marshalled
before the clock starts, in interleaved timing windows (yardstick, deck,
yardstick, deck, ...): proving in 384-proof batches one at a time (default
deck, drawn blindings), verifying 4096 proofs per call.  Reports both rates per
side, their ratio (deck / yardstick, of the window medians) and the windows'
spread (min .. max); where a side is not faster than its yardstick beyond that
spread, the context's stage profile of one more batch of each kind is added.
A tool, not part of bench.py; no threshold: the feature is the statement.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import random
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))

K, B, NV, GENS = 52, 384, 4096, 128
STAGES = ("pb_rng", "pb_pedersen_V", "pb_pedersen_Vx_witness", "pb_msm_AI_AO_S", "pb_host_poly", "pb_pedersen_T_lr",
          "pb_ipa", "verify_upload", "verify_replay", "verify_terms", "verify_replay_dev", "verify_decompress",
          "verify_scalars", "poly_coef", "poly_x")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "windows": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--prove-batches", type=int, default=200, help="batches per proving window (about 1 s)")
    ap.add_argument("--verify-calls", type=int, default=600, help="calls per verifying window (about 1 s)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bpperm
    from bpperm import check

    ctx = bpperm.Context(0)
    gens = bpperm.Gens(ctx, GENS)
    lib, label = ctx.lib, b"bp-perm"
    rnd = random.Random(52)

    def perms(n):
        flat = []
        for _ in range(n):
            p = list(range(K))
            rnd.shuffle(p)
            flat += p
        return (C.c_uint32 * (n * K))(*flat)

    cards = b"".join(b"".join(i.to_bytes(32, "little") for i in range(1, K + 1)) for _ in range(NV))
    pm = perms(NV)
    two_len, deck_len = lib.bpp_perm_proof_len(K), lib.bpp_deck_proof_len(K)
    two_pf, two_V = C.create_string_buffer(two_len * NV), C.create_string_buffer(32 * (2 * K + 1) * NV)
    deck_pf, deck_V = C.create_string_buffer(deck_len * NV), C.create_string_buffer(32 * (K + 1) * NV)
    cbuf = C.c_char_p(cards)

    def prove_two(n):
        check(lib.bpp_perm_prove_shuffle_batch(ctx.h, gens.h, K, n, cbuf, pm, None, None, label, len(label), two_pf,
                                               two_V), "bpp_perm_prove_shuffle_batch", ctx.h)

    def prove_deck(n):
        check(lib.bpp_deck_prove_batch(ctx.h, gens.h, K, n, None, pm, None, None, label, len(label), deck_pf, deck_V),
              "bpp_deck_prove_batch", ctx.h)

    def verify_two():
        check(lib.bpp_perm_verify_batch(ctx.h, gens.h, K, NV, label, len(label), two_pf, two_V),
              "bpp_perm_verify_batch", ctx.h)

    def verify_deck():
        check(lib.bpp_deck_verify_batch(ctx.h, gens.h, K, NV, None, label, len(label), deck_pf, deck_V),
              "bpp_deck_verify_batch", ctx.h)

    def window(f, reps, per):
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        return reps * per / (time.perf_counter() - t0)

    for _ in range(2):  # warmup: window tables, workspaces
        prove_two(B)
        prove_deck(B)
    runs = {"prove_two_half": [], "prove_deck": [], "verify_two_half": [], "verify_deck": []}
    for _ in range(a.windows):
        runs["prove_two_half"].append(window(lambda: prove_two(B), a.prove_batches, B))
        runs["prove_deck"].append(window(lambda: prove_deck(B), a.prove_batches, B))
    prove_two(NV)  # the verifiers' inputs
    prove_deck(NV)
    verify_two()
    verify_deck()
    for _ in range(a.windows):
        runs["verify_two_half"].append(window(verify_two, a.verify_calls, NV))
        runs["verify_deck"].append(window(verify_deck, a.verify_calls, NV))

    out = {"shape": {"cards": K, "prove_batch": B, "verify_proofs": NV, "windows": a.windows,
                     "prove_batches_per_window": a.prove_batches, "verify_calls_per_window": a.verify_calls},
           "unit": "proofs/s", "yardstick": "bpp_perm_prove_shuffle_batch / bpp_perm_verify_batch, same process, "
                                            "interleaved windows",
           "proof_bytes": {"two_half": two_len, "deck": deck_len}}
    for side in ("prove", "verify"):
        y, d = stats(runs[side + "_two_half"]), stats(runs[side + "_deck"])
        out[side] = {"two_half": y, "deck": d, "ratio": d["median"] / y["median"],
                     "faster_beyond_spread": d["min"] > y["max"]}
    if not (out["prove"]["faster_beyond_spread"] and out["verify"]["faster_beyond_spread"]):
        prof = {}
        for name, f in (("two_half", lambda: (prove_two(B), verify_two())), ("deck", lambda: (prove_deck(B), verify_deck()))):
            ctx.profile(True)
            ctx.profile_reset()
            f()
            prof[name] = {}
            for s in STAGES:
                try:
                    prof[name][s] = round(ctx.profile_get(s)[0], 4)
                except bpperm.BppError:  # a stage this build does not name
                    pass
            ctx.profile(False)
        out["stage_profile_ms"] = prof
    print(json.dumps({k: ({kk: vv for kk, vv in out[k].items() if kk in ("ratio", "faster_beyond_spread")} |
                          {s: {q: round(out[k][s][q]) for q in ("median", "min", "max")} for s in ("two_half", "deck")})
                      for k in ("prove", "verify")}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    gens.close()
    ctx.close()


if __name__ == "__main__":
    main()
