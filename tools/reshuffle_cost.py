"""Cost of the blind re-shuffle proof (bpp_reshuffle_*) against its inner proof
alone, the shuffle_of_public(52) circuit through bpp_circuit_prove_batch_pub /
bpp_circuit_verify_batch_pub, at 52 cards.

    python tools/reshuffle_cost.py [--windows 5] [--out profiles/reshuffle_cost_ab.json]

One process, one context, both sides through the C ABI with buffers marshalled
before the clock starts, in interleaved timing windows (circuit, reshuffle,
circuit, reshuffle, ...): proving in 384-proof batches one at a time, verifying
4096 proofs per call.  The yardstick is the proof the re-shuffle carries inside,
so the ratio (reshuffle / circuit, of the window medians) is the cost of the
new argument: the commitments A, E, T_i, T_S, three transcript phases and the
responses when proving; the decompression of 5k + 1 points, D_i = y A_i + E_i
and one more MSM of 4k + 1 points per proof when verifying.  The context's stage
profile of one batch of each kind is added.  A tool, not part of bench.py; no
threshold: a finding.
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
L = 2**252 + 27742317777372353535851937790883648493
STAGES = ("rs_draws", "rs_outputs", "rs_transcript", "rs_exponents", "rs_tsum_mul", "rs_tsum_sum", "rs_responses", "rs_D",
          "rs_weights", "rs_sigma_terms", "rs_sigma_sums", "rs_sigma_merge", "decompress", "pedersen", "compress", "msm_horner", "pb_rng", "pb_pedersen_V",
          "pb_pedersen_Vx_witness", "pb_msm_AI_AO_S", "pb_host_poly", "pb_pedersen_T_lr", "pb_ipa", "verify_upload",
          "verify_replay_dev", "verify_terms", "verify_decompress", "verify_scalars")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "windows": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--prove-batches", type=int, default=40, help="batches per proving window")
    ap.add_argument("--verify-calls", type=int, default=20, help="calls per verifying window")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bpperm
    from bpperm import check, gadgets as gd

    ctx = bpperm.Context(0)
    gens = bpperm.Gens(ctx, GENS)
    lib, label = ctx.lib, b"bp-perm"
    rnd = random.Random(52)
    sb = lambda x: (x % L).to_bytes(32, "little")

    flat = []
    for _ in range(NV):
        p = list(range(K))
        rnd.shuffle(p)
        flat += p
    pm = (C.c_uint32 * (NV * K))(*flat)
    # the re-shuffle's inputs: NV decks of K commitments nobody here opens
    cards = b"".join(gens.pedersen_commit([sb(rnd.randrange(L)) for _ in range(NV * K)],
                                          [sb(rnd.randrange(L)) for _ in range(NV * K)]))
    rs_len = lib.bpp_reshuffle_proof_len(K)
    rs_out, rs_pf = C.create_string_buffer(32 * K * NV), C.create_string_buffer(rs_len * NV)
    # the yardstick's: NV decks of K scalars, public, and their permutations, committed
    circ = bpperm.Circuit(gd.shuffle_of_public(K))
    deck = [[rnd.randrange(L) for _ in range(K)] for _ in range(NV)]
    pub = b"".join(sb(x) for d in deck for x in d)
    vals = b"".join(sb(deck[p][flat[p * K + i]]) for p in range(NV) for i in range(K))
    c_len = circ.proof_len
    c_pf, c_V = C.create_string_buffer(c_len * NV), C.create_string_buffer(32 * (K + 1) * NV)
    cbuf, pbuf, vbuf = C.c_char_p(cards), C.c_char_p(pub), C.c_char_p(vals)

    def prove_rs(n):
        check(lib.bpp_reshuffle_prove_batch(ctx.h, gens.h, K, n, cbuf, pm, None, None, label, len(label), rs_out, rs_pf),
              "bpp_reshuffle_prove_batch", ctx.h)

    def prove_c(n):
        check(lib.bpp_circuit_prove_batch_pub(ctx.h, gens.h, circ.h, n, vbuf, None, pbuf, None, None, label, len(label),
                                              c_pf, c_V), "bpp_circuit_prove_batch_pub", ctx.h)

    def verify_rs():
        check(lib.bpp_reshuffle_verify_batch(ctx.h, gens.h, K, NV, label, len(label), cbuf, rs_out, rs_pf),
              "bpp_reshuffle_verify_batch", ctx.h)

    def verify_c():
        check(lib.bpp_circuit_verify_batch_pub(ctx.h, gens.h, circ.h, NV, label, len(label), c_pf, c_V, pbuf),
              "bpp_circuit_verify_batch_pub", ctx.h)

    def window(f, reps, per):
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        return reps * per / (time.perf_counter() - t0)

    for _ in range(2):  # warmup: window tables, workspaces
        prove_c(B)
        prove_rs(B)
    runs = {"prove_circuit": [], "prove_reshuffle": [], "verify_circuit": [], "verify_reshuffle": []}
    for _ in range(a.windows):
        runs["prove_circuit"].append(window(lambda: prove_c(B), a.prove_batches, B))
        runs["prove_reshuffle"].append(window(lambda: prove_rs(B), a.prove_batches, B))
    prove_c(NV)  # the verifiers' inputs
    prove_rs(NV)
    verify_c()
    verify_rs()
    for _ in range(a.windows):
        runs["verify_circuit"].append(window(verify_c, a.verify_calls, NV))
        runs["verify_reshuffle"].append(window(verify_rs, a.verify_calls, NV))

    out = {"shape": {"cards": K, "prove_batch": B, "verify_proofs": NV, "windows": a.windows,
                     "prove_batches_per_window": a.prove_batches, "verify_calls_per_window": a.verify_calls},
           "unit": "proofs/s",
           "yardstick": "bpp_circuit_prove_batch_pub / bpp_circuit_verify_batch_pub on shuffle_of_public(52), same "
                        "process, interleaved windows",
           "proof_bytes": {"circuit": c_len, "reshuffle": rs_len}}
    for side in ("prove", "verify"):
        y, d = stats(runs[side + "_circuit"]), stats(runs[side + "_reshuffle"])
        out[side] = {"circuit": y, "reshuffle": d, "ratio": d["median"] / y["median"]}
    prof = {}
    for name, f in (("circuit", lambda: (prove_c(B), verify_c())), ("reshuffle", lambda: (prove_rs(B), verify_rs()))):
        ctx.profile(True)
        ctx.profile_reset()
        f()
        prof[name] = {}
        for s in STAGES:
            try:
                prof[name][s] = round(ctx.profile_get(s)[0], 4)
            except bpperm.BppError:  # a stage this run did not pass
                pass
        ctx.profile(False)
    out["stage_profile_ms"] = prof
    print(json.dumps({k: {"ratio": round(out[k]["ratio"], 4)} |
                      {s: {q: round(out[k][s][q]) for q in ("median", "min", "max")} for s in ("circuit", "reshuffle")}
                      for k in ("prove", "verify")}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    circ.close()
    gens.close()
    ctx.close()


if __name__ == "__main__":
    main()
