"""Cost of a caller-defined circuit (bpp_circuit_*) against the built-in
statement it restates: two_half_shuffle(52) through bpp_circuit_prove_batch /
bpp_circuit_verify_batch against bpp_perm_prove_shuffle_batch /
bpp_perm_verify_batch at 52 cards -- the same statement, n_p and m, so the only
differences are the interpreted witness (k_witness_program for k_witness_cards),
k_v_inputs' arguments (v as it stands, for cards and cards[perm]) and the
"circuit" digest in the transcript.

    python tools/circuit_cost.py [--windows 5] [--out profiles/circuit_cost_ab.json]

One process, one context, both sides through the C ABI with buffers marshalled
before the clock starts, in interleaved timing windows (yardstick, circuit,
yardstick, circuit, ...): proving in 384-proof batches one at a time (drawn
blindings), verifying 4096 proofs per call.  Reports both rates per side, their
ratio (circuit / yardstick, of the window medians), the windows' spread (min ..
max), and the witness kernels' stage times (witness_cards, witness_program)
with the rest of the context's stage profile of one more batch of each kind.
A tool, not part of bench.py; recorded, not gated.
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
STAGES = ("witness_cards", "witness_program", "pb_rng", "pb_pedersen_V", "pb_pedersen_Vx_witness", "pb_msm_AI_AO_S",
          "pb_host_poly", "pb_pedersen_T_lr", "pb_ipa", "verify_upload", "verify_replay_dev", "verify_decompress",
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
    from bpperm import check, gadgets

    ctx = bpperm.Context(0)
    gens = bpperm.Gens(ctx, GENS)
    lib, label = ctx.lib, b"bp-perm"
    rnd = random.Random(52)
    circ = bpperm.Circuit(gadgets.two_half_shuffle(K))

    deck = [i.to_bytes(32, "little") for i in range(1, K + 1)]
    flat, vals = [], []
    for _ in range(NV):
        p = list(range(K))
        rnd.shuffle(p)
        flat += p
        vals.append(b"".join(deck) + b"".join(deck[i] for i in p))
    pm = (C.c_uint32 * (NV * K))(*flat)
    cbuf = C.c_char_p(b"".join(deck) * NV)
    vbuf = C.c_char_p(b"".join(vals))  # the circuit's v = cards then cards[perm], the same statement
    plen, m = lib.bpp_perm_proof_len(K), 2 * K + 1
    assert circ.proof_len == plen and circ.m == m
    two_pf, two_V = C.create_string_buffer(plen * NV), C.create_string_buffer(32 * m * NV)
    cir_pf, cir_V = C.create_string_buffer(plen * NV), C.create_string_buffer(32 * m * NV)

    def prove_two(n):
        check(lib.bpp_perm_prove_shuffle_batch(ctx.h, gens.h, K, n, cbuf, pm, None, None, label, len(label), two_pf,
                                               two_V), "bpp_perm_prove_shuffle_batch", ctx.h)

    def prove_cir(n):
        check(lib.bpp_circuit_prove_batch(ctx.h, gens.h, circ.h, n, vbuf, None, None, None, label, len(label), cir_pf,
                                          cir_V), "bpp_circuit_prove_batch", ctx.h)

    def verify_two():
        check(lib.bpp_perm_verify_batch(ctx.h, gens.h, K, NV, label, len(label), two_pf, two_V),
              "bpp_perm_verify_batch", ctx.h)

    def verify_cir():
        check(lib.bpp_circuit_verify_batch(ctx.h, gens.h, circ.h, NV, label, len(label), cir_pf, cir_V),
              "bpp_circuit_verify_batch", ctx.h)

    def window(f, reps, per):
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        return reps * per / (time.perf_counter() - t0)

    for _ in range(2):  # warmup: window tables, workspaces
        prove_two(B)
        prove_cir(B)
    runs = {"prove_two_half": [], "prove_circuit": [], "verify_two_half": [], "verify_circuit": []}
    for _ in range(a.windows):
        runs["prove_two_half"].append(window(lambda: prove_two(B), a.prove_batches, B))
        runs["prove_circuit"].append(window(lambda: prove_cir(B), a.prove_batches, B))
    prove_two(NV)  # the verifiers' inputs
    prove_cir(NV)
    verify_two()
    verify_cir()
    for _ in range(a.windows):
        runs["verify_two_half"].append(window(verify_two, a.verify_calls, NV))
        runs["verify_circuit"].append(window(verify_cir, a.verify_calls, NV))

    out = {"shape": {"cards": K, "prove_batch": B, "verify_proofs": NV, "windows": a.windows,
                     "prove_batches_per_window": a.prove_batches, "verify_calls_per_window": a.verify_calls},
           "unit": "proofs/s", "yardstick": "bpp_perm_prove_shuffle_batch / bpp_perm_verify_batch, same process, "
                                            "interleaved windows",
           "circuit": {"gadget": "two_half_shuffle(52)", "n_p": circ.n_p, "Q": circ.Q, "m": circ.m,
                       "proof_bytes": circ.proof_len}}
    for side in ("prove", "verify"):
        y, c = stats(runs[side + "_two_half"]), stats(runs[side + "_circuit"])
        out[side] = {"two_half": y, "circuit": c, "ratio": c["median"] / y["median"],
                     "within_spread": c["max"] >= y["min"] and y["max"] >= c["min"]}
    prof = {}
    for name, f in (("two_half", lambda: (prove_two(B), verify_two())), ("circuit", lambda: (prove_cir(B), verify_cir()))):
        ctx.profile(True)
        ctx.profile_reset()
        f()
        prof[name] = {}
        for s in STAGES:
            try:
                prof[name][s] = round(ctx.profile_get(s)[0], 4)
            except bpperm.BppError:  # a stage this batch did not run
                pass
        ctx.profile(False)
    out["stage_profile_ms"] = prof
    print(json.dumps({k: ({kk: vv for kk, vv in out[k].items() if kk in ("ratio", "within_spread")} |
                          {s: {q: round(out[k][s][q]) for q in ("median", "min", "max")} for s in ("two_half", "circuit")})
                      for k in ("prove", "verify")} |
                     {"witness_ms_per_384": {"witness_cards": prof["two_half"].get("witness_cards"),
                                             "witness_program": prof["circuit"].get("witness_program")}}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    circ.close()
    gens.close()
    ctx.close()


if __name__ == "__main__":
    main()
