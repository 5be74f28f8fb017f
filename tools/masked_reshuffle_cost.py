"""Cost of the masked re-shuffle proof (bpp_masked_reshuffle_*) against the blind
re-shuffle it widens (bpp_reshuffle_*), at 52 cards, and -- with --ab-tree -- the
existing entry points of this checkout against another built checkout.

    python tools/masked_reshuffle_cost.py [--windows 3] [--ab-tree OTHER/bulletproof-perm_amd]
                                          [--out profiles/masked_reshuffle_cost_ab.json]

One process, one context, both sides through the C ABI with buffers marshalled
before the clock starts, in interleaved timing windows (plain, masked, plain,
masked, ...): proving in 384-proof batches one at a time, verifying 4096 proofs
per call.  The ratio (masked / plain, of the window medians) is the cost of the
second group element per card: two more constant-time 253-bit walks per card
when proving (r_i K and t_i W'_i beside t_i U'_i), 6k + 2 instead of 4k + 1 MSM
terms and 7k + 2 instead of 5k + 1 decoded points per proof when verifying, with
the D_i step and the inner proof the same.  The context's stage profile of one
batch of each kind is added.

--ab-tree: bpp_reshuffle_verify_batch, bpp_reshuffle_prove_batch,
bpp_perm_verify_batch and bpp_circuit_verify_batch_pub on the same shapes, this
checkout's library and the other one's in alternating child processes (each
imports its own checkout's package), --windows windows each per process; the ratio of the medians is
reported beside the other library's own window spread, inside which it should
lie.  A tool, not part of bench.py; no threshold: a finding.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import random
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

K, B, NV, GENS = 52, 384, 4096, 128
L = 2**252 + 27742317777372353535851937790883648493
STAGES = ("rs_draws", "rs_outputs", "rs_transcript", "rs_exponents", "rs_tsum_mul", "rs_tsum_sum", "rs_responses", "rs_D",
          "rs_weights", "rs_sigma_terms", "rs_sigma_sums", "rs_sigma_merge", "mrs_key_mul", "mrs_outputs", "mrs_tsum_mul",
          "mrs_tsum_sum", "mrs_D", "mrs_sigma_terms", "mrs_sigma_sums", "mrs_sigma_merge", "decompress", "pedersen",
          "compress", "msm_horner", "pb_rng", "pb_pedersen_V", "pb_pedersen_Vx_witness", "pb_msm_AI_AO_S", "pb_host_poly",
          "pb_pedersen_T_lr", "pb_ipa", "verify_upload", "verify_replay_dev", "verify_terms", "verify_decompress",
          "verify_scalars")
AB_ENTRIES = ("reshuffle_verify", "reshuffle_prove", "perm_verify", "circuit_verify_pub")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "windows": v}


def window(f, reps, per):
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return reps * per / (time.perf_counter() - t0)


def sb(x):
    return (x % L).to_bytes(32, "little")


class Shapes:
    """The buffers of every side, marshalled once."""

    def __init__(self, masked: bool = True):
        import bpperm
        self.bpperm = bpperm
        self.ctx = bpperm.Context(0)
        self.gens = bpperm.Gens(self.ctx, GENS)
        self.lib, self.label = self.ctx.lib, b"bp-perm"
        rnd = self.rnd = random.Random(52)
        flat = []
        for _ in range(NV):
            p = list(range(K))
            rnd.shuffle(p)
            flat += p
        self.flat = flat
        self.pm = (C.c_uint32 * (NV * K))(*flat)
        # points nobody here opens: NV decks of K commitments (the plain cards), and as many again (the W halves)
        pts = self.gens.pedersen_commit([sb(rnd.randrange(L)) for _ in range((2 if masked else 1) * NV * K)],
                                        [sb(rnd.randrange(L)) for _ in range((2 if masked else 1) * NV * K)])
        self.cards = C.c_char_p(b"".join(pts[:NV * K]))
        self.rs_len = self.lib.bpp_reshuffle_proof_len(K)
        self.rs_out, self.rs_pf = C.create_string_buffer(32 * K * NV), C.create_string_buffer(self.rs_len * NV)
        if masked:
            self.mcards = C.c_char_p(b"".join(pts))  # (consecutive points pair up as U | W)
            self.key = self.gens.pedersen_commit([sb(rnd.randrange(L))], [sb(0)])[0]
            self.m_len = self.lib.bpp_masked_reshuffle_proof_len(K)
            self.m_out, self.m_pf = C.create_string_buffer(64 * K * NV), C.create_string_buffer(self.m_len * NV)

    def prove_rs(self, n):
        self.bpperm.check(self.lib.bpp_reshuffle_prove_batch(self.ctx.h, self.gens.h, K, n, self.cards, self.pm, None, None,
                                                             self.label, len(self.label), self.rs_out, self.rs_pf),
                          "bpp_reshuffle_prove_batch", self.ctx.h)

    def verify_rs(self):
        self.bpperm.check(self.lib.bpp_reshuffle_verify_batch(self.ctx.h, self.gens.h, K, NV, self.label, len(self.label),
                                                              self.cards, self.rs_out, self.rs_pf),
                          "bpp_reshuffle_verify_batch", self.ctx.h)

    def prove_m(self, n):
        self.bpperm.check(self.lib.bpp_masked_reshuffle_prove_batch(self.ctx.h, self.gens.h, K, n, self.key, self.mcards,
                                                                    self.pm, None, None, self.label, len(self.label),
                                                                    self.m_out, self.m_pf),
                          "bpp_masked_reshuffle_prove_batch", self.ctx.h)

    def verify_m(self):
        self.bpperm.check(self.lib.bpp_masked_reshuffle_verify_batch(self.ctx.h, self.gens.h, K, NV, self.key, self.label,
                                                                     len(self.label), self.mcards, self.m_out,
                                                                     self.m_pf),
                          "bpp_masked_reshuffle_verify_batch", self.ctx.h)

    def close(self):
        self.gens.close()
        self.ctx.close()


def child(entry: str, windows: int, prove_batches: int, verify_calls: int):
    """One existing entry point in this process's library: its windows, as JSON."""
    import bpperm
    from bpperm import check, gadgets as gd
    s = Shapes(masked=False)
    lib, ctx, gens, label = s.lib, s.ctx, s.gens, s.label
    if entry == "reshuffle_prove":
        f, reps, per = (lambda: s.prove_rs(B)), prove_batches, B
    elif entry == "reshuffle_verify":
        s.prove_rs(NV)
        f, reps, per = s.verify_rs, verify_calls, NV
    elif entry == "perm_verify":
        pb = C.create_string_buffer(lib.bpp_perm_proof_len(K) * NV)
        vb = C.create_string_buffer(32 * (2 * K + 1) * NV)
        sd = (C.c_uint64 * NV)(*range(1, NV + 1))
        check(lib.bpp_perm_prove_batch(ctx.h, gens.h, K, NV, sd, label, len(label), pb, vb), "bpp_perm_prove_batch", ctx.h)
        f = lambda: check(lib.bpp_perm_verify_batch(ctx.h, gens.h, K, NV, label, len(label), pb, vb),
                          "bpp_perm_verify_batch", ctx.h)
        reps, per = verify_calls, NV
    elif entry == "circuit_verify_pub":
        circ = bpperm.Circuit(gd.shuffle_of_public(K))
        deck = [[s.rnd.randrange(L) for _ in range(K)] for _ in range(NV)]
        pub = C.c_char_p(b"".join(sb(x) for d in deck for x in d))
        vals = C.c_char_p(b"".join(sb(deck[p][s.flat[p * K + i]]) for p in range(NV) for i in range(K)))
        c_pf, c_V = C.create_string_buffer(circ.proof_len * NV), C.create_string_buffer(32 * (K + 1) * NV)
        check(lib.bpp_circuit_prove_batch_pub(ctx.h, gens.h, circ.h, NV, vals, None, pub, None, None, label, len(label),
                                              c_pf, c_V), "bpp_circuit_prove_batch_pub", ctx.h)
        f = lambda: check(lib.bpp_circuit_verify_batch_pub(ctx.h, gens.h, circ.h, NV, label, len(label), c_pf, c_V, pub),
                          "bpp_circuit_verify_batch_pub", ctx.h)
        reps, per = verify_calls, NV
    else:
        raise SystemExit("unknown entry " + entry)
    f()
    f()  # warmup: window tables, workspaces
    print(json.dumps([window(f, reps, per) for _ in range(windows)]))


def ab(other: str, a) -> dict:
    """Every existing entry point, this checkout and `other` in alternating processes."""
    out = {}
    for entry in AB_ENTRIES:
        runs = {"this": [], "other": []}
        for side in ("other", "this", "other", "this"):
            tree = other if side == "other" else str(ROOT / "bulletproof-perm_amd")
            r = subprocess.run([sys.executable, __file__, "--child", entry, "--tree", tree, "--windows", str(a.windows),
                                "--prove-batches", str(a.prove_batches), "--verify-calls", str(a.verify_calls)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"{entry} ({side}) failed:\n{r.stderr[-2000:]}")
            runs[side] += json.loads(r.stdout.strip().splitlines()[-1])
        t, o = stats(runs["this"]), stats(runs["other"])
        out[entry] = {"this": t, "other": o, "ratio": t["median"] / o["median"],
                      "other_spread": (o["max"] - o["min"]) / o["median"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--prove-batches", type=int, default=20, help="batches per proving window")
    ap.add_argument("--verify-calls", type=int, default=10, help="calls per verifying window")
    ap.add_argument("--ab-tree", default="", help="another built checkout's bulletproof-perm_amd directory")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=str(ROOT / "bulletproof-perm_amd"), help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    if a.child:
        return child(a.child, a.windows, a.prove_batches, a.verify_calls)

    s = Shapes()
    ctx = s.ctx
    for _ in range(2):  # warmup: window tables, workspaces
        s.prove_rs(B)
        s.prove_m(B)
    runs = {"prove_plain": [], "prove_masked": [], "verify_plain": [], "verify_masked": []}
    for _ in range(a.windows):
        runs["prove_plain"].append(window(lambda: s.prove_rs(B), a.prove_batches, B))
        runs["prove_masked"].append(window(lambda: s.prove_m(B), a.prove_batches, B))
    s.prove_rs(NV)  # the verifiers' inputs
    s.prove_m(NV)
    s.verify_rs()
    s.verify_m()
    for _ in range(a.windows):
        runs["verify_plain"].append(window(s.verify_rs, a.verify_calls, NV))
        runs["verify_masked"].append(window(s.verify_m, a.verify_calls, NV))

    out = {"shape": {"cards": K, "prove_batch": B, "verify_proofs": NV, "windows": a.windows,
                     "prove_batches_per_window": a.prove_batches, "verify_calls_per_window": a.verify_calls},
           "unit": "proofs/s",
           "yardstick": "bpp_reshuffle_prove_batch / bpp_reshuffle_verify_batch on the same shapes, same process, "
                        "interleaved windows",
           "proof_bytes": {"plain": s.rs_len, "masked": s.m_len}}
    for side in ("prove", "verify"):
        y, d = stats(runs[side + "_plain"]), stats(runs[side + "_masked"])
        out[side] = {"plain": y, "masked": d, "ratio": d["median"] / y["median"]}
    prof = {}
    for name, f in (("plain", lambda: (s.prove_rs(B), s.verify_rs())), ("masked", lambda: (s.prove_m(B), s.verify_m()))):
        ctx.profile(True)
        ctx.profile_reset()
        f()
        prof[name] = {}
        for st in STAGES:
            try:
                prof[name][st] = round(ctx.profile_get(st)[0], 4)
            except s.bpperm.BppError:  # a stage this run did not pass
                pass
        ctx.profile(False)
    out["stage_profile_ms"] = prof
    s.close()
    if a.ab_tree:
        out["existing_entry_points_vs_other_checkout"] = ab(a.ab_tree, a)
    print(json.dumps({k: {"ratio": round(out[k]["ratio"], 4)} |
                      {q: {r: round(out[k][q][r]) for r in ("median", "min", "max")} for q in ("plain", "masked")}
                      for k in ("prove", "verify")}))
    if a.ab_tree:
        print(json.dumps({e: {"ratio": round(v["ratio"], 4), "other_spread": round(v["other_spread"], 4)}
                          for e, v in out["existing_entry_points_vs_other_checkout"].items()}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
