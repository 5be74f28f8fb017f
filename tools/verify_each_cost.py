"""Cost of bpp_perm_verify_batch_each on the config-5 shape: 52 cards, 4096
proofs in one call, pageable inputs, one batch at a time.

    timeout -k 10 900 python tools/verify_each_cost.py [--passes 3] [--reps 20] [--out FILE]

(a) A batch that passes: bpp_perm_verify_batch_each against
    bpp_perm_verify_batch.  Both issue the same launches (the work counters
    are equal, tests/test_gpu_verify_each.py); required: the difference of
    the medians stays inside the spread of the interleaved passes.
(b) A batch with 1 bad proof and one with 64: bpp_perm_verify_batch_each
    against a loop of bpp_perm_verify over the same 4096 proofs -- the only
    way to the same answer without it.  Required: faster than the loop; the
    ratio is reported as measured.
(c) The ctx.profile stages of one failing call.

All through the C ABI on buffers marshalled before the clock starts, in one
process, the sides interleaved (box-to-box spread is up to 7 %: only same-box
interleaved numbers compare): in every pass the two sides of (a) alternate
window by window, in either order, behind an untimed window, and the spread is
that of all timed windows of a side.  Exit status 1 if (a) or (b) is
not met, or a verdict vector is wrong.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
K, COUNT, GENS = 52, 4096, 128
STAGES = ("verify_upload", "verify_replay", "verify_replay_dev", "verify_replay_post", "verify_decompress",
          "verify_terms", "verify_scalars", "msm_digits", "msm_scan", "msm_scatter", "msm_count", "msm_accumulate",
          "msm_fixup", "msm_reduce", "verify_each_terms", "msm_horner", "compress", "verify_each_verdict")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--count", type=int, default=COUNT)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bpperm
    n = a.count
    ctx = bpperm.Context(0)
    g = bpperm.Gens(ctx, GENS)
    pr = bpperm.PermProver(g, K)
    pl, vl = pr.proof_len, 32 * pr.m
    pb, vb = b"", b""
    for b0 in range(0, n, 256):
        p, v = pr.prove_batch(list(range(500_000 + b0, 500_000 + min(b0 + 256, n))), raw=True)
        pb += p
        vb += v
    lib, lab = ctx.lib, pr.label

    def tampered(bad):
        b = bytearray(pb)
        for i in bad:
            b[i * pl + 8 * 32 + 70] ^= 1  # t_hat, stays canonical
        return bytes(b)

    ok = C.create_string_buffer(n)

    def batch(p):
        return lib.bpp_perm_verify_batch(ctx.h, g.h, K, n, lab, len(lab), p, vb)

    def each(p):
        return lib.bpp_perm_verify_batch_each(ctx.h, g.h, K, n, lab, len(lab), p, vb, ok)

    def loop(p):
        out = bytearray(n)
        for i in range(n):
            rc = lib.bpp_perm_verify(ctx.h, g.h, K, lab, len(lab), p[i * pl:(i + 1) * pl], pl, vb[i * vl:(i + 1) * vl])
            if rc not in (0, 6):
                raise RuntimeError(f"bpp_perm_verify rc={rc}")
            out[i] = rc == 0
        return bytes(out)

    def timed(f, p, reps, want_rc):
        t0 = time.perf_counter()
        for _ in range(reps):
            rc = f(p)
            if rc != want_rc:
                raise RuntimeError(f"{f.__name__} rc={rc}, expected {want_rc}: "
                                   f"{(lib.bpp_ctx_last_error(ctx.h) or b'').decode()}")
        return (time.perf_counter() - t0) / reps * 1e3

    bad1, bad64 = [n // 2 + 1], sorted({(i * 64 + 17) % n for i in range(64)})
    p1, p64 = tampered(bad1), tampered(bad64)
    want = {}
    for name, bad in (("bad1", bad1), ("bad64", bad64)):
        w = bytearray(b"\x01" * n)
        for i in bad:
            w[i] = 0
        want[name] = bytes(w)
    for _ in range(3):  # warm-up: every shape the timed windows use
        assert batch(pb) == 0 and each(pb) == 0 and each(p1) == 6 and each(p64) == 6
    good = True
    runs = {"batch_good": [], "each_good": [], "each_bad1": [], "each_bad64": [], "loop_bad1": [], "loop_bad64": []}
    for ps in range(a.passes):
        # (an untimed window first: the loops of singles that end a pass leave
        # the device and the host caches in another state than a batch does;
        # then the two sides alternate, in either order)
        timed(batch, pb, a.reps, 0)
        for f, name in ((batch, "batch_good"), (each, "each_good"), (each, "each_good"), (batch, "batch_good")):
            runs[name].append(timed(f, pb, a.reps, 0))
        runs["each_bad1"].append(timed(each, p1, a.reps, 6))
        good &= ok.raw == want["bad1"]
        runs["each_bad64"].append(timed(each, p64, a.reps, 6))
        good &= ok.raw == want["bad64"]
        for name, p in (("bad1", p1), ("bad64", p64)):
            t0 = time.perf_counter()
            got = loop(p)
            runs["loop_" + name].append((time.perf_counter() - t0) * 1e3)
            good &= got == want[name]
        print(f"pass {ps}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in runs.items()), flush=True)

    def med(k):
        v = sorted(runs[k])
        return v[len(v) // 2]

    spread = max(max(runs[k]) - min(runs[k]) for k in ("batch_good", "each_good"))
    diff = med("each_good") - med("batch_good")
    ctx.profile(True)
    ctx.profile_reset()
    assert each(p64) == 6
    stages = {}
    for s in STAGES:
        try:
            ms, cnt = ctx.profile_get(s)
        except Exception:
            continue
        if cnt:
            stages[s] = {"ms": ms, "launches": cnt}
    ctx.profile(False)
    out = {"shape": {"cards": K, "proofs": n, "inputs": "pageable", "reps_per_window": a.reps, "passes": a.passes},
           "ms_per_call": runs, "median_ms": {k: med(k) for k in runs},
           "good_batch": {"each_minus_batch_ms": diff, "spread_of_the_passes_ms": spread,
                          "within_spread": abs(diff) <= spread},
           "failing_batch": {f"loop_over_each_{b}": med("loop_" + b) / med("each_" + b) for b in ("bad1", "bad64")},
           "stages_of_one_failing_call_64_bad": stages, "verdicts_correct": good}
    out["ok"] = bool(good and out["good_batch"]["within_spread"]
                     and all(r > 1 for r in out["failing_batch"].values()))
    print(json.dumps({k: out[k] for k in ("median_ms", "good_batch", "failing_batch", "ok")}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    g.close()
    ctx.close()
    sys.exit(0 if out["ok"] else 1)


if __name__ == "__main__":
    main()
