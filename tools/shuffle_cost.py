"""Cost of proving caller-supplied shuffles (bpp_perm_prove_shuffle_batch)
against the seeded production prover (bpp_perm_prove_batch_entropy) of the
PARENT commit, on the config-4 shape: 52 cards, 384-proof batches, one batch at
a time and 32 batches in flight (README.md / VERDICT.md; bench.py's harness:
one host thread and context per batch in flight, 8 hardware queues).

    python tools/shuffle_cost.py --parent-lib PATH [--passes 3] [--out FILE]

PATH is libbpperm.so built from the parent commit (a checkout of it and
`python bulletproof-perm_amd/build.py`).  The two libraries run interleaved,
one fresh process per measurement (a process loads one libbpperm): parent
seeded, this tree's shuffle with drawn blindings, this tree's shuffle with
supplied blindings, this tree's seeded entry (reported only), and again,
`--passes` times.  Both sides go through the C
ABI with buffers marshalled before the clock starts.

The only intended extra work is the V commitments' value half (full-width
cards: 8 + 8 instead of 8 + 2 table additions on the longest lane, 128
instead of 66 per commitment, gens.hip pedersen_dev; the Pedersen kernel is
~12 % of a batch's summed kernel time) -- some percent of a
batch.  Accepted: the new entry no more than 15 % below
the parent's seeded rate in both regimes (the ~7 % box-to-box spread of
README.md plus that cost).  Exit status 1 if it is.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW_LIB = ROOT / "bulletproof-perm_amd" / "bpperm" / "libbpperm.so"
K, B, GENS = 52, 384, 128
LIMIT = 0.85
L = 2**252 + 27742317777372353535851937790883648493


def child(a):
    # as bench.py: eight hardware queues for the many streams, before HIP starts
    os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("BPP_BENCH_HW_QUEUES", "8")
    lib = C.CDLL(a.lib)
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    lib.bpp_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.bpp_gens_create.argtypes = [vp, sz, C.POINTER(vp)]
    lib.bpp_ctx_last_error.restype = C.c_char_p
    lib.bpp_ctx_last_error.argtypes = [vp]
    lib.bpp_perm_proof_len.restype = sz
    lib.bpp_perm_proof_len.argtypes = [u32]
    lib.bpp_host_tuning.argtypes = [u32]
    lib.bpp_perm_prove_batch_entropy.argtypes = [vp, vp, u32, sz, vp, vp, sz, vp, vp]
    lib.bpp_perm_verify_batch.argtypes = [vp, vp, u32, sz, vp, sz, vp, vp]
    shuffle = a.mode.startswith("shuffle")
    if shuffle:
        lib.bpp_perm_prove_shuffle_batch.argtypes = [vp, vp, u32, sz, vp, vp, vp, vp, vp, sz, vp, vp]
    lib.bpp_host_tuning(1)
    S = a.streams
    ctxs = []
    for _ in range(S):
        h = vp()
        assert lib.bpp_ctx_create(0, C.byref(h)) == 0
        ctxs.append(h)
    gens = vp()
    assert lib.bpp_gens_create(ctxs[0], GENS, C.byref(gens)) == 0
    label = b"bp-perm"
    pl = lib.bpp_perm_proof_len(K)

    import random
    rnd = random.Random(52)

    def scalars(n):  # canonical: below 2^252
        b = bytearray(rnd.randbytes(32 * n))
        for i in range(31, len(b), 32):
            b[i] &= 0x0F
        return bytes(b)

    class Stream:
        def __init__(self, ctx):
            self.ctx = ctx
            self.pf = C.create_string_buffer(pl * B)
            self.V = C.create_string_buffer(32 * (2 * K + 1) * B)
            if shuffle:
                self.cards = C.create_string_buffer(scalars(B * K), 32 * B * K)
                flat = []
                for _ in range(B):
                    p = list(range(K))
                    rnd.shuffle(p)
                    flat += p
                self.perms = (C.c_uint32 * (B * K))(*flat)
                self.gam = C.create_string_buffer(scalars(2 * B * K), 64 * B * K) if a.mode == "shuffle_gammas" else None

        def batch(self):
            if shuffle:
                rc = lib.bpp_perm_prove_shuffle_batch(self.ctx, gens, K, B, self.cards, self.perms, self.gam, None,
                                                      label, len(label), self.pf, self.V)
            else:
                rc = lib.bpp_perm_prove_batch_entropy(self.ctx, gens, K, B, None, label, len(label), self.pf, self.V)
            if rc:
                raise RuntimeError(f"prove rc={rc}: {(lib.bpp_ctx_last_error(self.ctx) or b'').decode()}")

    st = [Stream(c) for c in ctxs]
    for s in st:  # warmup (window tables, workspaces)
        s.batch()
        s.batch()
    assert lib.bpp_perm_verify_batch(ctxs[0], gens, K, B, label, len(label), st[0].pf, st[0].V) == 0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        st[0].batch()
    el_one = time.perf_counter() - t0

    errs = []

    def run(s):
        try:
            for _ in range(a.steps):
                s.batch()
        except Exception as e:  # surfaced after the join
            errs.append(e)

    th = [threading.Thread(target=run, args=(s,)) for s in st]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    el_fl = time.perf_counter() - t0
    if errs:
        raise errs[0]
    assert lib.bpp_perm_verify_batch(ctxs[0], gens, K, B, label, len(label), st[-1].pf, st[-1].V) == 0
    print("RESULT " + json.dumps({"mode": a.mode, "one_at_a_time_proofs_s": a.steps * B / el_one,
                                  "one_at_a_time_ms_per_batch": el_one / a.steps * 1e3,
                                  "in_flight_proofs_s": S * a.steps * B / el_fl, "streams": S, "steps": a.steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=str(ROOT / "bulletproof-perm_amd" / "bpperm" / "variants" /
                                                "libbpperm_parent.so"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=24, help="batches per stream per measurement")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="seeded", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not Path(a.parent_lib).exists():
        sys.exit(f"no parent library at {a.parent_lib}: build the parent commit and pass --parent-lib")
    # (seeded_this_tree: this tree's seeded entry, reported only -- that path is meant to be unchanged)
    runs = {"seeded": [], "shuffle": [], "shuffle_gammas": [], "seeded_this_tree": []}
    for p in range(a.passes):
        for mode in runs:  # interleaved: parent, new, new, new, parent, ...
            lib = a.parent_lib if mode == "seeded" else str(NEW_LIB)
            r = subprocess.run([sys.executable, __file__, "--child", "--lib", lib, "--mode", mode, "--streams",
                                str(a.streams), "--steps", str(a.steps)], capture_output=True, text=True, timeout=240)
            if r.returncode != 0:  # nothing more on the GPU after a failed step
                sys.exit(f"pass {p} {mode}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            res = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
            runs[mode].append(res)
            print(f"pass {p} {mode:16s} one at a time {res['one_at_a_time_proofs_s'] / 1e3:7.1f} K proofs/s "
                  f"({res['one_at_a_time_ms_per_batch']:.3f} ms per batch), {a.streams} in flight "
                  f"{res['in_flight_proofs_s'] / 1e3:7.1f} K proofs/s", flush=True)

    def med(mode, key):
        v = sorted(r[key] for r in runs[mode])
        return v[len(v) // 2]

    out = {"shape": {"cards": K, "batch": B, "in_flight": a.streams, "steps_per_stream": a.steps, "passes": a.passes},
           "baseline": "bpp_perm_prove_batch_entropy, parent commit's library, interleaved on the same box",
           "limit": LIMIT, "runs": runs, "median": {}, "ratio_vs_parent_seeded": {}, "ok": True}
    for key in ("one_at_a_time_proofs_s", "in_flight_proofs_s"):
        base = med("seeded", key)
        out["median"][key] = {m: med(m, key) for m in runs}
        for m in ("shuffle", "shuffle_gammas"):
            ratio = med(m, key) / base
            out["ratio_vs_parent_seeded"][f"{m}:{key}"] = ratio
            out["ok"] &= ratio >= LIMIT
    print(json.dumps({k: out[k] for k in ("median", "ratio_vs_parent_seeded", "ok")}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    sys.exit(0 if out["ok"] else 1)


if __name__ == "__main__":
    main()
