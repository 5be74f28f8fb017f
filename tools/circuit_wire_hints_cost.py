"""Cost of hints over wires and x (bpp_circuit_create_wire_hinted): what deriving
late auxiliary values inside the witness kernel costs against handing every
value over, and that the feature costs the existing entry points nothing.

    python tools/circuit_wire_hints_cost.py [--windows 7] [--parent-lib PATH]
        [--out profiles/circuit_wire_hints_cost_ab.json]

(a) Derived against supplied: max_of(52, 6) (BPP_CIRCUIT_LARGE, 720 gates) and
    blackjack_total(5) (92 gates, one public input), proved in 64-proof batches
    by one circuit handle -- aux == NULL (k_hint_aux, then the late hints inside
    k_witness_program*_late) and aux = aux_of(v) prepared before any clock starts
    (the kernels of before) -- one process, one context, interleaved windows
    (derived, supplied, derived, ...).  proofs/s with medians and window spread;
    the "hint_aux" and "witness_program" stage times of one more batch each way
    (Context.profile); the bytes a batch stages ("prove_stage_bytes").
    Reported, no threshold.
(b) What exists, against the parent commit's library (--parent-lib), in fresh
    child processes that alternate between the two libraries, raw C ABI common
    to both: bpp_perm_verify_batch (52 cards x 4096 proofs),
    bpp_circuit_prove_batch on a hinted in_range(64) with aux == NULL (64-proof
    batches) and bpp_circuit_verify_batch_pub (shuffle_of_public(52) x 4096
    proofs).  within_parent_spread: this library's median lies inside the
    min..max of the parent's own windows (or above it).  The existing kernels
    compile to the parent's code, so anything outside that spread is a finding.

A tool, not part of bench.py; recorded, not gated.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import circuit_large_cost as clc  # noqa: E402  (stats, window, shuffle_rows)

BATCH = 64
K, NV = clc.K, clc.NV


def bj(ranks):
    S = sum(min(r, 10) for r in ranks)
    return S + (10 if 1 in ranks and S <= 11 else 0)


class Case:
    """One wire-hinted circuit's marshalled inputs: BATCH proofs' v, pub and
    aux_of(v), made before any clock starts; prove(derived) is the raw C-ABI call."""

    def __init__(self, ctx, gens, circ, desc, rows, pubs, label=b"bp-perm"):
        import bpperm
        self.ctx, self.gens, self.circ, self.label = ctx, gens, circ, label
        self.lib, self.check = ctx.lib, bpperm.check
        sb = lambda x: x.to_bytes(32, "little")
        self.v = C.c_char_p(b"".join(sb(x) for v in rows for x in v))
        self.aux = C.c_char_p(b"".join(sb(x) for v in rows for x in desc.aux_of(v)))
        self.pub = C.c_char_p(b"".join(sb(x) for u in pubs for x in u)) if pubs else None
        self.pf = C.create_string_buffer(circ.proof_len * BATCH)
        self.V = C.create_string_buffer(32 * circ.m * BATCH)

    def prove(self, derived: bool):
        self.check(self.lib.bpp_circuit_prove_batch_pub(self.ctx.h, self.gens.h, self.circ.h, BATCH, self.v,
                                                        None if derived else self.aux, self.pub, None, None,
                                                        self.label, len(self.label), self.pf, self.V),
                   "bpp_circuit_prove_batch_pub", self.ctx.h)

    def one_batch(self, derived: bool):
        """stage times (ms) and staged bytes of one profiled batch"""
        import bpperm
        self.ctx.profile(True)
        self.ctx.profile_reset()
        self.ctx.work_reset()
        self.prove(derived)
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


def derived_vs_supplied(a, ctx, gens):
    import bpperm
    from bpperm import gadgets
    rnd = random.Random(5206)
    out = {"unit": "proofs/s", "shape": {"batch": BATCH, "batches_per_window": a.batches, "windows": a.windows},
           "order": "derived, supplied, derived, ... in one process on one context"}
    for name, desc, large in (("max_of(52, 6)", gadgets.max_of(52, 6), True),
                              ("blackjack_total(5)", gadgets.blackjack_total(5), False)):
        if desc.n_pub:
            rows = [[rnd.randrange(1, 14) for _ in range(desc.m_in)] for _ in range(BATCH)]
            pubs = [[bj(r)] for r in rows]
        else:
            rows = [[rnd.randrange(1 << 6) for _ in range(desc.m_in - 1)] for _ in range(BATCH)]
            rows = [r + [max(r)] for r in rows]
            pubs = None
        circ = bpperm.Circuit(desc, large=large)
        assert circ.has_hints and desc.hints.wire
        c = Case(ctx, gens, circ, desc, rows, pubs)
        for _ in range(3):
            c.prove(True)
            c.prove(False)
        runs = {"derived": [], "supplied": []}
        for _ in range(a.windows):
            for side in runs:
                runs[side].append(clc.window(lambda: c.prove(side == "derived"), a.batches, BATCH))
        d, s = clc.stats(runs["derived"]), clc.stats(runs["supplied"])
        late = sum(1 for t in range(desc.n_aux)
                   if any(v == 1 + desc.m_in or v >= 2 + desc.m_in + desc.n_pub
                          for v in desc.hints.lc_var[desc.hints.lc_off[t]:desc.hints.lc_off[t + 1]]))
        out[name] = {"n_gates": desc.n_gates, "n_aux": desc.n_aux, "late_hints": late, "n_p": circ.n_p, "Q": circ.Q,
                     "aux_bytes_per_proof": 32 * desc.n_aux, "derived": d, "supplied": s,
                     "ratio": d["median"] / s["median"],
                     "derived_spread": (d["max"] - d["min"]) / d["median"],
                     "supplied_spread": (s["max"] - s["min"]) / s["median"],
                     "one_batch": {"derived": c.one_batch(True), "supplied": c.one_batch(False)}}
        circ.close()
        print(f"part a: {name} done", file=sys.stderr, flush=True)
    return out


def existing_child(a):
    """One library (BPP_LIB, or the tree's), raw C ABI common to both; one JSON line."""
    from bpperm import _lib, gadgets
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args

    def ok(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {rc}")

    class Desc(C.Structure):
        _fields_ = [("m_in", C.c_uint32), ("n_gates", C.c_uint32), ("n_aux", C.c_uint32), ("n_asserts", C.c_uint32),
                    ("side_aux", C.POINTER(C.c_uint32)), ("lc_off", C.POINTER(C.c_uint32)),
                    ("lc_var", C.POINTER(C.c_uint32)), ("lc_coef", C.c_char_p)]

    class Hints(C.Structure):
        _fields_ = [("op", C.POINTER(C.c_uint32)), ("lc_off", C.POINTER(C.c_uint32)),
                    ("lc_var", C.POINTER(C.c_uint32)), ("lc_coef", C.c_char_p)]

    keep = []
    u32a = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)

    def create(desc, hinted=False):
        arrs = (u32a(desc.side_aux), u32a(desc.lc_off), u32a(desc.lc_var), b"".join(desc.lc_coef))
        keep.append(arrs)
        h = C.c_void_p()
        d = Desc(desc.m_in, desc.n_gates, desc.n_aux, desc.n_asserts, *arrs)
        if hinted:
            hd = desc.hints
            harr = (u32a(hd.op), u32a(hd.lc_off), u32a(hd.lc_var), b"".join(hd.lc_coef))
            keep.append(harr)
            ok(lib.bpp_circuit_create_hinted(C.byref(d), desc.n_pub, 0, C.byref(Hints(*harr)), C.byref(h)), "hinted")
        else:
            ok(lib.bpp_circuit_create_pub(C.byref(d), desc.n_pub, C.byref(h)), "circuit")
        return h

    ctx, gens = C.c_void_p(), C.c_void_p()
    ok(lib.bpp_ctx_create(0, C.byref(ctx)), "ctx")
    ok(lib.bpp_gens_create(ctx, 128, C.byref(gens)), "gens")
    rng, pubc = create(gadgets.in_range(64), True), create(gadgets.shuffle_of_public(K))
    label = b"bp-perm"
    rnd = random.Random(52)
    deck = [i.to_bytes(32, "little") for i in range(1, K + 1)]
    flat = []
    for _ in range(NV):
        p = list(range(K))
        rnd.shuffle(p)
        flat += p
    pm = (C.c_uint32 * (NV * K))(*flat)
    cbuf = C.c_char_p(b"".join(deck) * NV)
    plen, m = lib.bpp_perm_proof_len(K), 2 * K + 1
    pf, V = C.create_string_buffer(plen * NV), C.create_string_buffer(32 * m * NV)
    ok(lib.bpp_perm_prove_shuffle_batch(ctx, gens, K, NV, cbuf, pm, None, None, label, len(label), pf, V), "prove")
    rbuf = C.c_char_p(b"".join(rnd.randrange(1 << 64).to_bytes(32, "little") for _ in range(BATCH)))
    rpf = C.create_string_buffer(lib.bpp_circuit_proof_len(rng) * BATCH)
    rV = C.create_string_buffer(32 * 2 * BATCH)
    prow = clc.shuffle_rows(rnd, K, NV)
    pv, pu = C.c_char_p(b"".join(r[0] for r in prow)), C.c_char_p(b"".join(r[2] for r in prow))
    plen2 = lib.bpp_circuit_proof_len(pubc)
    ppf, pV = C.create_string_buffer(plen2 * NV), C.create_string_buffer(32 * (K + 1) * NV)
    ok(lib.bpp_circuit_prove_batch_pub(ctx, gens, pubc, NV, pv, None, pu, None, None, label, len(label), ppf, pV), "pub")

    def verify():
        ok(lib.bpp_perm_verify_batch(ctx, gens, K, NV, label, len(label), pf, V), "bpp_perm_verify_batch")

    def prove():
        ok(lib.bpp_circuit_prove_batch(ctx, gens, rng, BATCH, rbuf, None, None, None, label, len(label), rpf, rV),
           "bpp_circuit_prove_batch")

    def verify_pub():
        ok(lib.bpp_circuit_verify_batch_pub(ctx, gens, pubc, NV, label, len(label), ppf, pV, pu),
           "bpp_circuit_verify_batch_pub")

    for _ in range(3):
        verify()
        prove()
        verify_pub()
    runs = {"verify": [], "prove": [], "verify_pub": []}
    for _ in range(a.windows):
        runs["verify"].append(clc.window(verify, a.verify_calls, NV))
        runs["prove"].append(clc.window(prove, a.prove_batches, BATCH))
        runs["verify_pub"].append(clc.window(verify_pub, a.verify_calls, NV))
    print("AB " + json.dumps(runs))
    for c in (rng, pubc):
        lib.bpp_circuit_destroy(c)
    lib.bpp_gens_destroy(gens)
    lib.bpp_ctx_destroy(ctx)


def existing(a):
    keys = ("verify", "prove", "verify_pub")
    runs = {s: {k: [] for k in keys} | {"per_process": []} for s in ("parent", "this")}
    for _ in range(a.ab_rounds):
        for side, path in (("parent", a.parent_lib), ("this", "")):
            env = {k: v for k, v in os.environ.items() if k != "BPP_LIB"}
            if path:
                env["BPP_LIB"] = str(Path(path).resolve())
            r = subprocess.run([sys.executable, __file__, "--existing-child", "--ab-windows", str(a.ab_windows),
                                "--prove-batches", str(a.prove_batches), "--verify-calls", str(a.verify_calls)],
                               capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                raise RuntimeError((r.stdout + r.stderr)[-3000:])
            got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1][3:])
            runs[side]["per_process"].append(got)
            print(f"part b: a {side} process done", file=sys.stderr, flush=True)
            for k in keys:
                runs[side][k] += got[k]
    out = {"what": {"verify": "bpp_perm_verify_batch, 52 cards x 4096 proofs",
                    "prove": "bpp_circuit_prove_batch, hinted in_range(64), aux == NULL, 64-proof batches one at a time",
                    "verify_pub": "bpp_circuit_verify_batch_pub, shuffle_of_public(52) x 4096 proofs"},
           "unit": "proofs/s", "processes_per_library": a.ab_rounds, "windows_per_process": a.ab_windows}
    for k in keys:
        p, t = clc.stats(runs["parent"][k]), clc.stats(runs["this"][k])
        out[k] = {"parent": p, "this": t, "ratio": t["median"] / p["median"],
                  "parent_spread": (p["max"] - p["min"]) / p["median"], "this_spread": (t["max"] - t["min"]) / t["median"],
                  "within_parent_spread": p["min"] <= t["median"] <= p["max"] or t["median"] >= p["max"]}
    out["per_process"] = {s: runs[s]["per_process"] for s in runs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batches", type=int, default=40, help="64-proof batches per window of part a")
    ap.add_argument("--prove-batches", type=int, default=200, help="64-proof batches per proving window of part b")
    ap.add_argument("--verify-calls", type=int, default=100, help="4096-proof calls per verifying window of part b")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libbpperm.so (part b; skipped without it)")
    ap.add_argument("--ab-rounds", type=int, default=2, help="processes per library in part b")
    ap.add_argument("--ab-windows", type=int, default=5, help="windows per process in part b")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: a, b")
    ap.add_argument("--existing-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.existing_child:
        a.windows = a.ab_windows
        return existing_child(a)
    skip = set(a.skip.split(","))
    out = {}
    if "a" not in skip:
        import bpperm
        ctx = bpperm.Context(0)
        gens = bpperm.Gens(ctx, 1024)
        out["derived_vs_supplied"] = derived_vs_supplied(a, ctx, gens)
        gens.close()
        ctx.close()
    if a.parent_lib and "b" not in skip:
        out["existing"] = existing(a)
    brief = {}
    if "derived_vs_supplied" in out:
        brief["derived_vs_supplied"] = {
            n: {"derived": round(v["derived"]["median"], 1), "supplied": round(v["supplied"]["median"], 1),
                "ratio": round(v["ratio"], 3), "one_batch": v["one_batch"]}
            for n, v in out["derived_vs_supplied"].items() if isinstance(v, dict) and "derived" in v}
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
