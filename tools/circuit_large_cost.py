"""Cost of the large-circuit kernels (bpp_circuit_create_ex), and that they cost
the existing entry points nothing.

    python tools/circuit_large_cost.py [--windows 5] [--parent-lib PATH] [--out profiles/circuit_large_cost_ab.json]

(a) What tiling costs where the narrow kernels fit: two_half_shuffle(52) created
    plain and with BPP_CIRCUIT_TILED, one process, one context, interleaved
    windows (plain, tiled, plain, tiled, ...): proving in 384-proof batches,
    verifying 4096 proofs per call, and the three kernels' stage times
    (Context.profile: poly_coef, verify_scalars, witness_program) of one more
    batch of each.  Reported, no threshold.
(b) The new capability at a user's size: shuffle_of_public(416) (an 8-deck shoe,
    830 gates, n_p = 1024) and in_range_many(16, 64) (1024 gates, n_p = 1024)
    under BPP_CIRCUIT_LARGE: proofs/s proving (--large-batch proofs a batch),
    proofs/s verifying 1024 proofs a call, the same three stage times.  First
    measurements: nothing exists to compare them with.
(c) What exists, against the parent commit's library (--parent-lib) in fresh
    child processes that alternate between the two libraries: bpp_perm_verify_batch,
    bpp_circuit_prove_batch (two_half_shuffle(52)) and bpp_circuit_verify_batch_pub
    (shuffle_of_public(52)) at 52 cards.  within_parent_spread: this library's
    median lies inside the min..max of the parent's own windows (or above it).

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
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))

K, B, NV, NVL = 52, 384, 4096, 1024
L = 2**252 + 27742317777372353535851937790883648493
KERNELS = ("witness_program", "poly_coef", "verify_scalars")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "windows": v}


def window(f, reps, per):
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return reps * per / (time.perf_counter() - t0)


class Case:
    """One circuit's marshalled inputs and raw C-ABI calls: n proofs' v, aux and
    pub (the first `batch` of them prove), buffers made before any clock starts."""

    def __init__(self, ctx, gens, circ, rows, n, batch, label=b"bp-perm"):
        import bpperm
        self.ctx, self.gens, self.circ, self.n, self.batch, self.label = ctx, gens, circ, n, batch, label
        self.lib, self.check = ctx.lib, bpperm.check
        self.raw = [b"".join(r[k] for r in rows) for k in range(3)]  # v, aux, pub: proof-major
        self.v, self.aux, self.pub = (C.c_char_p(b) if b else None for b in self.raw)
        self.pf = C.create_string_buffer(circ.proof_len * n)
        self.V = C.create_string_buffer(32 * circ.m * n)

    def prove(self, n=None):
        self.check(self.lib.bpp_circuit_prove_batch_pub(self.ctx.h, self.gens.h, self.circ.h, n or self.batch, self.v,
                                                        self.aux, self.pub, None, None, self.label, len(self.label),
                                                        self.pf, self.V), "bpp_circuit_prove_batch_pub", self.ctx.h)

    def fill(self):
        """the verifier's n proofs, proved batch by batch"""
        m, pl = self.circ.m, self.circ.proof_len
        for o in range(0, self.n, self.batch):
            cnt = min(self.batch, self.n - o)
            part = lambda b, per: C.c_char_p(b[per * o:per * (o + cnt)]) if b else None
            self.check(self.lib.bpp_circuit_prove_batch_pub(
                self.ctx.h, self.gens.h, self.circ.h, cnt, part(self.raw[0], 32 * self.circ.m_in),
                part(self.raw[1], 32 * self.circ.n_aux), part(self.raw[2], 32 * self.circ.n_pub), None, None, self.label,
                len(self.label), C.byref(self.pf, pl * o), C.byref(self.V, 32 * m * o)),
                "bpp_circuit_prove_batch_pub", self.ctx.h)

    def verify(self):
        self.check(self.lib.bpp_circuit_verify_batch_pub(self.ctx.h, self.gens.h, self.circ.h, self.n, self.label,
                                                         len(self.label), self.pf, self.V, self.pub),
                   "bpp_circuit_verify_batch_pub", self.ctx.h)

    def kernel_ms(self):
        import bpperm
        self.ctx.profile(True)
        self.ctx.profile_reset()
        self.prove()
        self.verify()
        out = {}
        for s in KERNELS:
            try:
                out[s] = round(self.ctx.profile_get(s)[0], 4)
            except bpperm.BppError:
                pass
        self.ctx.profile(False)
        return out


def two_half_rows(rnd, n):
    rows = []
    for _ in range(n):
        cards = [rnd.randrange(L).to_bytes(32, "little") for _ in range(K)]
        p = list(range(K))
        rnd.shuffle(p)
        rows.append((b"".join(cards) + b"".join(cards[i] for i in p), b"", b""))
    return rows


def shuffle_rows(rnd, k, n):
    rows = []
    for _ in range(n):
        deck = [rnd.randrange(L).to_bytes(32, "little") for _ in range(k)]
        p = list(range(k))
        rnd.shuffle(p)
        rows.append((b"".join(deck[i] for i in p), b"", b"".join(deck)))
    return rows


def range_rows(rnd, desc, count, n):
    rows = []
    for _ in range(n):
        v = [rnd.randrange(1 << 64) for _ in range(count)]
        rows.append((b"".join(x.to_bytes(32, "little") for x in v),
                     b"".join(x.to_bytes(32, "little") for x in desc.aux_of(v)), b""))
    return rows


def tiling(a, ctx, gens):
    import bpperm
    from bpperm import gadgets
    rnd = random.Random(5201)
    desc = gadgets.two_half_shuffle(K)
    rows = two_half_rows(rnd, NV)
    sides = {"plain": Case(ctx, gens, bpperm.Circuit(desc), rows, NV, B),
             "tiled": Case(ctx, gens, bpperm.Circuit(desc, tiled=True), rows, NV, B)}
    for _ in range(2):
        for c in sides.values():
            c.prove()
    runs = {f"{w}_{s}": [] for w in ("prove", "verify") for s in sides}
    for _ in range(a.windows):
        for s, c in sides.items():
            runs["prove_" + s].append(window(c.prove, a.prove_batches, B))
    for c in sides.values():
        c.fill()
        c.verify()
    for _ in range(a.windows):
        for s, c in sides.items():
            runs["verify_" + s].append(window(c.verify, a.verify_calls, NV))
    out = {"circuit": "two_half_shuffle(52)", "n_p": sides["plain"].circ.n_p, "Q": sides["plain"].circ.Q,
           "unit": "proofs/s", "shape": {"prove_batch": B, "verify_proofs": NV, "windows": a.windows}}
    for w in ("prove", "verify"):
        p, t = stats(runs[w + "_plain"]), stats(runs[w + "_tiled"])
        out[w] = {"plain": p, "tiled": t, "ratio": t["median"] / p["median"]}
    out["kernel_ms"] = {s: c.kernel_ms() for s, c in sides.items()}
    out["kernel_ms"]["note"] = "one 384-proof batch proved, 4096 proofs verified; verify_scalars = consts + scalars + merge"
    return out


def capability(a, ctx, gens):
    import bpperm
    from bpperm import gadgets
    rnd = random.Random(4160)
    out = {"unit": "proofs/s", "first_measurements": True,
           "shape": {"prove_batch": a.large_batch, "verify_proofs": NVL, "windows": a.windows}}
    rm = gadgets.in_range_many(16, 64)
    for name, desc, rows in (("shuffle_of_public(416)", gadgets.shuffle_of_public(416), None),
                             ("in_range_many(16, 64)", rm, None)):
        rows = shuffle_rows(rnd, 416, NVL) if desc is not rm else range_rows(rnd, rm, 16, NVL)
        c = Case(ctx, gens, bpperm.Circuit(desc, large=True), rows, NVL, a.large_batch)
        c.prove()
        pv = [window(c.prove, a.large_prove_batches, a.large_batch) for _ in range(a.windows)]
        c.fill()
        c.verify()
        vv = [window(c.verify, a.large_verify_calls, NVL) for _ in range(a.windows)]
        out[name] = {"n_gates": desc.n_gates, "n_p": c.circ.n_p, "Q": c.circ.Q, "m": c.circ.m, "n_pub": c.circ.n_pub,
                     "proof_bytes": c.circ.proof_len, "prove": stats(pv), "verify": stats(vv),
                     "kernel_ms": c.kernel_ms()}
        c.circ.close()
    return out


def existing_child(a):
    """One library (BPP_LIB, or the tree's), raw C ABI common to both: windows of
    bpp_perm_verify_batch, bpp_circuit_prove_batch(two_half_shuffle(52)) and
    bpp_circuit_verify_batch_pub(shuffle_of_public(52)); one JSON line."""
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

    keep = []

    def create(desc):
        u32a = lambda xs: (C.c_uint32 * len(xs))(*xs)
        arrs = (u32a(desc.side_aux), u32a(desc.lc_off), u32a(desc.lc_var), b"".join(desc.lc_coef))
        keep.append(arrs)
        h = C.c_void_p()
        ok(lib.bpp_circuit_create_pub(C.byref(Desc(desc.m_in, desc.n_gates, desc.n_aux, desc.n_asserts, *arrs)),
                                      desc.n_pub, C.byref(h)), "circuit")
        return h

    ctx, gens = C.c_void_p(), C.c_void_p()
    ok(lib.bpp_ctx_create(0, C.byref(ctx)), "ctx")
    ok(lib.bpp_gens_create(ctx, 128, C.byref(gens)), "gens")
    two, pubc = create(gadgets.two_half_shuffle(K)), create(gadgets.shuffle_of_public(K))
    label = b"bp-perm"
    rnd = random.Random(52)
    deck = [i.to_bytes(32, "little") for i in range(1, K + 1)]
    flat, vals = [], []
    for _ in range(NV):
        p = list(range(K))
        rnd.shuffle(p)
        flat += p
        vals.append(b"".join(deck) + b"".join(deck[i] for i in p))
    pm = (C.c_uint32 * (NV * K))(*flat)
    cbuf, vbuf = C.c_char_p(b"".join(deck) * NV), C.c_char_p(b"".join(vals))
    plen, m = lib.bpp_perm_proof_len(K), 2 * K + 1
    pf, V = C.create_string_buffer(plen * NV), C.create_string_buffer(32 * m * NV)
    cpf, cV = C.create_string_buffer(plen * B), C.create_string_buffer(32 * m * B)
    ok(lib.bpp_perm_prove_shuffle_batch(ctx, gens, K, NV, cbuf, pm, None, None, label, len(label), pf, V), "prove")
    prow = shuffle_rows(rnd, K, NV)
    pv, pu = C.c_char_p(b"".join(r[0] for r in prow)), C.c_char_p(b"".join(r[2] for r in prow))
    plen2 = lib.bpp_circuit_proof_len(pubc)
    ppf, pV = C.create_string_buffer(plen2 * NV), C.create_string_buffer(32 * (K + 1) * NV)
    ok(lib.bpp_circuit_prove_batch_pub(ctx, gens, pubc, NV, pv, None, pu, None, None, label, len(label), ppf, pV), "pub")

    def verify():
        ok(lib.bpp_perm_verify_batch(ctx, gens, K, NV, label, len(label), pf, V), "bpp_perm_verify_batch")

    def prove():
        ok(lib.bpp_circuit_prove_batch(ctx, gens, two, B, vbuf, None, None, None, label, len(label), cpf, cV),
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
        runs["verify"].append(window(verify, a.verify_calls, NV))
        runs["prove"].append(window(prove, a.prove_batches, B))
        runs["verify_pub"].append(window(verify_pub, a.verify_calls, NV))
    print("AB " + json.dumps(runs))
    for c in (two, pubc):
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
            r = subprocess.run([sys.executable, __file__, "--existing-child", "--windows", str(a.windows),
                                "--prove-batches", str(a.prove_batches), "--verify-calls", str(a.verify_calls)],
                               capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                raise RuntimeError((r.stdout + r.stderr)[-3000:])
            got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1][3:])
            runs[side]["per_process"].append(got)
            for k in keys:
                runs[side][k] += got[k]
    out = {"what": {"verify": "bpp_perm_verify_batch, 52 cards x 4096 proofs",
                    "prove": "bpp_circuit_prove_batch, two_half_shuffle(52), 384-proof batches one at a time",
                    "verify_pub": "bpp_circuit_verify_batch_pub, shuffle_of_public(52) x 4096 proofs"},
           "unit": "proofs/s", "processes_per_library": a.ab_rounds, "windows_per_process": a.windows}
    for k in keys:
        p, t = stats(runs["parent"][k]), stats(runs["this"][k])
        out[k] = {"parent": p, "this": t, "ratio": t["median"] / p["median"],
                  "parent_spread": (p["max"] - p["min"]) / p["median"], "this_spread": (t["max"] - t["min"]) / t["median"],
                  "within_parent_spread": p["min"] <= t["median"] <= p["max"] or t["median"] >= p["max"]}
    out["per_process"] = {s: runs[s]["per_process"] for s in runs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--prove-batches", type=int, default=100, help="384-proof batches per proving window")
    ap.add_argument("--verify-calls", type=int, default=200, help="4096-proof calls per verifying window")
    ap.add_argument("--large-batch", type=int, default=64, help="proofs per large-circuit proving batch")
    ap.add_argument("--large-prove-batches", type=int, default=4)
    ap.add_argument("--large-verify-calls", type=int, default=4)
    ap.add_argument("--parent-lib", default="", help="the parent commit's libbpperm.so (part c; skipped without it)")
    ap.add_argument("--ab-rounds", type=int, default=2, help="processes per library in part c")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: a, b, c")
    ap.add_argument("--existing-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.existing_child:
        return existing_child(a)
    skip = set(a.skip.split(","))
    out = {}
    if not {"a", "b"} <= skip:
        import bpperm
        ctx = bpperm.Context(0)
        gens = bpperm.Gens(ctx, 1024)
        if "a" not in skip:
            out["tiling"] = tiling(a, ctx, gens)
        if "b" not in skip:
            out["capability"] = capability(a, ctx, gens)
        gens.close()
        ctx.close()
    if a.parent_lib and "c" not in skip:
        out["existing"] = existing(a)
    brief = {}
    if "tiling" in out:
        brief["tiling"] = {w: round(out["tiling"][w]["ratio"], 3) for w in ("prove", "verify")} | {
            "kernel_ms": out["tiling"]["kernel_ms"]}
    if "capability" in out:
        brief["capability"] = {n: {"prove": round(v["prove"]["median"], 1), "verify": round(v["verify"]["median"], 1),
                                   "kernel_ms": v["kernel_ms"]}
                               for n, v in out["capability"].items() if isinstance(v, dict) and "prove" in v}
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
