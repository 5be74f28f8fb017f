"""Cost of mixed batches (bpp_verify_groups) against the per-kind calls they
replace, and that they cost the existing entry points nothing.

    python tools/groups_cost.py [--windows 5] [--parent-lib PATH] [--out profiles/groups_cost_ab.json]

1. A table round at 52 cards: 1 deck proof (n_p = 64), 3 two-half re-shuffles
   (128), 8 opens_to (4), 4 member_of_public(13) (16), 4 in_range(16) (16), 2
   sum_equals(5) (4) -- one bpp_verify_groups call against the loop of six
   per-kind _verify_batch calls, one process, one context, buffers marshalled
   before the clock starts, interleaved timing windows (loop, groups, loop,
   ...).  ms per round: window medians with min-max.  not_slower: the merged
   call's median is at most the loop's median plus the loop's own window spread
   (max - min).  The stage times (Context.profile) of one more round of each
   kind are recorded either way.
2. A wide mix: 1024 proofs each of four kinds (two-half, deck,
   member_of_public(13), in_range(16)), the same comparison; the ratio is
   reported, parity expected (the saving is the shared generator terms).
3. What exists (--parent-lib: the parent commit's libbpperm.so built to a second
   path): bpp_perm_verify_batch, bpp_circuit_verify_batch_pub
   (shuffle_of_public(52)) and bpp_perm_verify_batch_each at 4096 x 52 cards, in
   fresh child processes that alternate between the two libraries (parent, this,
   parent, this), each timing its own windows.  within_parent_spread: this
   library's median lies inside the min..max of the parent's own windows over
   its processes (or is faster).

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

K, NV, GENS = 52, 4096, 128
L = 2**252 + 27742317777372353535851937790883648493
STAGES = ("verify_upload", "verify_replay", "verify_replay_dev", "verify_replay_post", "verify_decompress",
          "verify_terms", "verify_scalars", "verify_merge_groups", "msm_digits", "msm_count", "msm_scan", "msm_scatter",
          "msm_accumulate", "msm_fixup", "msm_reduce")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "windows": v}


def window_ms(f, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return (time.perf_counter() - t0) * 1e3 / reps


def sb(x):
    return (x % L).to_bytes(32, "little")


class Kind:
    """count valid proofs of one statement, marshalled: a per-kind verify_batch
    closure and the fields of its bpp_verify_group."""

    def __init__(self, bpperm, gens, rnd, name, count):
        from bpperm import gadgets as gd
        self.name, self.count = name, count
        self.pub = None
        sc = lambda: rnd.randrange(L)
        shuffled = lambda n: rnd.sample(range(n), n)
        if name == "perm":
            pr = bpperm.PermProver(gens, K)
            pf, V = pr.prove_batch_entropy(count, raw=True)
        elif name == "deck":
            pr = bpperm.DeckProver(gens, K)
            pf, V = pr.prove_batch([shuffled(K) for _ in range(count)], raw=True)
        else:
            desc = {"opens_to": gd.opens_to, "member_of_public": lambda: gd.member_of_public(13),
                    "in_range": lambda: gd.in_range(16), "sum_equals": lambda: gd.sum_equals(5),
                    "shuffle_of_public": lambda: gd.shuffle_of_public(K)}[name]()
            pr = bpperm.CircuitProver(gens, desc)
            vs, auxs, pubs = [], None, None
            for _ in range(count):
                if name == "opens_to":
                    x = sc()
                    v, u = [x], [x]
                elif name == "member_of_public":
                    u = [sc() for _ in range(13)]
                    v = [u[rnd.randrange(13)]]
                elif name == "in_range":
                    v, u = [rnd.randrange(2**16)], None
                    auxs = (auxs or []) + [b"".join(sb(h) for h in desc.aux_of(v))]
                elif name == "sum_equals":
                    v = [sc() for _ in range(5)]
                    u = [sum(v) % L]
                else:
                    u = [sc() for _ in range(K)]
                    v = [u[i] for i in shuffled(K)]
                vs.append(b"".join(sb(x) for x in v))
                if u is not None:
                    pubs = (pubs or []) + [b"".join(sb(x) for x in u)]
            pf, V = pr.prove_batch(vs, auxs, raw=True, pub=pubs)
            self.pub = b"".join(pubs) if pubs else None
        self.pr, self.pf, self.V = pr, pf, V
        self.n_p = pr.circuit.n_p if hasattr(pr, "circuit") else {"perm": 128, "deck": 64}[name]  # (52 cards)
        lib, ctx, g, lab = pr.ctx.lib, pr.ctx.h, gens.h, pr.label
        cp, cv, cu = C.c_char_p(pf), C.c_char_p(V), (C.c_char_p(self.pub) if self.pub else None)
        self._keep = (cp, cv, cu)
        if name == "perm":
            self.call = lambda: lib.bpp_perm_verify_batch(ctx, g, K, count, lab, len(lab), cp, cv)
        elif name == "deck":
            self.call = lambda: lib.bpp_deck_verify_batch(ctx, g, K, count, None, lab, len(lab), cp, cv)
        else:
            self.call = lambda: lib.bpp_circuit_verify_batch_pub(ctx, g, pr.circuit.h, count, lab, len(lab), cp, cv, cu)

    def fill(self, grp):
        pr = self.pr
        grp.label, grp.label_len, grp.count = pr.label, len(pr.label), self.count
        grp.proofs, grp.V, grp.pub = self.pf, self.V, self.pub
        if self.name == "perm":
            grp.kind, grp.k = 0, K
        elif self.name == "deck":
            grp.kind, grp.k = 1, K
        else:
            grp.kind, grp.circuit = 2, pr.circuit.h


def compare(bpperm, ctx, gens, kinds, a, reps):
    """loop of per-kind calls vs one bpp_verify_groups, interleaved windows -> dict"""
    arr = (bpperm._VerifyGroupC * len(kinds))()
    for k, grp in zip(kinds, arr):
        k.fill(grp)
    lib = ctx.lib

    def loop():
        for k in kinds:
            if k.call():
                raise RuntimeError(k.name)

    def groups():
        if lib.bpp_verify_groups(ctx.h, gens.h, arr, len(kinds)):
            raise RuntimeError("bpp_verify_groups")

    for _ in range(3):  # warmup: workspaces, group contexts, circuit uploads
        loop()
        groups()
    runs = {"loop": [], "groups": []}
    for _ in range(a.windows):
        runs["loop"].append(window_ms(loop, reps))
        runs["groups"].append(window_ms(groups, reps))
    lo, gr = stats(runs["loop"]), stats(runs["groups"])
    prof = {}
    for name, f in (("loop", loop), ("groups", groups)):
        ctx.profile(True)
        ctx.profile_reset()
        f()
        prof[name] = {}
        for s in STAGES:
            ms, n = ctx.profile_get(s)
            if n:
                prof[name][s] = {"ms": round(ms, 4), "launches": n}
        ctx.profile(False)
    w0 = ctx.work()
    groups()
    w1 = ctx.work()
    return {"unit": "ms per call of everything", "calls_per_window": reps, "loop": lo, "groups": gr,
            "ratio_groups_over_loop": gr["median"] / lo["median"], "loop_spread_ms": lo["max"] - lo["min"],
            "not_slower": gr["median"] <= lo["median"] + (lo["max"] - lo["min"]),
            "groups_msm_terms": w1["msm_terms"] - w0["msm_terms"], "stage_profile": prof,
            "kinds": [{"name": k.name, "count": k.count, "n_p": k.n_p} for k in kinds]}


def feature(a):
    import bpperm
    ctx = bpperm.Context(0)
    gens = bpperm.Gens(ctx, GENS)
    rnd = random.Random(5253)
    table = [Kind(bpperm, gens, rnd, n, c) for n, c in (("deck", 1), ("perm", 3), ("opens_to", 8),
                                                        ("member_of_public", 4), ("in_range", 4), ("sum_equals", 2))]
    out = {"table_round": compare(bpperm, ctx, gens, table, a, a.round_calls)}
    wide = [Kind(bpperm, gens, rnd, n, 1024) for n in ("perm", "deck", "member_of_public", "in_range")]
    out["wide_mix"] = compare(bpperm, ctx, gens, wide, a, a.wide_calls)
    gens.close()
    ctx.close()
    return out


def existing_child(a):
    """One library (BPP_LIB, or the tree's): windows of the three existing entry
    points at 4096 x 52 cards; one JSON line."""
    from bpperm import _lib
    probe = C.CDLL(str(_lib.LIB_PATH))
    for name in list(_lib.SIGNATURES):  # (the parent's library has no bpp_verify_groups)
        if not hasattr(probe, name):
            del _lib.SIGNATURES[name]
    import bpperm
    ctx = bpperm.Context(0)
    gens = bpperm.Gens(ctx, GENS)
    rnd = random.Random(52)
    perm, pub = Kind(bpperm, gens, rnd, "perm", NV), Kind(bpperm, gens, rnd, "shuffle_of_public", NV)
    lib, lab = ctx.lib, perm.pr.label
    ok = C.create_string_buffer(NV)
    cp, cv = perm._keep[0], perm._keep[1]

    def each():
        return lib.bpp_perm_verify_batch_each(ctx.h, gens.h, K, NV, lab, len(lab), cp, cv, ok)

    calls = {"perm_verify_batch": perm.call, "circuit_verify_batch_pub": pub.call, "perm_verify_batch_each": each}
    for f in calls.values():
        for _ in range(3):
            if f():
                raise RuntimeError("verify failed")
    runs = {k: [] for k in calls}
    for _ in range(a.windows):
        for k, f in calls.items():
            runs[k].append(window_ms(f, a.verify_calls))
    print("AB " + json.dumps(runs))
    gens.close()
    ctx.close()


def existing(a):
    names = ("perm_verify_batch", "circuit_verify_batch_pub", "perm_verify_batch_each")
    runs = {s: {k: [] for k in names} | {"per_process": []} for s in ("parent", "this")}
    for _ in range(a.ab_rounds):
        for side, path in (("parent", a.parent_lib), ("this", "")):
            env = {k: v for k, v in os.environ.items() if k != "BPP_LIB"}
            if path:
                env["BPP_LIB"] = str(Path(path).resolve())
            r = subprocess.run([sys.executable, __file__, "--existing-child", "--windows", str(a.windows),
                                "--verify-calls", str(a.verify_calls)], capture_output=True, text=True, env=env,
                               timeout=600)
            if r.returncode != 0:
                raise RuntimeError((r.stdout + r.stderr)[-3000:])
            got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1][3:])
            runs[side]["per_process"].append(got)
            for k in names:
                runs[side][k] += got[k]
    out = {"what": "4096 proofs x 52 cards per call; circuit_verify_batch_pub over shuffle_of_public(52)",
           "unit": "ms per call", "processes_per_library": a.ab_rounds, "windows_per_process": a.windows}
    for k in names:
        p, t = stats(runs["parent"][k]), stats(runs["this"][k])
        out[k] = {"parent": p, "this": t, "ratio": t["median"] / p["median"],
                  "parent_spread": (p["max"] - p["min"]) / p["median"], "this_spread": (t["max"] - t["min"]) / t["median"],
                  "within_parent_spread": t["median"] <= p["max"]}
    out["per_process"] = {s: runs[s]["per_process"] for s in runs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--round-calls", type=int, default=300, help="table rounds per window")
    ap.add_argument("--wide-calls", type=int, default=100, help="wide mixes per window")
    ap.add_argument("--verify-calls", type=int, default=150, help="calls per window in part 3")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libbpperm.so (part 3; skipped without it)")
    ap.add_argument("--ab-rounds", type=int, default=2, help="processes per library in part 3")
    ap.add_argument("--existing-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.existing_child:
        return existing_child(a)
    out = {"feature": feature(a)}
    if a.parent_lib:
        out["existing"] = existing(a)
    brief = {}
    for part in ("table_round", "wide_mix"):
        f = out["feature"][part]
        brief[part] = {s: {q: round(f[s][q], 4) for q in ("median", "min", "max")} for s in ("loop", "groups")} | {
            "ratio_groups_over_loop": round(f["ratio_groups_over_loop"], 3), "not_slower": f["not_slower"]}
    if a.parent_lib:
        brief["existing"] = {k: {q: out["existing"][k][q] for q in ("ratio", "parent_spread", "within_parent_spread")}
                             for k in ("perm_verify_batch", "circuit_verify_batch_pub", "perm_verify_batch_each")}
    print(json.dumps(brief))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
