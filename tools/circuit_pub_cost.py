"""Cost of per-proof public inputs (bpp_circuit_*_pub), and that they cost the
existing entry points nothing.

    python tools/circuit_pub_cost.py [--windows 5] [--parent-lib PATH] [--out profiles/circuit_pub_cost_ab.json]

1. The feature: shuffle_of_public(52) -- every proof over its own public deck,
   2k - 2 = 102 gates, n_p = 128 -- through bpp_circuit_prove_batch_pub /
   bpp_circuit_verify_batch_pub against bpp_deck_prove_batch /
   bpp_deck_verify_batch on ONE shared deck, the nearest existing statement (k -
   1 = 51 gates, n_p = 64).  One process, one context, buffers marshalled before
   the clock starts, interleaved timing windows (deck, public, deck, public,
   ...): proving in 384-proof batches one at a time, verifying 4096 proofs per
   call.  Reports both rates, their ratio (of the window medians), the windows'
   spread, and the stage times of the replay and scalar launches
   (verify_replay_dev: k_verify_replay_g; verify_scalars: k_verify_consts +
   k_verify_scalars* + k_verify_merge) of one more batch of each kind.
2. What exists (--parent-lib: the parent commit's libbpperm.so built to a second
   path): bpp_perm_verify_batch at 52 cards x 4096 proofs and one 384-proof
   bpp_circuit_prove_batch of two_half_shuffle(52), in fresh child processes
   that alternate between the two libraries (parent, this, parent, this), each
   timing its own windows.  within_parent_spread: this library's median lies
   inside the min..max of the parent's own windows over its processes.

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

K, B, NV, GENS = 52, 384, 4096, 128
L = 2**252 + 27742317777372353535851937790883648493
STAGES = ("witness_program", "witness_deck", "pb_rng", "pb_pedersen_V", "pb_pedersen_Vx_witness", "pb_msm_AI_AO_S",
          "pb_host_poly", "pb_pedersen_T_lr", "pb_ipa", "verify_upload", "verify_replay_dev", "verify_replay_post",
          "verify_decompress", "verify_scalars")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "windows": v}


def window(f, reps, per):
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return reps * per / (time.perf_counter() - t0)


def feature(a):
    import bpperm
    from bpperm import check, gadgets

    ctx = bpperm.Context(0)
    gens = bpperm.Gens(ctx, GENS)
    lib, label = ctx.lib, b"bp-perm"
    rnd = random.Random(5252)
    circ = bpperm.Circuit(gadgets.shuffle_of_public(K))
    assert (circ.n_pub, circ.m, circ.n_p) == (K, K + 1, 128)
    sc = lambda: rnd.randrange(L).to_bytes(32, "little")
    shared = [sc() for _ in range(K)]
    flat, vals, pubs = [], [], []
    for _ in range(NV):
        p = list(range(K))
        rnd.shuffle(p)
        flat += p
        deck = [sc() for _ in range(K)]  # this proof's own deck
        pubs.append(b"".join(deck))
        vals.append(b"".join(deck[i] for i in p))
    pm = (C.c_uint32 * (NV * K))(*flat)
    dbuf = C.c_char_p(b"".join(shared))
    vbuf, ubuf = C.c_char_p(b"".join(vals)), C.c_char_p(b"".join(pubs))
    dlen, plen, m = lib.bpp_deck_proof_len(K), circ.proof_len, K + 1
    dk_pf, dk_V = C.create_string_buffer(dlen * NV), C.create_string_buffer(32 * m * NV)
    pb_pf, pb_V = C.create_string_buffer(plen * NV), C.create_string_buffer(32 * m * NV)

    def prove_deck(n):
        check(lib.bpp_deck_prove_batch(ctx.h, gens.h, K, n, dbuf, pm, None, None, label, len(label), dk_pf, dk_V),
              "bpp_deck_prove_batch", ctx.h)

    def prove_pub(n):
        check(lib.bpp_circuit_prove_batch_pub(ctx.h, gens.h, circ.h, n, vbuf, None, ubuf, None, None, label, len(label),
                                              pb_pf, pb_V), "bpp_circuit_prove_batch_pub", ctx.h)

    def verify_deck():
        check(lib.bpp_deck_verify_batch(ctx.h, gens.h, K, NV, dbuf, label, len(label), dk_pf, dk_V),
              "bpp_deck_verify_batch", ctx.h)

    def verify_pub():
        check(lib.bpp_circuit_verify_batch_pub(ctx.h, gens.h, circ.h, NV, label, len(label), pb_pf, pb_V, ubuf),
              "bpp_circuit_verify_batch_pub", ctx.h)

    for _ in range(2):  # warmup: window tables, workspaces
        prove_deck(B)
        prove_pub(B)
    runs = {"prove_deck": [], "prove_public": [], "verify_deck": [], "verify_public": []}
    for _ in range(a.windows):
        runs["prove_deck"].append(window(lambda: prove_deck(B), a.prove_batches, B))
        runs["prove_public"].append(window(lambda: prove_pub(B), a.prove_batches, B))
    prove_deck(NV)  # the verifiers' inputs
    prove_pub(NV)
    verify_deck()
    verify_pub()
    for _ in range(a.windows):
        runs["verify_deck"].append(window(verify_deck, a.verify_calls, NV))
        runs["verify_public"].append(window(verify_pub, a.verify_calls, NV))
    out = {"shape": {"cards": K, "prove_batch": B, "verify_proofs": NV, "windows": a.windows,
                     "prove_batches_per_window": a.prove_batches, "verify_calls_per_window": a.verify_calls},
           "unit": "proofs/s",
           "yardstick": "bpp_deck_prove_batch / bpp_deck_verify_batch on one shared deck, same process, interleaved "
                        "windows",
           "public": {"gadget": "shuffle_of_public(52)", "n_p": circ.n_p, "Q": circ.Q, "m": circ.m,
                      "n_pub": circ.n_pub, "proof_bytes": circ.proof_len, "deck_proof_bytes": dlen}}
    for side in ("prove", "verify"):
        y, c = stats(runs[side + "_deck"]), stats(runs[side + "_public"])
        out[side] = {"deck": y, "public": c, "ratio": c["median"] / y["median"]}
    prof = {}
    for name, f in (("deck", lambda: (prove_deck(B), verify_deck())), ("public", lambda: (prove_pub(B), verify_pub()))):
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
    circ.close()
    gens.close()
    ctx.close()
    return out


def existing_child(a):
    """One library (BPP_LIB, or the tree's), raw C ABI only (the parent's has no
    _pub exports): windows of bpp_perm_verify_batch and of
    bpp_circuit_prove_batch(two_half_shuffle(52)); one JSON line."""
    from bpperm import _lib, gadgets
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args

    def ok(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {rc}")

    ctx, gens, circ = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(lib.bpp_ctx_create(0, C.byref(ctx)), "ctx")
    ok(lib.bpp_gens_create(ctx, GENS, C.byref(gens)), "gens")
    desc = gadgets.two_half_shuffle(K)
    u32a = lambda xs: (C.c_uint32 * len(xs))(*xs)
    keep = (u32a(desc.side_aux), u32a(desc.lc_off), u32a(desc.lc_var), b"".join(desc.lc_coef))

    class Desc(C.Structure):
        _fields_ = [("m_in", C.c_uint32), ("n_gates", C.c_uint32), ("n_aux", C.c_uint32), ("n_asserts", C.c_uint32),
                    ("side_aux", C.POINTER(C.c_uint32)), ("lc_off", C.POINTER(C.c_uint32)),
                    ("lc_var", C.POINTER(C.c_uint32)), ("lc_coef", C.c_char_p)]

    d = Desc(desc.m_in, desc.n_gates, desc.n_aux, desc.n_asserts, *keep)
    ok(lib.bpp_circuit_create(C.byref(d), C.byref(circ)), "circuit")
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

    def verify():
        ok(lib.bpp_perm_verify_batch(ctx, gens, K, NV, label, len(label), pf, V), "bpp_perm_verify_batch")

    def prove():
        ok(lib.bpp_circuit_prove_batch(ctx, gens, circ, B, vbuf, None, None, None, label, len(label), cpf, cV),
           "bpp_circuit_prove_batch")

    for _ in range(3):
        verify()
        prove()
    runs = {"verify": [], "prove": []}
    for _ in range(a.windows):
        runs["verify"].append(window(verify, a.verify_calls, NV))
        runs["prove"].append(window(prove, a.prove_batches, B))
    print("AB " + json.dumps(runs))
    lib.bpp_circuit_destroy(circ)
    lib.bpp_gens_destroy(gens)
    lib.bpp_ctx_destroy(ctx)


def existing(a):
    runs = {"parent": {"verify": [], "prove": [], "per_process": []}, "this": {"verify": [], "prove": [], "per_process": []}}
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
            for k in ("verify", "prove"):
                runs[side][k] += got[k]
    out = {"what": {"verify": "bpp_perm_verify_batch, 52 cards x 4096 proofs",
                    "prove": "bpp_circuit_prove_batch, two_half_shuffle(52), 384-proof batches one at a time"},
           "unit": "proofs/s", "processes_per_library": a.ab_rounds, "windows_per_process": a.windows}
    for k in ("verify", "prove"):
        p, t = stats(runs["parent"][k]), stats(runs["this"][k])
        out[k] = {"parent": p, "this": t, "ratio": t["median"] / p["median"],
                  "parent_spread": (p["max"] - p["min"]) / p["median"], "this_spread": (t["max"] - t["min"]) / t["median"],
                  "within_parent_spread": p["min"] <= t["median"] <= p["max"] or t["median"] >= p["max"]}
    out["per_process"] = {s: runs[s]["per_process"] for s in runs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--prove-batches", type=int, default=200, help="batches per proving window (about 1 s)")
    ap.add_argument("--verify-calls", type=int, default=500, help="calls per verifying window (about 1 s)")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libbpperm.so (part 2; skipped without it)")
    ap.add_argument("--ab-rounds", type=int, default=2, help="processes per library in part 2")
    ap.add_argument("--existing-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.existing_child:
        return existing_child(a)
    out = {"feature": feature(a)}
    if a.parent_lib:
        out["existing"] = existing(a)
    f = out["feature"]
    brief = {k: {"ratio": round(f[k]["ratio"], 3)} |
             {s: {q: round(f[k][s][q]) for q in ("median", "min", "max")} for s in ("deck", "public")}
             for k in ("prove", "verify")}
    brief["launch_ms"] = {s: {n: f["stage_profile_ms"][s].get(n) for n in ("verify_replay_dev", "verify_scalars")}
                          for s in ("deck", "public")}
    if a.parent_lib:
        brief["existing"] = {k: {q: out["existing"][k][q] for q in ("ratio", "parent_spread", "this_spread",
                                                                       "within_parent_spread")}
                             for k in ("verify", "prove")}
    print(json.dumps(brief))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
