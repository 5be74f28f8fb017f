"""One pass of the parent-commit gate for one tree (its own package and
library): the median of 5 windows of bpp_perm_verify_batch (52 cards x 4096),
bpp_circuit_prove_batch (two_half_shuffle(52) x 384) and
bpp_circuit_verify_batch_pub (shuffle_of_public(52) x 4096), proofs/s, as one
JSON line.

    python tools/gate_pass.py TREE

TREE: a checkout with its built library (this one: `.`; the parent commit's: a
`git archive` of it, built).  The gate runs this in alternating fresh processes
(parent, this, parent, this, ...), three passes a side, and asks that every
entry's median over this tree's passes be at or above the parent's lowest pass
(profiles/reshuffle_gate_ab.json)."""
import ctypes as C, json, random, sys, time
from pathlib import Path
ROOT = Path(sys.argv[1]).resolve()
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
import bpperm
from bpperm import check, gadgets as gd
K, B, NV, W = 52, 384, 4096, 5
L = 2**252 + 27742317777372353535851937790883648493
ctx = bpperm.Context(0); gens = bpperm.Gens(ctx, 128); lib = ctx.lib; label = b"bp-perm"
rnd = random.Random(7); sb = lambda x: (x % L).to_bytes(32, "little")
# perm verify
pl = lib.bpp_perm_proof_len(K)
ppf, pV = C.create_string_buffer(pl * NV), C.create_string_buffer(32 * (2 * K + 1) * NV)
sd = (C.c_uint64 * NV)(*range(1, NV + 1))
check(lib.bpp_perm_prove_batch(ctx.h, gens.h, K, NV, sd, label, len(label), ppf, pV), "prove", ctx.h)
def verify(): check(lib.bpp_perm_verify_batch(ctx.h, gens.h, K, NV, label, len(label), ppf, pV), "verify", ctx.h)
# circuit prove, two_half_shuffle(52)
c2 = bpperm.Circuit(gd.two_half_shuffle(K))
rows = []
for _ in range(B):
    cards = [rnd.randrange(L) for _ in range(K)]; p = list(range(K)); rnd.shuffle(p)
    rows.append(b"".join(sb(x) for x in cards + [cards[i] for i in p]))
v2 = C.c_char_p(b"".join(rows))
cpf, cV = C.create_string_buffer(c2.proof_len * B), C.create_string_buffer(32 * (2 * K + 1) * B)
def prove_c(): check(lib.bpp_circuit_prove_batch(ctx.h, gens.h, c2.h, B, v2, None, None, None, label, len(label), cpf, cV), "cprove", ctx.h)
# circuit verify pub, shuffle_of_public(52)
c3 = bpperm.Circuit(gd.shuffle_of_public(K))
deck = [[rnd.randrange(L) for _ in range(K)] for _ in range(NV)]
pub = C.c_char_p(b"".join(sb(x) for d in deck for x in d))
vals = []
for d in deck:
    p = list(range(K)); rnd.shuffle(p); vals.append(b"".join(sb(d[i]) for i in p))
v3 = C.c_char_p(b"".join(vals))
qpf, qV = C.create_string_buffer(c3.proof_len * NV), C.create_string_buffer(32 * (K + 1) * NV)
check(lib.bpp_circuit_prove_batch_pub(ctx.h, gens.h, c3.h, NV, v3, None, pub, None, None, label, len(label), qpf, qV), "pprove", ctx.h)
def verify_pub(): check(lib.bpp_circuit_verify_batch_pub(ctx.h, gens.h, c3.h, NV, label, len(label), qpf, qV, pub), "pverify", ctx.h)
def med(f, reps, per):
    f(); f()
    out = []
    for _ in range(W):
        t0 = time.perf_counter()
        for _ in range(reps): f()
        out.append(reps * per / (time.perf_counter() - t0))
    return sorted(out)[W // 2]
print(json.dumps({"verify": med(verify, 600, NV), "prove_circuit_two_half": med(prove_c, 200, B), "verify_pub": med(verify_pub, 500, NV)}))
