"""One pass of the parent-commit gate for one tree (its own package and
library), as one JSON line: per entry the median of 5 windows in proofs/s, the
calls per window, and the work of ONE call -- ctx.work()'s delta and the
launches per profiled stage (Context.profile).  The entries:

    verify                  bpp_perm_verify_batch, 52 cards x 4096
    prove_circuit_two_half  bpp_circuit_prove_batch, two_half_shuffle(52) x 384
    verify_pub              bpp_circuit_verify_batch_pub, shuffle_of_public(52) x 4096
    verify_groups           bpp_verify_groups, four kinds x 1024 (tools/groups_cost.py's wide mix)
    reshuffle_verify        bpp_reshuffle_verify_batch, 52 cards x 4096
    verify_each_one_bad     bpp_perm_verify_batch_each, 52 cards x 4096, one tampered proof (the fallback)
    reshuffle_prove         bpp_reshuffle_prove_batch, 52 cards x 384
    masked_reshuffle_prove  bpp_masked_reshuffle_prove_batch, 52 cards x 384
    masked_reshuffle_verify bpp_masked_reshuffle_verify_batch, 52 cards x 4096
    reshuffle_verify_each_one_bad, masked_reshuffle_verify_each_one_bad
                            the two kinds' _verify_batch_each, 52 cards x 4096, one proof's z_0 with its
                            lowest bit flipped (the sigma fallback)

    python tools/gate_pass.py TREE

TREE: a checkout with its built library (this one: `.`; the parent commit's: a
`git archive` of it, built).  The gate runs this in alternating fresh processes
(parent, this, parent, this, ...), three passes a side, and asks that every
entry's median over this tree's passes be at or above the parent's lowest pass,
and that the work of one call be equal on both sides, entry by entry
(profiles/verify_once_gate_ab.json).  A window is as many calls as fill about a
second (0.2-second windows moved by several per cent between processes,
profiles/reshuffle_gate_ab.json)."""
import ctypes as C, json, random, re, sys, time
from pathlib import Path
ROOT = Path(sys.argv[1]).resolve()
sys.path.insert(0, str(ROOT / "bulletproof-perm_amd"))
import bpperm
from bpperm import check, gadgets as gd
sys.path.append(str(Path(__file__).resolve().parent))
from groups_cost import Kind  # (after bpperm: the statements' marshalling, over TREE's package)
K, B, NV, W = 52, 384, 4096, 5
L = 2**252 + 27742317777372353535851937790883648493
ctx = bpperm.Context(0); gens = bpperm.Gens(ctx, 128); lib = ctx.lib; label = b"bp-perm"
rnd = random.Random(7); sb = lambda x: (x % L).to_bytes(32, "little")
# every stage name TREE's sources could profile under (an unknown name reads as 0 launches)
STAGES = sorted({s for p in (ROOT / "bulletproof-perm_amd" / "csrc").glob("*.hip")
                 for s in re.findall(r'"([a-z][a-z0-9_]+)"', p.read_text())})
# perm verify
pl = lib.bpp_perm_proof_len(K)
ppf, pV = C.create_string_buffer(pl * NV), C.create_string_buffer(32 * (2 * K + 1) * NV)
sd = (C.c_uint64 * NV)(*range(1, NV + 1))
check(lib.bpp_perm_prove_batch(ctx.h, gens.h, K, NV, sd, label, len(label), ppf, pV), "prove", ctx.h)
def verify(): check(lib.bpp_perm_verify_batch(ctx.h, gens.h, K, NV, label, len(label), ppf, pV), "verify", ctx.h)
# the same batch, proof 1000 with t_hat's lowest bit flipped: every proof's own MSM
bpf, ok = C.create_string_buffer(ppf.raw, pl * NV), C.create_string_buffer(NV)
bpf[1000 * pl + 10 * 32] = bytes([ppf.raw[1000 * pl + 10 * 32] ^ 1])
def verify_each_bad():
    rc = lib.bpp_perm_verify_batch_each(ctx.h, gens.h, K, NV, label, len(label), bpf, pV, ok)
    assert rc == 6 and ok.raw.count(b"\0") == 1 and ok.raw[1000] == 0, rc
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
# mixed batch: 1024 proofs each of four kinds
kinds = [Kind(bpperm, gens, rnd, n, 1024) for n in ("perm", "deck", "member_of_public", "in_range")]
garr = (bpperm._VerifyGroupC * len(kinds))()
for k, g in zip(kinds, garr): k.fill(g)
def verify_groups(): check(lib.bpp_verify_groups(ctx.h, gens.h, garr, len(kinds)), "groups", ctx.h)
# blind re-shuffle: one committed deck, 4096 shuffles of it
rs = bpperm.Reshuffler(gens, K)
rdeck = b"".join(gens.pedersen_commit([sb(10 + i) for i in range(K)], [sb(rnd.randrange(L)) for _ in range(K)]))
rin = rdeck * NV
rout, rpf = rs.shuffle_batch(rin, [rnd.sample(range(K), K) for _ in range(NV)], seeds32=rnd.randbytes(32 * NV), raw=True)
def reshuffle_verify(): check(lib.bpp_reshuffle_verify_batch(ctx.h, gens.h, K, NV, label, len(label), rin, rout, rpf), "rverify", ctx.h)
# .. the same batch, proof 1000 with z_0's lowest bit flipped: every proof's own sigma MSM
def one_bad(pf, pl, z0): return pf[:1000 * pl + z0] + bytes([pf[1000 * pl + z0] ^ 1]) + pf[1000 * pl + z0 + 1:]
def each_bad(fn, *args):
    def f():
        rc = fn(ctx.h, gens.h, K, NV, *args, ok)
        assert rc == 6 and ok.raw.count(b"\0") == 1 and ok.raw[1000] == 0, rc
    return f
rbad = one_bad(rpf, rs.proof_len, 32 * (3 * K + 1))
reshuffle_each_bad = each_bad(lib.bpp_reshuffle_verify_batch_each, label, len(label), rin, rout, rbad)
# .. and its prover: 384 shuffles of the deck, the scalars r_i drawn from fixed seeds
rperms = (C.c_uint32 * (K * B))(*[i for _ in range(B) for i in rnd.sample(range(K), K)])
rseeds = rnd.randbytes(32 * B)
rout_b, rpf_b = C.create_string_buffer(32 * K * B), C.create_string_buffer(rs.proof_len * B)
def reshuffle_prove(): check(lib.bpp_reshuffle_prove_batch(ctx.h, gens.h, K, B, rin, rperms, None, rseeds, label, len(label), rout_b, rpf_b), "rprove", ctx.h)
# masked re-shuffle: the open deck over the same points under a committed point as the key, 4096 shuffles of it
ms = bpperm.MaskedReshuffler(gens, K, gens.pedersen_commit([sb(9)], [sb(rnd.randrange(L))])[0])
mkey, mlen = ms.key, ms.proof_len
min_ = b"".join(bytes(32) + rdeck[32 * i:32 * i + 32] for i in range(K)) * NV
mout, mpf = ms.shuffle_batch(min_, [rnd.sample(range(K), K) for _ in range(NV)], seeds32=rnd.randbytes(32 * NV), raw=True)
def masked_reshuffle_verify(): check(lib.bpp_masked_reshuffle_verify_batch(ctx.h, gens.h, K, NV, mkey, label, len(label), min_, mout, mpf), "mverify", ctx.h)
masked_each_bad = each_bad(lib.bpp_masked_reshuffle_verify_batch_each, mkey, label, len(label), min_, mout,
                           one_bad(mpf, mlen, 32 * (3 * K + 2)))
mout_b, mpf_b = C.create_string_buffer(64 * K * B), C.create_string_buffer(mlen * B)
def masked_reshuffle_prove(): check(lib.bpp_masked_reshuffle_prove_batch(ctx.h, gens.h, K, B, mkey, min_, rperms, None, rseeds, label, len(label), mout_b, mpf_b), "mprove", ctx.h)
def one_call(f):
    """the work counters' delta and the launches per stage of one call"""
    w0 = ctx.work(); f(); w1 = ctx.work()
    ctx.profile(True); ctx.profile_reset(); f()
    launches = {s: n for s in STAGES for n in [ctx.profile_get(s)[1]] if n}
    ctx.profile(False)
    return {"work": {n: w1[n] - w0[n] for n in w1 if w1[n] != w0[n]}, "launches": launches}
def med(f, per):
    f(); f()
    t0 = time.perf_counter(); f(); f(); f()
    reps = max(1, round(3 / (time.perf_counter() - t0)))  # about a second a window
    out = []
    for _ in range(W):
        t0 = time.perf_counter()
        for _ in range(reps): f()
        out.append(reps * per / (time.perf_counter() - t0))
    return {"value": sorted(out)[W // 2], "calls_per_window": reps, **one_call(f)}
ENTRIES = (("verify", verify, NV), ("prove_circuit_two_half", prove_c, B), ("verify_pub", verify_pub, NV),
           ("verify_groups", verify_groups, NV), ("reshuffle_verify", reshuffle_verify, NV),
           ("verify_each_one_bad", verify_each_bad, NV), ("reshuffle_prove", reshuffle_prove, B),
           ("masked_reshuffle_prove", masked_reshuffle_prove, B), ("masked_reshuffle_verify", masked_reshuffle_verify, NV),
           ("reshuffle_verify_each_one_bad", reshuffle_each_bad, NV),
           ("masked_reshuffle_verify_each_one_bad", masked_each_bad, NV))
print(json.dumps({name: med(f, per) for name, f, per in ENTRIES}))
