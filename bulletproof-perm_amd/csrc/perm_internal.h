// Permutation proof: what the prover (perm_prove.hip), the verifier
// (perm_verify.hip) and the C ABI (perm_api.hip) share -- the proof and its
// wire format, the verification job, and the functions the ABI calls.
// Every block of the namespace is opened hidden (namespace perm_impl
// BPP_HIDDEN): none of it reaches the shared object's dynamic symbol table.
#pragma once
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "ctx.h"
#include "gens.h"
#include "host/par.h"
#include "host/perm.h"
#include "ipa.h"
#include "msm_engine.h"

#define BPP_HIDDEN __attribute__((visibility("hidden")))

namespace perm_impl BPP_HIDDEN {

using hsc::Sc;

struct Proof {
  std::vector<Enc32> V;
  Enc32 AI, AO, S, T[5];
  Sc tau_x, mu, t_hat;
  IpaProofHost ipa;
  std::vector<uint32_t> pi;  // prover side only
};

// Proof layout (bpp_perm_proof_len): A_I A_O S T1 T3 T4 T5 T6 | tau_x mu
// t_hat | (L_j R_j) x lg | a b; the V commitments travel beside it.
inline void serialize(const perm::Circuit& C, const Proof& P, uint8_t* out) {
  auto put = [&](const void* p32) {  // (a canonical Sc is its 32 bytes)
    memcpy(out, p32, 32);
    out += 32;
  };
  for (const Enc32* e : {&P.AI, &P.AO, &P.S, &P.T[0], &P.T[1], &P.T[2], &P.T[3], &P.T[4]}) put(e->data());
  for (const Sc* s : {&P.tau_x, &P.mu, &P.t_hat}) put(s->v);
  for (uint32_t j = 0; j < C.lg; ++j) {
    put(P.ipa.L[j].data());
    put(P.ipa.R[j].data());
  }
  put(P.ipa.a.v);
  put(P.ipa.b.v);
}

inline bool deserialize(const perm::Circuit& C, const uint8_t* in, size_t len, const uint8_t* V, Proof& P) {
  if (len != perm::proof_len(C)) return false;
  size_t o = 0;
  auto pt = [&](Enc32& e) {
    memcpy(e.data(), in + o, 32);
    o += 32;
  };
  auto sc = [&](Sc& s) {
    bool ok = hsc::from_canonical(s, in + o);
    o += 32;
    return ok;
  };
  for (Enc32* e : {&P.AI, &P.AO, &P.S, &P.T[0], &P.T[1], &P.T[2], &P.T[3], &P.T[4]}) pt(*e);
  if (!sc(P.tau_x) || !sc(P.mu) || !sc(P.t_hat)) return false;
  P.ipa.L.resize(C.lg);
  P.ipa.R.resize(C.lg);
  for (uint32_t j = 0; j < C.lg; ++j) {
    pt(P.ipa.L[j]);
    pt(P.ipa.R[j]);
  }
  if (!sc(P.ipa.a) || !sc(P.ipa.b)) return false;
  P.V.resize(C.m);
  for (uint32_t j = 0; j < C.m; ++j) memcpy(P.V[j].data(), V + 32 * j, 32);
  return true;
}

// The proof's points in the order of its MSM scalars (verify_expand) -> out.
inline void proof_points(const Proof& P, uint8_t* out) {
  auto add = [&](const Enc32& e) {
    memcpy(out, e.data(), 32);
    out += 32;
  };
  for (auto& v : P.V) add(v);
  add(P.AI);
  add(P.AO);
  add(P.S);
  for (int i = 0; i < 5; ++i) add(P.T[i]);
  for (auto& l : P.ipa.L) add(l);
  for (auto& r : P.ipa.R) add(r);
}

// A caller's array of canonical scalars, [P][per] x 32 bytes (p = nullptr: none).
struct ScalarRows {
  const uint8_t* p = nullptr;
  uint32_t per = 0;
  const uint8_t* at(size_t i) const { return p + i * 32 * (size_t)per; }
  size_t bytes(size_t P) const { return p ? P * 32 * (size_t)per : 0; }
};

// The witness a caller hands the prover in place of the seed's own: this
// batch's rows of the caller's arrays, validated by the entry point.
//   statement                        perms  values      aux    gammas  pub
//   two-half shuffle (perm::build)   [k]    k cards     -      2k      -
//   deck (perm::build_deck)          [k]    - (C.cards) -      k       -
//   circuit (C.program)              -      m_in (v)    n_aux  m_in    n_pub
// gammas: the blindings of V_0..V_{nv-1}, drawn when there are none.
struct ProveInputs {
  const uint32_t* perms = nullptr;  // [P][n_perm], each a bijection on [0, n_perm)
  uint32_t n_perm = 0;
  ScalarRows values, aux, gammas, pub;
  size_t first = 0;  // the batch's first proof in the caller's call (error messages)

  // the same from the batch's proof b on
  ProveInputs slice(size_t b) const {
    ProveInputs s = *this;
    if (perms) s.perms += b * (size_t)n_perm;
    for (ScalarRows* r : {&s.values, &s.aux, &s.gammas, &s.pub})
      if (r->p) r->p = r->at(b);
    s.first += b;
    return s;
  }
};

// One batch's staged upload ("pb_rng_in", one copy): the draw templates [P][7]
// u64 and pi [P][k] u32, then -- with inputs, 32-byte aligned: the kernels read
// them with 16-byte loads -- values, aux, gammas and pub (public, wiped with the
// secrets all the same).  Offsets in bytes, computed here once.
struct StageLayout {
  struct Rows {
    ScalarRows src;  // the caller's
    size_t off = 0, bytes = 0;
    void stage(uint8_t* base, size_t i) const {  // proof i's row into the staging buffer
      if (src.p) memcpy(base + off + i * 32 * (size_t)src.per, src.at(i), 32 * (size_t)src.per);
    }
    const uint32_t* dev(const void* base) const {  // the uploaded rows
      return src.p ? (const uint32_t*)((const uint8_t*)base + off) : nullptr;
    }
  };
  size_t tmpl = 0, tmpl_bytes, pi, pi_bytes, pad, pad_bytes;
  Rows values, aux, gammas, pub;
  size_t bytes;
  StageLayout(size_t P, uint32_t k, const ProveInputs* in) {
    tmpl_bytes = P * 7 * sizeof(uint64_t);
    pi = tmpl_bytes;
    pi_bytes = P * 4 * (size_t)k;
    pad = bytes = pi + pi_bytes;
    if (in) bytes = (bytes + 31) & ~(size_t)31;
    pad_bytes = bytes - pad;
    auto place = [&](Rows& r, const ScalarRows& src) {
      r.src = src;
      r.off = bytes;
      r.bytes = src.bytes(P);
      bytes += r.bytes;
    };
    if (in) {
      place(values, in->values);
      place(aux, in->aux);
      place(gammas, in->gammas);
      place(pub, in->pub);
    }
  }
};

// One proof's Fiat-Shamir challenges (verify_replay).
struct VerifyChallenges {
  Sc x_perm, y, z, x, w, r;
  std::vector<Sc> u;  // IPA round challenges
};

// "the generators cover the padded circuit"
inline int gens_cover(bpp_ctx* ctx, const bpp_gens* G, uint32_t n_p) {
  if (G->n >= n_p) return BPP_OK;
  ctx->err = "generators shorter than the padded circuit";
  return BPP_ERR_LEN;
}

// --- steps every batch verifier takes (perm_verify.hip verify_batch and
// verify_groups, reshuffle_api.hip), each stated once

using h25519::is_identity;  // "the MSM's result is the identity"

// "the OS gave no randomness" (perm::os_entropy, perm::verify_seed)
inline int no_entropy(bpp_ctx* ctx) {
  ctx->err = "getrandom failed";
  return BPP_ERR_DEVICE;
}
// the verifier's own randomness for the batch weights
inline int verify_seed_or_err(bpp_ctx* ctx, uint8_t seed[32]) {
  return perm::verify_seed(seed) ? BPP_OK : no_entropy(ctx);
}

// Proofs per pass of a fallback's per-proof MSMs (TP terms each, c-bit
// windows): the multi-MSM engine packs T W below 2^32 and keeps M W 2^(c-1)
// buckets (2^22 terms; 2^24 buckets of P3_BYTES = 2.5 GiB).  May be 0: the
// caller clamps.
inline size_t each_pass_proofs(size_t TP, uint32_t c) {
  const size_t W = (254 + c - 1) / c;
  return std::min(((size_t)1 << 22) / TP, ((size_t)1 << 24) / (W << (c - 1)));
}

// "ok_out never keeps a pass of a call that fails": zeroed on entry
// (ok_clear), and again when the call ends with anything but BPP_OK or
// BPP_ERR_VERIFY (ok_settle, around the call).  ok_out == nullptr: no verdicts.
inline void ok_clear(uint8_t* ok_out, size_t n) {
  if (ok_out && n) memset(ok_out, 0, n);
}
inline int ok_settle(int rc, uint8_t* ok_out, size_t n) {
  if (rc != BPP_OK && rc != BPP_ERR_VERIFY) ok_clear(ok_out, n);
  return rc;
}

// The report of a fallback that has filled ok_out [total] after a batch check
// did not pass: how many proofs failed and the first of them, BPP_ERR_VERIFY.
// No failing proof (every proof passes alone, yet the weighted sum did not:
// not reachable for sums of group elements): no pass is reported.
inline int each_report(bpp_ctx* ctx, uint8_t* ok_out, size_t total) {
  size_t bad = 0, first = total;
  for (size_t p = total; p-- > 0;)
    if (!ok_out[p]) {
      ++bad;
      first = p;
    }
  if (!bad) {
    memset(ok_out, 0, total);
    ctx->err = "the batch check failed but no single proof did";
    return BPP_ERR_DEVICE;
  }
  ctx->err = std::to_string(bad) + " of " + std::to_string(total) + " proofs failed, the first at index " +
             std::to_string(first);
  return BPP_ERR_VERIFY;
}

}  // namespace perm_impl

// A batch verification split into its host replay (begin) and its weighted
// MSM (partial), so that the MSM can be partitioned over GPUs: by bucket
// windows (every rank holds every proof) or by proofs (each rank holds a
// slice; only the r challenges are exchanged before the MSM).
struct bpp_verify_job {
  perm::Circuit C;
  size_t count = 0, npt = 0;
  std::vector<perm_impl::Proof> Ps;
  std::vector<hsc::Sc> rs;                      // per-proof weight challenges
  std::vector<perm_impl::VerifyChallenges> ch;  // every proof's transcript challenges
  // unweighted generator / proof-point scalars, expanded on the host only
  // when asked for (bpp_perm_verify_scalars); the GPU path expands them on
  // the device (k_verify_scalars)
  mutable std::mutex mu;
  mutable bool expanded = false;
  mutable std::vector<std::vector<hsc::Sc>> gen_p, pt_p;
  // device job (bpp_perm_verify_begin_dev): the replay ran on the GPU and the
  // records / decompressed proof points sit in dctx's "vj_*" workspaces
  // (generation dgen); Ps and ch stay empty.  An asynchronous begin
  // (verify_batch) leaves the replay's verdicts in bad_h (pinned, rcount
  // words) for the partial to check after its own synchronisation.
  const uint32_t* bad_h = nullptr;
  bool dev = false;
  bpp_ctx* dctx = nullptr;
  uint64_t dgen = 0;
  // sliced device job: all `count` proofs uploaded and their points
  // decompressed, only [rfirst, rfirst + rcount) replayed (records and rs of
  // that slice); a whole job has rcount = count.  (The sharded path,
  // bpp_perm_verify_partial_sharded, takes one whole job per slice.)
  size_t rfirst = 0, rcount = 0;
  // a circuit with public inputs: the batch's [count][n_pub][8] words in dctx's
  // "vj_pub" workspace, read by the replay and by k_verify_scalars_pub
  const uint32_t* d_pub = nullptr;
};

// A compiled caller-defined circuit (circuit_api.hip bpp_circuit_create_pub).
struct bpp_circuit {
  perm::Circuit C;  // (C.program: the compiled program)
};

namespace perm_impl BPP_HIDDEN {

// --- prover (perm_prove.hip)
int prove_batch(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const std::vector<perm::Seed>& seeds,
                const uint8_t* label, size_t llen, std::vector<Proof>& Ps, const ProveInputs* in = nullptr);
int prove_batch_api(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const std::vector<perm::Seed>& seeds,
                    const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out, bool wipe = false,
                    const ProveInputs* in = nullptr);
int prove_batch_entropy(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, size_t count, const uint8_t* seeds32,
                        const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out,
                        const ProveInputs* in = nullptr);
int prove_wipe(bpp_ctx* ctx);
int secret_residue(bpp_ctx* ctx, uint64_t* nz);

// --- verifier (perm_verify.hip)
int verify_begin(const perm::Circuit& C, const uint8_t* label, size_t llen, size_t count, const uint8_t* proofs,
                 size_t proof_stride, const uint8_t* V, std::unique_ptr<bpp_verify_job>& job);
int verify_begin_dev(bpp_ctx* ctx, const perm::Circuit& C, const uint8_t* label, size_t llen, size_t count,
                     const uint8_t* proofs, const uint8_t* V, std::unique_ptr<bpp_verify_job>& job, size_t rfirst = 0,
                     size_t rcount = SIZE_MAX, bool sync = true, bool each = false, const uint8_t* pub = nullptr);
// ok_out: nullptr (one verdict for the batch), or [count] per-proof verdicts.
// pub: [count][C.n_pub] canonical scalars (checked by the entry point), the
// proofs' public inputs; not read when C.n_pub = 0
int verify_batch(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const uint8_t* label, size_t llen,
                 size_t count, const uint8_t* proofs, const uint8_t* V, uint8_t* ok_out,
                 const uint8_t* pub = nullptr);
// One group of a mixed batch (bpp_verify_groups): count proofs of statement C
// (kept by the caller for the call) under one label, with the arrays
// verify_batch takes.
struct VerifyGroup {
  const perm::Circuit* C;
  const uint8_t* label;
  size_t llen, count;
  const uint8_t *proofs, *V, *pub;
};
// ok_out: nullptr, or [sum of counts] per-proof verdicts in group order
int verify_groups(bpp_ctx* ctx, const bpp_gens* G, const VerifyGroup* groups, size_t n, uint8_t* ok_out);
int verify_partial(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job& J, const uint8_t seed[32], size_t first,
                   uint32_t wb, uint32_t we, h25519::ge* out);
int verify_partial_dev(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job& J, const uint8_t seed[32], size_t first,
                       uint32_t wb, uint32_t we, h25519::ge* out);
int verify_partial_sharded_dev(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job& J, size_t first,
                               const uint8_t* d_blocks, size_t stride, const uint8_t* d_pblocks, size_t pstride,
                               const size_t* counts, size_t nslices, uint32_t wb, uint32_t we, h25519::ge* out);
int verify_slice_scalars_dev(bpp_ctx* ctx, const bpp_verify_job& J, const uint8_t seed[32], size_t first,
                             uint32_t* d_out);
int verify_slice_points_dev(bpp_ctx* ctx, const bpp_verify_job& J, void* d_out);
size_t verify_terms(const bpp_verify_job& J);
int verify_terms_weighted(const bpp_verify_job& J, const uint8_t seed[32], size_t first, std::vector<Sc>& sc,
                          std::vector<uint8_t>& enc);

// --- argument checks the C ABI's entry points share (perm_api.hip,
// circuit_api.hip).  They look at the caller's arrays alone, so the provers run
// them before the context's and the generators' null checks.

// bad[p] = BPP_ERR_ARG where perms[p] ([count][k]) is no bijection on [0, k)
inline void check_perms(const uint32_t* perms, size_t count, uint32_t k, std::vector<int>& bad) {
  par::for_each(count, [&](size_t p) {
    std::vector<uint8_t> seen(k, 0);
    const uint32_t* pm = perms + p * (size_t)k;
    for (uint32_t i = 0; i < k; ++i) {
      if (pm[i] >= k || seen[pm[i]]) {
        bad[p] = BPP_ERR_ARG;
        return;
      }
      seen[pm[i]] = 1;
    }
  });
}

// bad[p] = BPP_ERR_NONCANONICAL where one of proof p's scalars (ptr
// [count][per_proof] x 32 bytes; nullptr: none to check) is >= l; a proof
// already refused keeps its code and is not read
inline void check_canonical(const uint8_t* ptr, size_t per_proof, size_t count, std::vector<int>& bad) {
  if (!ptr) return;
  par::for_each(count, [&](size_t p) {
    if (bad[p] != BPP_OK) return;
    Sc t;
    for (size_t i = 0; i < per_proof; ++i)
      if (!hsc::from_canonical(t, ptr + (p * per_proof + i) * 32)) bad[p] = BPP_ERR_NONCANONICAL;
    t = hsc::zero();
  });
}

// the first proof refused with `code` (0: with any), or SIZE_MAX
inline size_t first_bad(const std::vector<int>& bad, int code = 0) {
  for (size_t p = 0; p < bad.size(); ++p)
    if (code ? bad[p] == code : bad[p] != BPP_OK) return p;
  return SIZE_MAX;
}

// --- the statements' own refusals, shared by the per-kind entry points and
// bpp_verify_groups

// "k is in range"
inline bool k_in_range(uint32_t k) { return k >= 2 && k <= (1u << 20); }

// "every deck card is a canonical scalar" (deck == nullptr: 1..k)
inline int deck_canonical(bpp_ctx* ctx, uint32_t k, const uint8_t* deck) {
  Sc t;
  for (uint32_t i = 0; deck && i < k; ++i)
    if (!hsc::from_canonical(t, deck + 32 * (size_t)i)) {
      if (ctx) ctx->err = "deck card " + std::to_string(i) + " is not a canonical scalar";
      return BPP_ERR_NONCANONICAL;
    }
  return BPP_OK;
}

// "every public scalar of the call is canonical", and a circuit with public
// inputs was given them: what the _pub entry points check before any device
// work (bad: the first proof with a scalar >= l)
inline int pub_check(const bpp_circuit* c, size_t count, const uint8_t* pub, size_t* bad) {
  const uint32_t n_pub = c->C.n_pub;
  if (!n_pub || !count) return BPP_OK;
  if (!pub) return BPP_ERR_ARG;
  std::vector<int> nc(count, BPP_OK);
  check_canonical(pub, n_pub, count, nc);
  *bad = first_bad(nc);
  return *bad == SIZE_MAX ? BPP_OK : BPP_ERR_NONCANONICAL;
}

// One call of bpp_*_verify (count = 1), _verify_batch or _verify_batch_each
// (each: ok_out [count], where no pass is ever left behind by a call that fails).
struct VerifyCall {
  bpp_ctx* ctx;
  const bpp_gens* G;
  const uint8_t* label;
  size_t llen, count;
  const uint8_t *proofs, *V;
  const uint8_t* pub = nullptr;  // [count][n_pub] (verify_batch)
  bool each = false;
  uint8_t* ok_out = nullptr;
};

// What every such entry point does, in the order its refusals win: the
// arguments (stmt_ok: the statement's own, "k is in range" or "the circuit is
// not null"), the statement's refusals (pre(): a non-canonical deck card or
// public input), an empty batch, a single proof of the wrong length (len_ok),
// the device; then the verifier on the circuit that build() returns.
template <class Pre, class Build>
int verify_entry(const VerifyCall& a, bool stmt_ok, bool len_ok, Pre&& pre, Build&& build) {
  uint8_t* const ok_out = a.each ? a.ok_out : nullptr;
  ok_clear(ok_out, a.count);
  bpp_ctx* const ctx = a.ctx;  // (BPP_HIP names it)
  const int rc = bpp_guard(ctx, [&]() -> int {
    if (!ctx || !a.G || ((!a.proofs || !a.V || (a.each && !a.ok_out)) && a.count) || (!a.label && a.llen) || !stmt_ok)
      return BPP_ERR_ARG;
    BPP_TRY(pre());
    if (!a.count) return BPP_OK;
    if (!len_ok) return BPP_ERR_VERIFY;
    // (the context's own spin: the verifier's waits already spin where they
    // sit on the critical path (ctx_sync_latency), and syncs that spin 300 us
    // before sleeping measured within noise, profiles/r06_sync_spin_ab.txt)
    BPP_HIP(hipSetDevice(ctx->device));
    const perm::Circuit& C = build();
    return verify_batch(a.ctx, a.G, C, a.label, a.llen, a.count, a.proofs, a.V, ok_out, a.pub);
  });
  return ok_settle(rc, ok_out, a.count);
}
inline int no_refusal() { return BPP_OK; }

}  // namespace perm_impl
