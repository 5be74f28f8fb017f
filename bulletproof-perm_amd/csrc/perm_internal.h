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

// A caller-supplied shuffle (bpp_perm_prove_shuffle_batch, bpp_deck_prove_batch):
// this batch's slices of the caller's arrays, validated by the entry point.
// The circuit form (bpp_circuit_prove_batch; C.program set): v, aux, gammas and
// (bpp_circuit_prove_batch_pub) pub, no cards and no perms.
struct ShuffleIn {
  const uint8_t* cards;   // [P][k] canonical scalars; nullptr with the deck circuit (the deck is the circuit's)
  const uint32_t* perms;  // [P][k], each a bijection on [0, k)
  const uint8_t* gammas;  // nullptr (drawn), or [P][C.nv] canonical scalars
  const uint8_t* v = nullptr;    // [P][m_in] canonical scalars: the committed inputs
  const uint8_t* aux = nullptr;  // [P][n_aux] canonical scalars: the free gate sides' values
  const uint8_t* pub = nullptr;  // [P][n_pub] canonical scalars: the public inputs (nullptr when n_pub = 0)
  size_t first = 0;              // this slice's first proof in the caller's batch (error messages)
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

namespace perm_impl BPP_HIDDEN {

// --- prover (perm_prove.hip)
int prove_batch(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const std::vector<perm::Seed>& seeds,
                const uint8_t* label, size_t llen, std::vector<Proof>& Ps, const ShuffleIn* sh = nullptr);
int prove_batch_api(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const std::vector<perm::Seed>& seeds,
                    const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out, bool wipe = false,
                    const ShuffleIn* sh = nullptr);
int prove_batch_entropy(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, size_t count, const uint8_t* seeds32,
                        const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out,
                        const ShuffleIn* sh = nullptr);
int prove_wipe(bpp_ctx* ctx);
int secret_residue(bpp_ctx* ctx, uint64_t* nz);

// --- verifier (perm_verify.hip)
int verify_begin(const perm::Circuit& C, const uint8_t* label, size_t llen, size_t count, const uint8_t* proofs,
                 size_t proof_stride, const uint8_t* V, std::unique_ptr<bpp_verify_job>& job);
int verify_begin_dev(bpp_ctx* ctx, const perm::Circuit& C, const uint8_t* label, size_t llen, size_t count,
                     const uint8_t* proofs, const uint8_t* V, std::unique_ptr<bpp_verify_job>& job, size_t rfirst = 0,
                     size_t rcount = SIZE_MAX, bool sync = true, bool each = false, const uint8_t* pub = nullptr);
// pub: [count][C.n_pub] canonical scalars (checked by the entry point), the
// proofs' public inputs; not read when C.n_pub = 0
int verify_batch(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const uint8_t* label, size_t llen,
                 size_t count, const uint8_t* proofs, const uint8_t* V, const uint8_t* pub = nullptr);
int verify_batch_each(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const uint8_t* label, size_t llen,
                      size_t count, const uint8_t* proofs, const uint8_t* V, uint8_t* ok_out,
                      const uint8_t* pub = nullptr);
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

}  // namespace perm_impl
