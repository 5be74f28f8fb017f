// Permutation proof: the C ABI (bpp_perm_*, include/bpperm.h) -- argument checks, bpp_guard, the device
// selection, and marshalling to and from the caller's buffers.  The prover is perm_prove.hip, the verifier
// perm_verify.hip, what they share perm_internal.h.
#include <string>

#include "perm_internal.h"
#include "layout.h"

using namespace perm_impl;

extern "C" {

size_t bpp_perm_proof_len(uint32_t k) { return k_in_range(k) ? perm::proof_len(k) : 0; }

int bpp_perm_prove(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, uint64_t seed, const uint8_t* label, size_t llen,
                   uint8_t* proof_out, uint8_t* V_out, uint32_t* perm_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !G || !proof_out || !V_out || (!label && llen) || !k_in_range(k)) return BPP_ERR_ARG;
    const perm::Circuit C = perm::build(k);
    BPP_TRY(gens_cover(ctx, G, C.n_p));
    BPP_HIP(hipSetDevice(ctx->device));
    std::vector<Proof> Ps;
    BPP_TRY(prove_batch(ctx, G, C, {perm::Seed::u64(seed)}, label, llen, Ps));
    serialize(C, Ps[0], proof_out);
    for (uint32_t j = 0; j < C.m; ++j) memcpy(V_out + 32 * j, Ps[0].V[j].data(), 32);
    if (perm_out) memcpy(perm_out, Ps[0].pi.data(), 4 * k);
    return BPP_OK;
  });
}

int bpp_perm_prove_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint64_t* seeds,
                         const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !G || (!seeds && count) || ((!proofs_out || !V_out) && count) || (!label && llen) || !k_in_range(k))
      return BPP_ERR_ARG;
    std::vector<perm::Seed> sd(count);
    for (size_t i = 0; i < count; ++i) sd[i] = perm::Seed::u64(seeds[i]);
    return prove_batch_api(ctx, G, perm::build(k), sd, label, llen, proofs_out, V_out);
  });
}

int bpp_perm_prove_batch_entropy(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* seeds32,
                                 const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !G || ((!proofs_out || !V_out) && count) || (!label && llen) || !k_in_range(k))
      return BPP_ERR_ARG;
    return prove_batch_entropy(ctx, G, perm::build(k), count, seeds32, label, llen, proofs_out, V_out);
  });
}

int bpp_perm_prove_shuffle_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* cards,
                                 const uint32_t* perms, const uint8_t* gammas, const uint8_t* seeds32,
                                 const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (((!cards || !perms || !proofs_out || !V_out) && count) || (!label && llen) || !k_in_range(k))
      return BPP_ERR_ARG;
    // the whole witness is checked before any device work and before any
    // output byte is written: every perm a bijection on [0, k), every card
    // and supplied blinding a canonical scalar
    std::vector<int> bad(count, BPP_OK);
    check_perms(perms, count, k, bad);
    check_canonical(cards, k, count, bad);
    check_canonical(gammas, 2 * (size_t)k, count, bad);
    if (const size_t p = first_bad(bad); p != SIZE_MAX) {
      if (ctx)
        ctx->err = bad[p] == BPP_ERR_ARG ? "shuffle " + std::to_string(p) + ": perm is not a bijection on [0, k)"
                                         : "shuffle " + std::to_string(p) + ": non-canonical card or blinding";
      return bad[p];
    }
    if (!ctx || !G) return BPP_ERR_ARG;
    if (!count) return BPP_OK;
    ProveInputs in;
    in.perms = perms;
    in.n_perm = k;
    in.values = {cards, k};
    in.gammas = {gammas, 2 * k};
    return prove_batch_entropy(ctx, G, perm::build(k), count, seeds32, label, llen, proofs_out, V_out, &in);
  });
}

// --- the deck circuit (perm.h build_deck): V_0..V_{k-1} commit to a
// permutation of the call's PUBLIC deck

size_t bpp_deck_proof_len(uint32_t k) {
  if (!k_in_range(k)) return 0;
  uint32_t n_p = 4, lg = 2;  // n_p = max(4, next_pow2(k - 1))
  for (; n_p < k - 1; n_p *= 2) ++lg;
  return 32 * (8 + 3 + 2 * (size_t)lg + 2);
}

int bpp_deck_prove_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* deck,
                         const uint32_t* perms, const uint8_t* gammas, const uint8_t* seeds32, const uint8_t* label,
                         size_t llen, uint8_t* proofs_out, uint8_t* V_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (((!perms || !proofs_out || !V_out) && count) || (!label && llen) || !k_in_range(k)) return BPP_ERR_ARG;
    // the whole witness is checked before any device work and before any
    // output byte is written: every perm a bijection on [0, k), then every
    // deck card, then every supplied blinding a canonical scalar
    std::vector<int> bad(count, BPP_OK);
    check_perms(perms, count, k, bad);
    check_canonical(gammas, k, count, bad);
    if (const size_t p = first_bad(bad, BPP_ERR_ARG); p != SIZE_MAX) {
      if (ctx) ctx->err = "deck proof " + std::to_string(p) + ": perm is not a bijection on [0, k)";
      return BPP_ERR_ARG;
    }
    BPP_TRY(deck_canonical(ctx, k, deck));
    if (const size_t p = first_bad(bad); p != SIZE_MAX) {
      if (ctx) ctx->err = "deck proof " + std::to_string(p) + ": non-canonical blinding";
      return bad[p];
    }
    if (!ctx || !G) return BPP_ERR_ARG;
    if (!count) return BPP_OK;
    ProveInputs in;
    in.perms = perms;
    in.n_perm = k;
    in.gammas = {gammas, k};
    return prove_batch_entropy(ctx, G, perm::build_deck(k, deck), count, seeds32, label, llen, proofs_out, V_out, &in);
  });
}

int bpp_deck_verify(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, const uint8_t* deck, const uint8_t* label,
                    size_t llen, const uint8_t* proof, size_t proof_len, const uint8_t* V) {
  return verify_entry({ctx, G, label, llen, 1, proof, V}, k_in_range(k), proof_len == bpp_deck_proof_len(k),
                      [&] { return deck_canonical(ctx, k, deck); }, [&] { return perm::build_deck(k, deck); });
}

int bpp_deck_verify_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* deck,
                          const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V) {
  return verify_entry({ctx, G, label, llen, count, proofs, V}, k_in_range(k), true,
                      [&] { return deck_canonical(ctx, k, deck); }, [&] { return perm::build_deck(k, deck); });
}

int bpp_deck_verify_batch_each(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* deck,
                               const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                               uint8_t* ok_out) {
  return verify_entry({ctx, G, label, llen, count, proofs, V, nullptr, true, ok_out}, k_in_range(k), true,
                      [&] { return deck_canonical(ctx, k, deck); }, [&] { return perm::build_deck(k, deck); });
}

int bpp_debug_secret_residue(bpp_ctx* ctx, uint64_t* nonzero_bytes) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !nonzero_bytes) return BPP_ERR_ARG;
    BPP_HIP(hipSetDevice(ctx->device));
    BPP_TRY(ctx_sync(ctx));
    *nonzero_bytes = 0;
    return secret_residue(ctx, nonzero_bytes);
  });
}

int bpp_perm_verify(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, const uint8_t* label, size_t llen,
                    const uint8_t* proof, size_t proof_len, const uint8_t* V) {
  return verify_entry({ctx, G, label, llen, 1, proof, V}, k_in_range(k), proof_len == bpp_perm_proof_len(k), no_refusal,
                      [&] { return perm::build(k); });
}

int bpp_perm_verify_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* label, size_t llen,
                          const uint8_t* proofs, const uint8_t* V) {
  return verify_entry({ctx, G, label, llen, count, proofs, V}, k_in_range(k), true, no_refusal,
                      [&] { return perm::build(k); });
}

int bpp_perm_verify_batch_each(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* label,
                               size_t llen, const uint8_t* proofs, const uint8_t* V, uint8_t* ok_out) {
  return verify_entry({ctx, G, label, llen, count, proofs, V, nullptr, true, ok_out}, k_in_range(k), true, no_refusal,
                      [&] { return perm::build(k); });
}

int bpp_perm_verify_begin(uint32_t k, size_t count, const uint8_t* label, size_t llen, const uint8_t* proofs,
                          const uint8_t* V, uint8_t* r_out, bpp_verify_job** out) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!out || ((!proofs || !V) && count) || (!label && llen) || !k_in_range(k)) return BPP_ERR_ARG;
    *out = nullptr;
    const perm::Circuit C = perm::build(k);
    std::unique_ptr<bpp_verify_job> job;
    BPP_TRY(verify_begin(C, label, llen, count, proofs, perm::proof_len(k), V, job));
    if (r_out)
      for (size_t p = 0; p < count; ++p) hsc::to_bytes(r_out + 32 * p, job->rs[p]);
    *out = job.release();
    return BPP_OK;
  });
}

int bpp_perm_verify_begin_dev(bpp_ctx* ctx, uint32_t k, size_t count, const uint8_t* label, size_t llen,
                              const uint8_t* proofs, const uint8_t* V, uint8_t* r_out, bpp_verify_job** out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !out || ((!proofs || !V) && count) || (!label && llen) || !k_in_range(k)) return BPP_ERR_ARG;
    *out = nullptr;
    BPP_HIP(hipSetDevice(ctx->device));
    const perm::Circuit C = perm::build(k);
    std::unique_ptr<bpp_verify_job> job;
    BPP_TRY(verify_begin_dev(ctx, C, label, llen, count, proofs, V, job));
    if (r_out && count) memcpy(r_out, job->rs.data(), 32 * count);
    *out = job.release();
    return BPP_OK;
  });
}

int bpp_perm_verify_begin_dev_async(bpp_ctx* ctx, uint32_t k, size_t count, const uint8_t* label, size_t llen,
                                    const uint8_t* proofs, const uint8_t* V, bpp_verify_job** out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !out || ((!proofs || !V) && count) || (!label && llen) || !k_in_range(k)) return BPP_ERR_ARG;
    *out = nullptr;
    BPP_HIP(hipSetDevice(ctx->device));
    const perm::Circuit C = perm::build(k);
    std::unique_ptr<bpp_verify_job> job;
    BPP_TRY(verify_begin_dev(ctx, C, label, llen, count, proofs, V, job, 0, SIZE_MAX, false));
    *out = job.release();
    return BPP_OK;
  });
}

int bpp_perm_verify_terms(const bpp_verify_job* job, size_t* terms) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!job || !terms) return BPP_ERR_ARG;
    *terms = verify_terms(*job);
    return BPP_OK;
  });
}

int bpp_verify_seed(uint8_t seed[32]) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!seed) return BPP_ERR_ARG;
    return perm::verify_seed(seed) ? BPP_OK : BPP_ERR_DEVICE;
  });
}

int bpp_perm_verify_scalars(const bpp_verify_job* job, const uint8_t seed[32], size_t first, uint8_t* scalars_out,
                            uint8_t* points_out) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!job || !seed || !scalars_out || (!points_out && job->count)) return BPP_ERR_ARG;
    if (job->dev) return BPP_ERR_ARG;  // (a device job keeps no host replay to expand)
    std::vector<Sc> sc;
    std::vector<uint8_t> enc;
    BPP_TRY(verify_terms_weighted(*job, seed, first, sc, enc));
    for (size_t i = 0; i < sc.size(); ++i) hsc::to_bytes(scalars_out + 32 * i, sc[i]);
    if (!enc.empty()) memcpy(points_out, enc.data(), enc.size());
    return BPP_OK;
  });
}

size_t bpp_perm_verify_slice_bytes(const bpp_verify_job* job) {
  return job ? (2 * (size_t)job->C.n_p + 2 + job->rcount * job->npt) * 32 : 0;
}

int bpp_perm_verify_slice_scalars_at(bpp_ctx* ctx, const bpp_verify_job* job, const uint8_t seed[32], size_t first,
                                     void* d_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !job || !d_out || !seed || !job->dev || first > (1u << 26)) return BPP_ERR_ARG;
    BPP_HIP(hipSetDevice(ctx->device));
    return verify_slice_scalars_dev(ctx, *job, seed, first, (uint32_t*)d_out);
  });
}

size_t bpp_perm_verify_slice_point_bytes(const bpp_verify_job* job) {
  return job ? job->count * job->npt * MSM_NIELS_WORDS * 4 : 0;
}

int bpp_perm_verify_slice_points(bpp_ctx* ctx, const bpp_verify_job* job, void* d_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !job || (!d_out && job->count) || !job->dev) return BPP_ERR_ARG;
    BPP_HIP(hipSetDevice(ctx->device));
    return verify_slice_points_dev(ctx, *job, d_out);
  });
}

int bpp_perm_verify_partial_sharded(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job* job, size_t first,
                                    const void* d_blocks, size_t stride, const void* d_pblocks, size_t pstride,
                                    const size_t* counts, size_t nslices, uint32_t w_begin, uint32_t w_end,
                                    uint8_t partial[128]) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !G || !job || !partial || !job->dev || !nslices || !d_blocks || !d_pblocks || !counts)
      return BPP_ERR_ARG;
    size_t total = 0;
    for (size_t r = 0; r < nslices; ++r) total += counts[r];
    const uint32_t c = msm_choose_c((double)(2 * (size_t)job->C.n_p + 2 + total * job->npt));
    if (w_begin > w_end || w_end > (254 + c - 1) / c) return BPP_ERR_ARG;
    BPP_HIP(hipSetDevice(ctx->device));
    h25519::ge r = h25519::ge_identity();
    if (total)
      BPP_TRY(verify_partial_sharded_dev(ctx, G, *job, first, (const uint8_t*)d_blocks, stride,
                                         (const uint8_t*)d_pblocks, pstride, counts, nslices, w_begin, w_end, &r));
    h25519::ge_to_words((uint32_t*)partial, r);
    return BPP_OK;
  });
}

int bpp_perm_verify_partial(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job* job, const uint8_t seed[32],
                            size_t first, uint32_t w_begin, uint32_t w_end, uint8_t partial[128]) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !G || !job || !partial || !seed) return BPP_ERR_ARG;
    const uint32_t c = msm_choose_c((double)verify_terms(*job));
    if (w_begin > w_end || w_end > (254 + c - 1) / c) return BPP_ERR_ARG;
    BPP_HIP(hipSetDevice(ctx->device));
    h25519::ge r = h25519::ge_identity();
    if (job->count) {
      if (job->dev)
        BPP_TRY(verify_partial_dev(ctx, G, *job, seed, first, w_begin, w_end, &r));
      else
        BPP_TRY(verify_partial(ctx, G, *job, seed, first, w_begin, w_end, &r));
    }
    h25519::ge_to_words((uint32_t*)partial, r);
    return BPP_OK;
  });
}

void bpp_perm_verify_end(bpp_verify_job* job) { delete job; }

int bpp_partials_is_identity(const uint8_t* partials, size_t count) {
  return bpp_guard(nullptr, [&]() -> int {
    uint8_t e[32];
    const int rc = bpp_partials_finish(partials, count, e);
    if (rc == BPP_ERR_ARG && partials) return BPP_ERR_VERIFY;  // a partial with Z = 0: never a pass
    BPP_TRY(rc);
    static const uint8_t zero[32] = {0};
    return memcmp(e, zero, 32) == 0 ? BPP_OK : BPP_ERR_VERIFY;
  });
}

}  // extern "C"
