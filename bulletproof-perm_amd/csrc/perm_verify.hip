// Permutation proof, verifier.  Restates ACProof::ArithmeticCircuitProof::verify
// (bp-perm/src/circuit_lib.rs:478-585) in sound mode as ONE GPU MSM (t-check
// weighted by a verifier challenge + the IPA check, generator scalars
// merged).  Transcript order matches oracle/bulletproofs.py ac_verify.
//
// In file order:
//   host jobs      verify_replay, verify_expand, verify_begin,
//                  verify_terms_weighted, verify_partial
//   the ONE MSM    verify_msm: the term layout [2 n_p + 2 generators | proof
//                  points] and its index list, for every path below
//   device jobs    verify_begin_dev (upload, replay, decompression), the slices
//                  of a sharded batch (verify_slice_*_dev,
//                  verify_partial_sharded_dev), job_queue_scalars (a job's
//                  scalars and its decode word), verify_partial_dev
//   fallback       verify_each_dev: each proof's own MSM over what a job left
//   batch drivers  verify_batch (one statement; ok_out names the failing
//                  proofs) and verify_groups (a mixed batch): seed, job(s),
//                  the MSM, is_identity, verify_each_dev, each_report
// The steps the drivers share with reshuffle_api.hip (verify_seed_or_err,
// is_identity, each_pass_proofs, each_report, ok_clear / ok_settle) are in
// perm_internal.h.
#include <string>

#include "perm_internal.h"
#include "layout.h"
#include "verify_dev.h"

int decompress_ws(bpp_ctx* ctx, const uint8_t* enc, size_t count, const char* name, uint32_t** d_out);

namespace {

// Gathered slice blocks -> one contiguous array in ONE launch (a
// hipMemcpyAsync per slice cost ~5 us of launch gap each: 8 slices of
// scalars took 50 us before config 5's rank MSM, tools/shard_model.py):
// slice r's n_r elements of `ew` 16-B units sit at src + r stride + off, and
// land at dst in slice order.
#define GB_MAX 64
struct GatherTab {
  uint32_t n;                // slices
  uint32_t pre[GB_MAX + 1];  // element prefix counts
};
__global__ void __launch_bounds__(256) k_gather_blocks(const uint8_t* __restrict__ src, size_t stride, size_t off,
                                                       uint32_t ew, GatherTab tab, uint4* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // 16-B unit
  const size_t e = i / ew;
  if (e >= tab.pre[tab.n]) return;
  uint32_t lo = 0, hi = tab.n;  // slice r: pre[r] <= e < pre[r + 1]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (tab.pre[mid] <= e) lo = mid;
    else hi = mid;
  }
  const uint4* s = reinterpret_cast<const uint4*>(src + lo * stride + off);
  dst[i] = s[(e - tab.pre[lo]) * ew + i % ew];
}

int gather_blocks_dev(bpp_ctx* ctx, const uint8_t* src, size_t stride, size_t off, size_t elem_bytes,
                             const size_t* counts, size_t nslices, uint8_t* dst) {
  if (nslices > GB_MAX || elem_bytes % 16 || stride % 16 || off % 16) {
    size_t o = 0;
    for (size_t r = 0; r < nslices; ++r) {
      if (counts[r])
        BPP_HIP(hipMemcpyAsync(dst + o * elem_bytes, src + r * stride + off, counts[r] * elem_bytes,
                               hipMemcpyDeviceToDevice, ctx->stream));
      o += counts[r];
    }
    return BPP_OK;
  }
  GatherTab tab;
  tab.n = (uint32_t)nslices;
  tab.pre[0] = 0;
  for (size_t r = 0; r < nslices; ++r) tab.pre[r + 1] = tab.pre[r] + (uint32_t)counts[r];
  const uint32_t ew = (uint32_t)(elem_bytes / 16);
  const size_t units = (size_t)tab.pre[nslices] * ew;
  if (!units) return BPP_OK;
  hipLaunchKernelGGL(k_gather_blocks, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, ctx->stream, src, stride,
                     off, ew, tab, (uint4*)dst);
  return ctx_check_launch(ctx, "k_gather_blocks");
}

// "this device job is ctx's current one"
int job_is_current(bpp_ctx* ctx, const bpp_verify_job& J) {
  if (J.dctx == ctx && J.dgen == ctx->vjob_gen) return BPP_OK;
  ctx->err = "device verify job belongs to another context or was superseded by a later begin";
  return BPP_ERR_ARG;
}

// "the replay rejected a proof": its n verdict words, once the stream has passed them
bool replay_rejected(const uint32_t* bad, size_t n) {
  uint32_t any = 0;
  for (size_t p = 0; p < n; ++p) any |= bad[p];
  return any != 0;
}
// ... of an asynchronous begin, which left the verdicts in J.bad_h
int async_replay_verdict(bpp_ctx* ctx, const bpp_verify_job& J) {
  if (!J.bad_h || !replay_rejected(J.bad_h, J.rcount)) return BPP_OK;
  ctx->err = "a proof's transcript replay rejected it";
  return BPP_ERR_VERIFY;
}

// "a point did not decode": the decompression's verdict word (the first bad
// index, all ones if none)
int decode_verdict(bpp_ctx* ctx, uint64_t dbad) {
  if (dbad == ~0ull) return BPP_OK;
  ctx->err = "undecodable proof point at index " + std::to_string(dbad);
  return BPP_ERR_VERIFY;
}

}  // namespace

namespace perm_impl BPP_HIDDEN {

// Verifier, phase 1: replay one proof's transcript (all Fiat-Shamir
// challenges; point validation as validate_and_append_point).
static bool verify_replay(const perm::Circuit& C, const Proof& P, merlin::Transcript& tr, VerifyChallenges& ch) {
  const uint32_t nv = C.nv, n_p = C.n_p, m = C.m;
  if (P.V.size() != m || P.ipa.L.size() != C.lg || P.ipa.R.size() != C.lg) return false;
  perm::transcript_prefix(C, tr);
  for (uint32_t j = 0; j < nv; ++j) tr.append_point("V", P.V[j].data());
  ch.x_perm = tr.challenge_scalar("x_perm");
  tr.append_point("V", P.V[nv].data());
  if (!tr.validate_and_append_point("A_I", P.AI.data())) return false;
  if (!tr.validate_and_append_point("A_O", P.AO.data())) return false;
  if (!tr.validate_and_append_point("S", P.S.data())) return false;
  ch.y = tr.challenge_scalar("y");
  ch.z = tr.challenge_scalar("z");
  static const char* lab[5] = {"T1", "T3", "T4", "T5", "T6"};
  for (int i = 0; i < 5; ++i)
    if (!tr.validate_and_append_point(lab[i], P.T[i].data())) return false;
  ch.x = tr.challenge_scalar("x");
  tr.append_scalar("TX", P.tau_x);
  tr.append_scalar("mu", P.mu);
  tr.append_scalar("t", P.t_hat);
  ch.w = tr.challenge_scalar("w");
  // bulletproofs InnerProductProof::verification_scalars, transcript part
  tr.innerproduct_domain_sep(n_p);
  ch.u.resize(C.lg);
  for (uint32_t j = 0; j < C.lg; ++j) {
    if (!tr.validate_and_append_point("L", P.ipa.L[j].data())) return false;
    if (!tr.validate_and_append_point("R", P.ipa.R[j].data())) return false;
    ch.u[j] = tr.challenge_scalar("u");
  }
  ch.r = tr.challenge_scalar("t-check-weight");
  return true;
}

// Verifier, phase 2: the proof's unweighted MSM scalars from its
// challenges, scaled by F = U^2 Y (U = prod u_j, Y = y^(n_p - 1)) so that no
// inverse is needed -- the same scalars as k_verify_consts / k_verify_scalars
// (formulas there).  gen_sc (2n_p + 2: G, H, B, Bb) is set; proof-point
// scalars (m + 8 + 2lg, order V, A_I, A_O, S, T1..T6, L.., R..) are appended.
static void verify_expand(const perm::Circuit& C, const Proof& P, const VerifyChallenges& ch,
                          std::vector<Sc>& gen_sc, std::vector<Sc>& pt_sc) {
  const uint32_t n_p = C.n_p, m = C.m, lg = C.lg;
  using hsc::add;
  using hsc::mul;
  using hsc::neg;
  using hsc::sub;
  // st[i] = s_i / s_0 = prod over the bits of i of u^2 (bulletproofs
  // verification_scalars' s_i with s_0 = prod u_j^-1 factored out)
  std::vector<Sc> u_sq(lg), st(n_p);
  Sc U = hsc::one();
  for (uint32_t j = 0; j < lg; ++j) {
    u_sq[j] = hsc::sq(ch.u[j]);
    U = mul(U, ch.u[j]);
  }
  st[0] = hsc::one();
  for (uint32_t i = 1; i < n_p; ++i) {
    const uint32_t lg_i = 31 - __builtin_clz(i), kk = 1u << lg_i;
    st[i] = mul(st[i - kk], u_sq[lg - 1 - lg_i]);
  }
  const Sc x = ch.x, r = ch.r, w = ch.w;
  std::vector<Sc> xp = hsc::powers(x, 7);
  std::vector<Sc> y_n = hsc::powers(ch.y, n_p);  // y^e, e < n_p
  const Sc Y = y_n[n_p - 1], U2 = hsc::sq(U), F = mul(U2, Y);
  std::vector<Sc> zq = hsc::powers(ch.z, C.Q + 1);
  zq.erase(zq.begin());
  const std::vector<Sc> zWL = perm::zW(C.WL, zq, n_p), zWR = perm::zW(C.WR, zq, n_p), zWO = perm::zW(C.WO, zq, n_p),
                        zWV = perm::zW(C.WV, zq, m);
  std::vector<Sc> c = C.c;
  c[C.Q - 1] = hsc::neg(ch.x_perm);
  if (C.deck) c[C.Q - 2] = perm::deck_product(C, ch.x_perm);
  const Sc a = P.ipa.a, b = P.ipa.b;
  const Sc uyaR = hsc::to_mont(mul(mul(U, Y), a)), ubR = hsc::to_mont(mul(U, b)), xR_ = hsc::to_mont(x),
           u2R = hsc::to_mont(U2);
  Sc delta = hsc::zero();  // sum_i U^2 yr_i zWR_i zWL_i (= F delta)
  for (uint32_t i = 0; i < n_p; ++i) {
    const Sc yr = y_n[n_p - 1 - i];  // y^(n_p - 1 - i) = Y y^-i
    const Sc yu = hsc::mulm(yr, u2R);
    const Sc yuR = hsc::to_mont(yu), yrR = hsc::to_mont(yr);
    delta = add(delta, mul(mul(yu, zWR[i]), zWL[i]));
    gen_sc[i] = sub(hsc::mulm(st[i], uyaR), hsc::mulm(hsc::mulm(zWR[i], xR_), yuR));
    gen_sc[n_p + i] = add(sub(hsc::mulm(hsc::mulm(st[n_p - 1 - i], ubR), yrR),
                              hsc::mulm(add(hsc::mulm(zWL[i], xR_), zWO[i]), yuR)),
                          F);
  }
  const Sc zc = hsc::inner_product(zq, c);
  const Sc tcheck_B = mul(r, sub(mul(F, P.t_hat), mul(xp[2], add(delta, mul(F, zc)))));
  const Sc ipa_B = mul(mul(w, F), sub(mul(a, b), P.t_hat));
  gen_sc[2 * n_p] = add(tcheck_B, ipa_B);
  gen_sc[2 * n_p + 1] = mul(F, add(mul(r, P.tau_x), P.mu));
  // proof points
  const Sc rx2FR = hsc::to_mont(mul(mul(r, xp[2]), F));
  for (uint32_t j = 0; j < m; ++j) pt_sc.push_back(neg(hsc::mulm(zWV[j], rx2FR)));
  pt_sc.push_back(neg(mul(F, x)));
  pt_sc.push_back(neg(mul(F, xp[2])));
  pt_sc.push_back(neg(mul(F, xp[3])));
  const int tidx[5] = {1, 3, 4, 5, 6};
  for (int i = 0; i < 5; ++i) pt_sc.push_back(neg(mul(F, mul(r, xp[tidx[i]]))));
  for (uint32_t j = 0; j < lg; ++j) pt_sc.push_back(neg(mul(F, u_sq[j])));
  for (uint32_t j = 0; j < lg; ++j) {  // -Y prod_{k != j} u_k^2 (= -F u_j^-2)
    Sc v = Y;
    for (uint32_t k = 0; k < lg; ++k)
      if (k != j) v = mul(v, u_sq[k]);
    pt_sc.push_back(neg(v));
  }
}

// pass 1 (parallel over chunks of proofs): parse and replay each transcript
// (all challenges and the proof's weight challenge r); a zero y or u_j
// rejects the proof (the checks are scaled by a product of them)
// (circuit_lib.rs:478-585 restated in sound mode)
int verify_begin(const perm::Circuit& C, const uint8_t* label, size_t llen, size_t count, const uint8_t* proofs,
                 size_t proof_stride, const uint8_t* V, std::unique_ptr<bpp_verify_job>& job) {
  job.reset(new bpp_verify_job);
  bpp_verify_job& J = *job;
  J.C = C;
  J.count = count;
  J.npt = (size_t)C.m + 8 + 2 * C.lg;
  J.Ps.resize(count);
  J.rs.resize(count);
  J.ch.resize(count);
  std::vector<uint8_t> ok(count, 0);
  par::for_each(count, [&](size_t p) {
    if (!deserialize(C, proofs + p * proof_stride, perm::proof_len(C), V + p * 32 * C.m, J.Ps[p])) return;
    merlin::Transcript tr(label, llen);
    VerifyChallenges& ch = J.ch[p];
    if (!verify_replay(C, J.Ps[p], tr, ch)) return;
    if (hsc::is_zero(ch.y)) return;
    for (const Sc& u : ch.u)
      if (hsc::is_zero(u)) return;
    J.rs[p] = ch.r;
    ok[p] = 1;
  });
  for (size_t p = 0; p < count; ++p)
    if (!ok[p]) return BPP_ERR_VERIFY;
  return BPP_OK;
}

// Host expansion of every proof's unweighted scalars (verify_expand), once.
static void job_expand_host(const bpp_verify_job& J) {
  std::lock_guard<std::mutex> g(J.mu);
  if (J.expanded) return;
  const perm::Circuit& C = J.C;
  J.gen_p.assign(J.count, std::vector<Sc>());
  J.pt_p.assign(J.count, std::vector<Sc>());
  par::for_each(J.count, [&](size_t p) {
    J.gen_p[p].assign(2 * C.n_p + 2, hsc::zero());
    verify_expand(C, J.Ps[p], J.ch[p], J.gen_p[p], J.pt_p[p]);
  });
  J.expanded = true;
}

// Terms of the job's MSM: merged generators (G, H, B, Bb) + every proof point.
size_t verify_terms(const bpp_verify_job& J) { return 2 * (size_t)J.C.n_p + 2 + J.count * J.npt; }

// pass 2 (host): the job's MSM terms with proof p weighted by
// perm::batch_weight(seed, first + p, r_p) -- generator scalars merged across
// its proofs (G[0..n_p), H[0..n_p), B, Bb), then each proof's points (V,
// A_I, A_O, S, T1..T6, L.., R..) weighted by their proof's weight; enc =
// those points' encodings.
int verify_terms_weighted(const bpp_verify_job& J, const uint8_t seed[32], size_t first, std::vector<Sc>& sc,
                          std::vector<uint8_t>& enc) {
  const uint32_t n_p = J.C.n_p;
  const size_t count = J.count, npt = J.npt;
  job_expand_host(J);
  std::vector<Sc> wR(count);  // Montgomery form (one step per product)
  par::for_each(count, [&](size_t p) { wR[p] = hsc::to_mont(perm::batch_weight(seed, first + p, J.rs[p])); });
  const Sc* wts = wR.data();
  const size_t NG = 2 * (size_t)n_p + 2;
  sc.assign(NG + count * npt, hsc::zero());
  enc.assign(count * npt * 32, 0);
  // proof chunks with private generator accumulators (each reads its proofs'
  // rows contiguously), summed at the end
  const size_t chunks = std::max<size_t>(1, std::min<size_t>(count, 64));
  std::vector<std::vector<Sc>> acc(chunks, std::vector<Sc>(NG, hsc::zero()));
  par::for_each(chunks, [&](size_t ch) {
    std::vector<Sc>& a = acc[ch];
    for (size_t p = ch * count / chunks; p < (ch + 1) * count / chunks; ++p) {
      const Sc& w = wts[p];
      for (size_t i = 0; i < NG; ++i) a[i] = hsc::add(a[i], hsc::mulm(J.gen_p[p][i], w));
      for (size_t j = 0; j < npt; ++j) sc[NG + p * npt + j] = hsc::mulm(J.pt_p[p][j], w);
      proof_points(J.Ps[p], &enc[p * npt * 32]);
    }
  });
  for (size_t ch = 0; ch < chunks; ++ch)
    for (size_t i = 0; i < NG; ++i) sc[i] = hsc::add(sc[i], acc[ch][i]);
  return BPP_OK;
}

// The batch's ONE MSM over windows [wb, we) of its c-bit signed digits (c =
// msm_choose_c(terms)) -> raw partial point: scalars d_sv (2 n_p + 2 merged
// generator scalars, then one per proof point), the npts proof points d_x.
static int verify_msm(bpp_ctx* ctx, const bpp_gens* G, uint32_t n_p, size_t npts, const uint32_t* d_sv,
                      const uint32_t* d_x, uint32_t wb, uint32_t we, h25519::ge* out, const char* idx_ws_name) {
  const size_t NG = 2 * (size_t)n_p + 2, T = NG + npts;
  // term t reads generator t of the resident table (G[0..n_p), H[0..n_p),
  // B, Bb) or proof point t - NG; the index list (workspace idx_ws_name, its
  // upload cached by content) is needed only when the generator set is longer
  // than the padded circuit
  const uint32_t n0 = (uint32_t)(2 * G->n + 2);
  uint32_t* d_idx = nullptr;
  if (G->n != n_p) {
    std::vector<uint32_t> idx(T);
    for (uint32_t i = 0; i < n_p; ++i) {
      idx[i] = G->gidx(i);
      idx[n_p + i] = G->hidx(i);
    }
    idx[2 * n_p] = G->bidx();
    idx[2 * n_p + 1] = G->bbidx();
    for (size_t j = NG; j < T; ++j) idx[j] = n0 + (uint32_t)(j - NG);
    void* d = nullptr;
    BPP_TRY(ctx_ws(ctx, idx_ws_name, idx.size() * 4 + 4, &d));
    BPP_TRY(ctx_h2d_const(ctx, idx_ws_name, d, idx.data(), idx.size() * 4));
    d_idx = (uint32_t*)d;
  }
  const uint32_t c = msm_choose_c((double)T);
  return msm_single_dev(ctx, d_sv, d_idx, G->d_tbl, T, c, wb, we - wb, out, d_x, n0);
}

// pass 2 of a host job: per-proof records built on the host from the host
// replay, then the same device scalars and MSM as a device job.
int verify_partial(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job& J, const uint8_t seed[32], size_t first,
                   uint32_t wb, uint32_t we, h25519::ge* out) {
  const uint32_t n_p = J.C.n_p;
  BPP_TRY(gens_cover(ctx, G, n_p));
  const size_t NG = 2 * (size_t)n_p + 2, count = J.count, npt = J.npt, T = NG + count * npt;
  const uint32_t lg = J.C.lg, nrec = vrec_n(J.C);
  // per-proof records for k_verify_consts / k_verify_scalars and the proof
  // points' encodings
  std::vector<uint32_t> rec(count * nrec * 8);
  std::vector<uint8_t> enc(count * npt * 32);
  {
    HostScope hs(ctx, "verify_terms");
    par::for_each(count, [&](size_t p) {
      const VerifyChallenges& ch = J.ch[p];
      const Proof& P = J.Ps[p];
      uint32_t* r = &rec[p * nrec * 8];
      auto put = [&](uint32_t k, const Sc& v) { hsc::to_bytes((uint8_t*)(r + 8 * k), v); };
      put(VREC_XPERM, ch.x_perm);
      put(VREC_Y, ch.y);
      put(VREC_Z, ch.z);
      put(VREC_X, ch.x);
      put(VREC_W, ch.w);
      put(VREC_R, ch.r);
      put(VREC_A, P.ipa.a);
      put(VREC_B, P.ipa.b);
      put(VREC_THAT, P.t_hat);
      put(VREC_TAUX, P.tau_x);
      put(VREC_MU, P.mu);
      put(VREC_WT, hsc::zero());
      for (uint32_t j = 0; j < lg; ++j) put(VREC_U + j, ch.u[j]);
      proof_points(P, &enc[p * npt * 32]);
    });
  }
  void* d_sv = nullptr;
  BPP_TRY(ctx_ws(ctx, "pv_s", T * 32 + 32, &d_sv));
  BPP_TRY(verify_scalars_dev(ctx, J.C, (uint32_t)count, rec, seed, first, (uint32_t*)d_sv));
  uint32_t* d_x = nullptr;
  int rc = decompress_ws(ctx, enc.data(), enc.size() / 32, "pv_x", &d_x);
  if (rc == BPP_ERR_DECOMPRESS) return BPP_ERR_VERIFY;
  BPP_TRY(rc);
  return verify_msm(ctx, G, n_p, count * npt, (const uint32_t*)d_sv, d_x, wb, we, out, "pv_idx");
}

// pass 1 on the device (bpp_perm_verify_begin_dev): upload the proofs and V,
// replay every transcript on the GPU (k_verify_replay_g, one 16-lane group per proof)
// and return the r challenges; meanwhile the proof points are decompressed
// on child stream VJ_CHILD into the "vj_x" workspace (k_verify_decompress,
// independent of the replay: the 64 replay waves are latency-bound, the
// decompression throughput-bound).  BPP_ERR_VERIFY if the replay rejects a
// proof; an undecodable point is reported by verify_partial_dev.
// rfirst / rcount: replay only that slice (the points of all count proofs
// are still decompressed; rcount = SIZE_MAX: all of them).
// sync = false (verify_batch): nothing waits here -- the replay's verdicts
// stay in J.bad_h for verify_partial_dev to check after its own
// synchronisation, so the weights, scalars and MSM are queued right behind
// the replay with no host round trip (J.rs stays empty).
// each (verify_batch_each): the decompression also keeps one flag per proof,
// behind its verdict word in "vj_dbad" and set by the same memset (all ones;
// cleared where a point of the proof does not decode).
// pub (a circuit with public inputs): the proofs' public scalars, uploaded to
// "vj_pub" beside the proofs and V (by DMA when pinned, else staged with them)
// for the replay and for k_verify_scalars_pub (J.d_pub).
int verify_begin_dev(bpp_ctx* ctx, const perm::Circuit& C, const uint8_t* label, size_t llen, size_t count,
                     const uint8_t* proofs, const uint8_t* V, std::unique_ptr<bpp_verify_job>& job,
                     size_t rfirst, size_t rcount, bool sync, bool each, const uint8_t* pub) {
  job.reset(new bpp_verify_job);
  bpp_verify_job& J = *job;
  if (rcount == SIZE_MAX) rcount = count;
  J.C = C;
  J.count = count;
  J.npt = vpts_n(C);
  J.rfirst = rfirst;
  J.rcount = rcount;
  J.rs.resize(rcount);
  J.dev = true;
  J.dctx = ctx;
  // (before the generation: a refused call supersedes nothing)
  if (count > (1u << 26) || rfirst > count || rcount > count - rfirst) return BPP_ERR_ARG;
  if (C.n_pub && !pub && count) return BPP_ERR_ARG;
  J.dgen = ++ctx->vjob_gen;
  if (!count) return BPP_OK;
  const size_t plen = perm::proof_len(C), vbytes = (size_t)C.m * 32, npts = count * J.npt;
  const size_t pub_bytes = count * (size_t)C.n_pub * 32;
  bpp_ctx* kid = nullptr;
  BPP_TRY(ctx_child(ctx, ctx->vj_child, &kid));
  if (!ctx->vj_ev_dec) BPP_HIP(hipEventCreateWithFlags(&ctx->vj_ev_dec, hipEventDisableTiming));
  // (the previous job's decompression may still read "vj_in")
  if (ctx->vj_dec_pending) BPP_HIP(hipStreamWaitEvent(ctx->stream, ctx->vj_ev_dec, 0));
  void *d_in = nullptr, *d_rec = nullptr, *d_x = nullptr, *d_dbad = nullptr;
  BPP_TRY(ctx_ws(ctx, "vj_in", count * (plen + vbytes), &d_in));
  const uint32_t* d_pf = (const uint32_t*)d_in;
  const uint32_t* d_V = (const uint32_t*)((uint8_t*)d_in + count * plen);
  void* d_pub = nullptr;
  if (pub_bytes) BPP_TRY(ctx_ws(ctx, "vj_pub", pub_bytes, &d_pub));
  J.d_pub = (const uint32_t*)d_pub;
  // (+1: the pad record of the replay's groups past the batch)
  BPP_TRY(ctx_ws(ctx, "vj_rec", (count + 1) * vrec_n(C) * 32, &d_rec));
  BPP_TRY(ctx_ws(ctx, "vj_x", npts * MSM_NIELS_WORDS * 4, &d_x));
  const size_t dbad_bytes = 8 + (each ? count * 4 : 0);
  BPP_TRY(ctx_ws(ctx, "vj_dbad", dbad_bytes, &d_dbad));
  BPP_HIP(hipMemsetAsync(d_dbad, 0xff, dbad_bytes, ctx->stream));
  uint32_t* d_pdec = each ? (uint32_t*)d_dbad + 2 : nullptr;
  {
    HostScope hs(ctx, "verify_upload");
    {
      // The proofs and V go up in chunks of proofs (each chunk's proof bytes
      // and V bytes to their places in the [proofs][V] layout), and each
      // chunk's points are decompressed on the child stream as soon as its
      // copies land, so the decompression -- the longest stage beside the
      // replay -- starts while later chunks are still being staged and copied
      // (at most 4 chunks).
      // (chunks of >= 1024 proofs: a decompression launch is a per-lane
      // latency chain of ~50-80 us however few points it has, and the
      // launches of one stream run in turn -- a 512-proof slice in two
      // chunks waited 0.32 ms for its points, tools/shard_model.py)
      const size_t nchunk = std::min<size_t>(4, std::max<size_t>(1, count / 1024));
      while (ctx->vj_ev_chunk.size() < nchunk) {
        hipEvent_t e = nullptr;
        BPP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->vj_ev_chunk.push_back(e);
      }
      // proofs and V already in pinned host memory (bpp_host_alloc, or memory
      // the caller registered itself) go up by DMA from where they are;
      // pageable buffers are staged through the pinned arena first (the host
      // copy then paces the upload)
      const bool direct = host_is_pinned(proofs, count * plen) && host_is_pinned(V, count * vbytes) &&
                          (!pub_bytes || host_is_pinned(pub, pub_bytes));
      uint8_t* stg = nullptr;
      if (!direct) BPP_TRY(ctx_h2d_stage(ctx, count * (plen + vbytes) + pub_bytes, &stg));
      if (pub_bytes) {  // (whole, first: the replay reads all of it, the decompression none)
        if (direct) {
          BPP_HIP(hipMemcpyAsync(d_pub, pub, pub_bytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
          uint8_t* ps = stg + count * (plen + vbytes);
          ctx_stage_copy(ps, pub, pub_bytes);
          BPP_TRY(ctx_h2d_staged(ctx, d_pub, ps, pub_bytes));
        }
      }
      // (The first nchunk - 1 chunks' transcripts started on a side stream
      // once their bytes were up, beside the last chunk's upload, did not pay
      // when measured behind a switch since removed: a replay launch is a
      // latency chain of ~0.26-0.28 ms however few transcripts it holds, so
      // the last chunk's replay ends when the whole one did: 1.84-1.89 vs
      // 1.80-1.86 ms per batch, profiles/r05_verify_ab.txt)
      for (size_t q = 0; q < nchunk; ++q) {
        const size_t p0 = count * q / nchunk, p1 = count * (q + 1) / nchunk;
        const size_t po = p0 * plen, pn = (p1 - p0) * plen, vo = count * plen + p0 * vbytes, vn = (p1 - p0) * vbytes;
        if (direct) {
          BPP_HIP(hipMemcpyAsync((uint8_t*)d_in + po, proofs + po, pn, hipMemcpyHostToDevice, ctx->stream));
          BPP_HIP(hipMemcpyAsync((uint8_t*)d_in + vo, V + p0 * vbytes, vn, hipMemcpyHostToDevice, ctx->stream));
        } else {
          // (whole parts: in pieces, each piece's DMA behind its host copy,
          // measured slower, r05_verify_ab.txt)
          auto staged = [&](size_t o, const uint8_t* src, size_t n) -> int {
            ctx_stage_copy(stg + o, src, n);
            return ctx_h2d_staged(ctx, (uint8_t*)d_in + o, stg + o, n);
          };
          BPP_TRY(staged(po, proofs + po, pn));
          BPP_TRY(staged(vo, V + p0 * vbytes, vn));
        }
        BPP_HIP(hipEventRecord(ctx->vj_ev_chunk[q], ctx->stream));
        BPP_HIP(hipStreamWaitEvent(kid->stream, ctx->vj_ev_chunk[q], 0));
        BPP_TRY(verify_decompress_dev(kid, C, (uint32_t)count, d_pf, d_V, (uint32_t*)d_x,
                                      (unsigned long long*)d_dbad, (uint32_t)p0, (uint32_t)p1, 0, ~0u, d_pdec));
      }
      BPP_HIP(hipEventRecord(ctx->vj_ev_dec, kid->stream));
      ctx->vj_dec_pending = true;
    }
  }
  HostScope hs(ctx, "verify_replay");
  uint32_t *h_r = nullptr, *h_bad = nullptr;
  uint32_t* h_init = nullptr;  // the shared transcript prefix, read in place (zero copy)
  {
    uint32_t init[52];
    verify_init_state(C, label, llen, init);
    BPP_TRY(ctx_zc_in(ctx, "vj_init", init, sizeof init, &h_init));
  }
  if (!rcount) return ctx_sync(ctx);
  BPP_TRY(ctx_zc_out(ctx, "vj_r", rcount * 32, &h_r));
  BPP_TRY(ctx_zc_out(ctx, "vj_bad", rcount * 4, &h_bad));
  BPP_TRY(verify_replay_dev(ctx, C, (uint32_t)rcount, h_init, d_pf + rfirst * (plen / 4),
                            d_V + rfirst * (vbytes / 4), (uint32_t*)d_rec, h_r, h_bad,
                            J.d_pub ? J.d_pub + rfirst * (size_t)C.n_pub * 8 : nullptr));
  if (!sync) {
    J.bad_h = h_bad;
    J.rs.clear();
    return BPP_OK;
  }
  BPP_TRY(ctx_sync_latency(ctx));
  if (replay_rejected(h_bad, rcount)) return BPP_ERR_VERIFY;
  memcpy(J.rs.data(), h_r, rcount * 32);
  return BPP_OK;
}

// A job's scalars as one slice of a sharded batch
// (bpp_perm_verify_slice_scalars_at): the slice's
// proofs weighted by perm::batch_weight(seed, rfirst + p, r_p), the generator
// scalars summed over the slice and the slice's proof-point scalars ->
// d_out = [NG | rcount x npt] x 32 B (device memory).
int verify_slice_scalars_dev(bpp_ctx* ctx, const bpp_verify_job& J, const uint8_t seed[32], size_t first,
                             uint32_t* d_out) {
  BPP_TRY(job_is_current(ctx, J));
  if (!J.rcount) {  // an empty slice adds nothing to the generator scalars
    BPP_HIP(hipMemsetAsync(d_out, 0, (2 * (size_t)J.C.n_p + 2) * 32, ctx->stream));
    return ctx_sync(ctx);
  }
  void* d_rec = nullptr;
  BPP_TRY(ctx_ws(ctx, "vj_rec", (J.rcount + 1) * vrec_n(J.C) * 32, &d_rec));
  uint32_t* h_seed = nullptr;
  BPP_TRY(ctx_zc_in(ctx, "vj_seed", seed, 32, &h_seed));
  BPP_TRY(verify_scalars_dev_rec(ctx, J.C, (uint32_t)J.rcount, (const uint32_t*)d_rec, h_seed, first + J.rfirst,
                                 d_out));
  BPP_TRY(ctx_sync(ctx));
  BPP_TRY(async_replay_verdict(ctx, J));
  return BPP_OK;
}

// A job's decompressed proof points (bpp_perm_verify_slice_points): count x
// npt extended-Niels records (MSM_NIELS_WORDS words each, proof-major) ->
// d_out, after the job's decompression; BPP_ERR_VERIFY if a point did not
// decode.  Synchronises ctx.
int verify_slice_points_dev(bpp_ctx* ctx, const bpp_verify_job& J, void* d_out) {
  BPP_TRY(job_is_current(ctx, J));
  if (!J.count) return BPP_OK;
  // on the decompression's own (child) stream, behind the decompression:
  // an asynchronous begin's replay may still be running on ctx's stream
  bpp_ctx* kid = nullptr;
  BPP_TRY(ctx_child(ctx, ctx->vj_child, &kid));
  void *d_x = nullptr, *d_dbad = nullptr;
  BPP_TRY(ctx_ws(ctx, "vj_x", J.count * J.npt * MSM_NIELS_WORDS * 4, &d_x));
  BPP_TRY(ctx_ws(ctx, "vj_dbad", 8, &d_dbad));
  uint64_t* h_dbad = nullptr;
  BPP_TRY(ctx_zc_out(kid, "sp_dbad_h", 8, (uint32_t**)&h_dbad));
  BPP_HIP(hipStreamWaitEvent(kid->stream, ctx->vj_ev_dec, 0));
  BPP_HIP(hipMemcpyAsync(h_dbad, d_dbad, 8, hipMemcpyDeviceToHost, kid->stream));
  BPP_HIP(hipMemcpyAsync(d_out, d_x, J.count * J.npt * MSM_NIELS_WORDS * 4, hipMemcpyDeviceToDevice, kid->stream));
  BPP_TRY(ctx_sync(kid));
  return decode_verdict(ctx, *h_dbad);
}

// The MSM of a sharded batch over windows [wb, we) (bpp_perm_verify_partial_sharded):
// slice s's scalar block at d_blocks + s stride ([NG | counts[s] x npt]:
// the generator scalars summed over the slice, then its proof-point scalars)
// and its decompressed points at d_pblocks + s
// pstride (counts[s] x npt Niels records, bpp_perm_verify_slice_points); J is
// this rank's job over its own slice, batch proofs [first, first + J.count).
int verify_partial_sharded_dev(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job& J, size_t first,
                               const uint8_t* d_blocks, size_t stride, const uint8_t* d_pblocks, size_t pstride,
                               const size_t* counts, size_t nslices, uint32_t wb, uint32_t we, h25519::ge* out) {
  BPP_TRY(job_is_current(ctx, J));
  if (J.rcount != J.count) {
    ctx->err = "a sharded batch takes one whole job per slice (bpp_perm_verify_begin_dev on the slice)";
    return BPP_ERR_ARG;
  }
  BPP_TRY(gens_cover(ctx, G, J.C.n_p));
  const size_t NG = 2 * (size_t)J.C.n_p + 2, npt = J.npt, prec = (size_t)MSM_NIELS_WORDS * 4;
  size_t total = 0;
  bool mine = false, tight = true;  // (tight: the point blocks already lie end to end)
  for (size_t r = 0; r < nslices; ++r) {
    if ((NG + counts[r] * npt) * 32 > stride || counts[r] * npt * prec > pstride) return BPP_ERR_ARG;
    mine |= total == first && counts[r] == J.count;
    tight &= r + 1 == nslices || counts[r] * npt * prec == pstride;
    total += counts[r];
  }
  if (stride % 16 || pstride % 16 || total > (1u << 26)) return BPP_ERR_ARG;
  if (!mine) {
    ctx->err = "the gathered blocks do not hold this job's slice at its proof offset";
    return BPP_ERR_ARG;
  }
  const size_t T = NG + total * npt;
  void* d_sv = nullptr;
  BPP_TRY(ctx_ws(ctx, "pv_s", T * 32 + 32, &d_sv));
  BPP_TRY(verify_sum_blocks_dev(ctx, (uint32_t)nslices, (uint32_t)NG, (const uint32_t*)d_blocks,
                                (uint32_t)(stride / 4), (uint32_t*)d_sv));
  const uint8_t* d_x = d_pblocks;
  if (!tight) {
    void* d = nullptr;
    BPP_TRY(ctx_ws(ctx, "vj_xg", total * npt * prec, &d));
    d_x = (const uint8_t*)d;
  }
  // the slices' proof-point scalars (and, when padded, points) in proof order
  BPP_TRY(gather_blocks_dev(ctx, d_blocks, stride, NG * 32, npt * 32, counts, nslices, (uint8_t*)d_sv + NG * 32));
  if (!tight) BPP_TRY(gather_blocks_dev(ctx, d_pblocks, pstride, 0, npt * prec, counts, nslices, (uint8_t*)d_x));
  BPP_TRY(verify_msm(ctx, G, J.C.n_p, total * npt, (const uint32_t*)d_sv, (const uint32_t*)d_x, wb, we, out, "pv_idx"));
  return ctx_sync(ctx);
}

// What a device job's MSM reads, once job_queue_scalars has queued it: the
// job's scalars in "pv_s" ([2 n_p + 2 merged | count x npt]; each proof's own
// generator rows stay in "vs_gen"), its decompressed points in "vj_x", and the
// decompression's verdict word in pinned memory.
struct JobTerms {
  const uint32_t *d_sv, *d_x;
  const uint64_t* h_dbad;  // valid once ctx's stream has been synchronised
};

// Queue a device job's scalars on ctx's stream, behind its replay: each
// proof's weight perm::batch_weight(seed, first + p, r_p) and constants
// (k_verify_consts) and the weighted scalars (k_verify_scalars); then, behind
// the decompression (vj_ev_dec), the copy of its verdict word.  No host wait.
static int job_queue_scalars(bpp_ctx* ctx, const bpp_verify_job& J, const uint8_t seed[32], size_t first,
                             JobTerms& q) {
  const size_t count = J.count, T = 2 * (size_t)J.C.n_p + 2 + count * J.npt;
  void *d_rec = nullptr, *d_x = nullptr, *d_sv = nullptr, *d_dbad = nullptr;
  BPP_TRY(ctx_ws(ctx, "vj_rec", (count + 1) * vrec_n(J.C) * 32, &d_rec));
  BPP_TRY(ctx_ws(ctx, "vj_x", count * J.npt * MSM_NIELS_WORDS * 4, &d_x));
  BPP_TRY(ctx_ws(ctx, "vj_dbad", 8, &d_dbad));
  BPP_TRY(ctx_ws(ctx, "pv_s", T * 32 + 32, &d_sv));
  {
    HostScope hs(ctx, "verify_terms");
    uint32_t* h_seed = nullptr;
    BPP_TRY(ctx_zc_in(ctx, "vj_seed", seed, 32, &h_seed));
    BPP_TRY(verify_scalars_dev_rec(ctx, J.C, (uint32_t)count, (const uint32_t*)d_rec, h_seed, first,
                                   (uint32_t*)d_sv, J.d_pub));
  }
  uint64_t* h_dbad = nullptr;
  BPP_TRY(ctx_zc_out(ctx, "vj_dbad_h", 8, (uint32_t**)&h_dbad));
  BPP_HIP(hipStreamWaitEvent(ctx->stream, ctx->vj_ev_dec, 0));
  BPP_HIP(hipMemcpyAsync(h_dbad, d_dbad, 8, hipMemcpyDeviceToHost, ctx->stream));
  q = {(const uint32_t*)d_sv, (const uint32_t*)d_x, h_dbad};
  return BPP_OK;
}

// pass 2 of a device job: its scalars (job_queue_scalars) and the MSM over
// windows [wb, we); BPP_ERR_VERIFY if a proof point did not decode or (an
// asynchronous begin) the replay rejected a proof.
int verify_partial_dev(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job& J, const uint8_t seed[32],
                       size_t first, uint32_t wb, uint32_t we, h25519::ge* out) {
  BPP_TRY(job_is_current(ctx, J));
  if (J.rcount != J.count) {
    ctx->err = "a partially replayed job has no whole-batch partial";
    return BPP_ERR_ARG;
  }
  BPP_TRY(gens_cover(ctx, G, J.C.n_p));
  JobTerms q;
  BPP_TRY(job_queue_scalars(ctx, J, seed, first, q));
  BPP_TRY(verify_msm(ctx, G, J.C.n_p, J.count * J.npt, q.d_sv, q.d_x, wb, we, out, "pv_idx"));
  BPP_TRY(ctx_sync_latency(ctx));  // (msm_single_dev has synchronised; this keeps h_dbad's contract)
  BPP_TRY(async_replay_verdict(ctx, J));
  return decode_verdict(ctx, *q.h_dbad);
}

// Per-proof verdicts of a device job whose batch check (verify_partial_dev)
// has run and not passed: everything it needs is still on the device -- each
// proof's own generator scalars ("vs_gen", k_verify_scalars' rows before the
// merge), its proof-point scalars ("pv_s" behind the merged generators), the
// decompressed points ("vj_x"), the decode flags (behind "vj_dbad"'s verdict
// word) and the replay's verdicts (J.bad_h) -- so nothing is uploaded,
// replayed, decompressed or expanded again.  R_p = sum_i gen[p][i] Gen_i +
// sum_j s[p][j] X_{p,j} (NG + npt terms, still weighted by w_p != 0) through
// the multi-MSM engine, in passes of proofs; ok[p] = R_p encodes as 0^32 and
// proof p decoded and was not replay-rejected.  One synchronisation.
static int verify_each_dev(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_job& J, uint8_t* ok_out) {
  const uint32_t n_p = J.C.n_p, n0 = (uint32_t)(2 * G->n + 2);
  const size_t count = J.count, npt = J.npt, NG = 2 * (size_t)n_p + 2, TP = NG + npt;
  if (n0 + count * npt >= 0x80000000ull) return BPP_ERR_LEN;  // (an engine entry is index | sign << 31)
  const uint32_t c = msm_choose_c((double)TP);
  size_t per = each_pass_proofs(TP, c);
  if (const char* e = getenv("BPP_VERIFY_EACH_PROOFS"))  // (read per call, as BPP_MSM_FB)
    per = std::min<size_t>(strtoull(e, nullptr, 10), ((size_t)1 << 24) / TP);
  per = std::min(std::max<size_t>(per, 1), count);
  void *d_gen, *d_sv, *d_x, *d_dbad, *d_rbad, *d_s, *d_idx, *d_off, *d_res, *d_enc;
  BPP_TRY(ctx_ws(ctx, "vs_gen", count * NG * 32, &d_gen));
  BPP_TRY(ctx_ws(ctx, "pv_s", (NG + count * npt) * 32 + 32, &d_sv));
  BPP_TRY(ctx_ws(ctx, "vj_x", count * npt * MSM_NIELS_WORDS * 4, &d_x));
  BPP_TRY(ctx_ws(ctx, "vj_dbad", 8 + count * 4, &d_dbad));
  BPP_TRY(ctx_ws(ctx, "ve_rbad", count * 4, &d_rbad));
  BPP_TRY(ctx_ws(ctx, "ve_s", per * TP * 32 + 32, &d_s));
  BPP_TRY(ctx_ws(ctx, "ve_idx", per * TP * 4 + 4, &d_idx));
  BPP_TRY(ctx_ws(ctx, "ve_off", (per + 1) * 4, &d_off));
  BPP_TRY(ctx_ws(ctx, "ve_res", count * P3_BYTES, &d_res));
  BPP_TRY(ctx_ws(ctx, "ve_enc", count * 32, &d_enc));
  uint32_t* h_ok = nullptr;
  BPP_TRY(ctx_zc_out(ctx, "ve_ok_h", count, &h_ok));
  // (the replay's verdicts are in pinned host memory: one copy instead of a
  // host read per term)
  BPP_HIP(hipMemcpyAsync(d_rbad, J.bad_h, count * 4, hipMemcpyHostToDevice, ctx->stream));
  for (size_t p0 = 0; p0 < count; p0 += per) {
    const uint32_t M = (uint32_t)std::min(per, count - p0);
    BPP_TRY(verify_each_terms_dev(ctx, J.C, (uint32_t)G->n, n0, (uint32_t)p0, M, (const uint32_t*)d_gen,
                                  (const uint32_t*)d_sv, (const uint32_t*)d_rbad, (uint32_t*)d_s, (uint32_t*)d_idx,
                                  (uint32_t*)d_off));
    BPP_TRY(msm_multi_dev(ctx, (const uint32_t*)d_s, (const uint32_t*)d_idx, (const uint32_t*)d_off, M,
                          (uint32_t)(M * TP), c, G->d_tbl, (const uint32_t*)d_x, n0, (uint32_t*)d_res + p0 * P3_WORDS));
  }
  BPP_TRY(points_compress_p3_dev(ctx, (const uint32_t*)d_res, count, (uint8_t*)d_enc));
  BPP_TRY(verify_each_verdict_dev(ctx, (uint32_t)count, (const uint32_t*)d_enc, (const uint32_t*)d_dbad + 2,
                                  (const uint32_t*)d_rbad, (uint8_t*)h_ok));
  BPP_TRY(ctx_sync(ctx));
  memcpy(ok_out, h_ok, count);
  return BPP_OK;
}

// Verify `count` proofs with ONE MSM: generator scalars summed across proofs
// with per-proof weights derived from every proof's r challenge; the
// transcripts are replayed on the device.  ok_out (nullptr: one verdict for the
// batch) names the failing proofs, [count], 1 = proof p verifies alone: the same
// job and the same ONE merged MSM, all ones when it passes; only when it does
// not, each proof's own MSM (verify_each_dev) and each_report.
int verify_batch(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const uint8_t* label, size_t llen,
                 size_t count, const uint8_t* proofs, const uint8_t* V, uint8_t* ok_out, const uint8_t* pub) {
  const bool each = ok_out != nullptr;
  uint8_t seed[32];
  BPP_TRY(verify_seed_or_err(ctx, seed));
  std::unique_ptr<bpp_verify_job> job;
  BPP_TRY(verify_begin_dev(ctx, C, label, llen, count, proofs, V, job, 0, SIZE_MAX, false, each, pub));
  const uint32_t c = msm_choose_c((double)verify_terms(*job));
  h25519::ge res;
  // (BPP_ERR_VERIFY: a replay verdict or an undecodable point, found after
  // the MSM and its synchronisation, with the job's device state complete)
  const int rc = verify_partial_dev(ctx, G, *job, seed, 0, 0, (254 + c - 1) / c, &res);
  if (rc != BPP_OK && !(each && rc == BPP_ERR_VERIFY)) return rc;
  if (rc == BPP_OK && is_identity(res)) {
    if (each) memset(ok_out, 1, count);
    return BPP_OK;
  }
  if (!each) return BPP_ERR_VERIFY;
  BPP_TRY(verify_each_dev(ctx, G, *job, ok_out));
  return each_report(ctx, ok_out, count);
}

// A mixed batch (bpp_verify_groups, _each with ok_out): n <= VG_MAX groups, each
// `count` proofs of one statement, verified with ONE MSM.  The proof at
// position p of group g is weighted by perm::batch_weight(seed, first_g + p,
// r_p), first_g = the proofs before it in the call.  Every non-empty group
// runs its job -- upload, replay, decompression, scalars -- on a group context
// of its own (ctx_group), so the groups' latency chains overlap; ctx's stream
// waits for one event per group, sums the groups' generator blocks into [G:
// n_max | H: n_max | B | Bb] and gathers their proof-point scalars and points
// behind it (k_verify_merge_groups, k_verify_gather_groups), and runs the MSM.
// Nothing waits on the host before the MSM's own synchronisation; the replay
// and decode verdicts of every group are read after it.  ok_out: as
// verify_batch's -- all ones when the batch passes, else each group's
// verify_each_dev over what its job left on its context.
int verify_groups(bpp_ctx* ctx, const bpp_gens* G, const VerifyGroup* groups, size_t n, uint8_t* ok_out) {
  if (n > VG_MAX) return BPP_ERR_LEN;
  uint32_t n_max = 0;
  size_t total = 0, pts = 0;
  for (size_t g = 0; g < n; ++g) {
    if (!groups[g].count) continue;
    const perm::Circuit& C = *groups[g].C;
    if (groups[g].count > (1u << 26) || (C.n_pub && !groups[g].pub)) return BPP_ERR_ARG;
    n_max = std::max(n_max, C.n_p);
    total += groups[g].count;
    pts += groups[g].count * vpts_n(C);
  }
  if (!total) return BPP_OK;
  // (before any context's job generation moves)
  BPP_TRY(gens_cover(ctx, G, n_max));
  const uint32_t n0 = (uint32_t)(2 * G->n + 2);
  const size_t NG = 2 * (size_t)n_max + 2, T = NG + pts, prec = (size_t)MSM_NIELS_WORDS * 4;
  if (total > (1u << 26) || n0 + pts >= 0x80000000ull) return BPP_ERR_LEN;  // (an engine entry is index | sign << 31)
  uint8_t seed[32];
  BPP_TRY(verify_seed_or_err(ctx, seed));
  struct Run {
    bpp_ctx* gctx = nullptr;
    std::unique_ptr<bpp_verify_job> job;
    size_t first = 0;
    const uint64_t* h_dbad = nullptr;
  };
  Run run[VG_MAX];
  size_t started = 0;  // group contexts with work queued
  // "a failed call leaves no kernel reading the caller's buffers": every
  // group context that has work queued is drained, then ctx
  auto drain = [&]() {
    for (size_t s = 0; s < started; ++s) {
      bpp_ctx* gc = run[s].gctx;
      if (!gc->children.empty()) (void)hipStreamSynchronize(gc->children[0]->stream);
      (void)ctx_sync(gc);
    }
    (void)ctx_sync(ctx);
  };
  // a group context's refusal, reported on ctx
  auto fail = [&](bpp_ctx* gc, int rc) {
    if (gc && !gc->err.empty()) ctx->err = gc->err;
    drain();
    return rc;
  };
  void *d_sv = nullptr, *d_x = nullptr;
  if (int rc = ctx_ws(ctx, "vg_s", T * 32 + 32, &d_sv)) return rc;
  if (int rc = ctx_ws(ctx, "vg_x", pts * prec, &d_x)) return rc;
  VerifyGroupTab tab;
  VerifyGatherTab gt;
  const bool each = ok_out != nullptr;
  size_t first = 0, pt0 = 0;
  for (size_t g = 0; g < n; ++g) {
    const VerifyGroup& grp = groups[g];
    if (!grp.count) continue;
    const perm::Circuit& C = *grp.C;
    Run& R = run[started];
    if (int rc = ctx_group(ctx, started, &R.gctx)) return fail(nullptr, rc);
    bpp_ctx* gc = R.gctx;
    gc->err.clear();
    R.first = first;
    ++started;
    // the group's job, asynchronous: upload, replay, decompression
    if (int rc = verify_begin_dev(gc, C, grp.label, grp.llen, grp.count, grp.proofs, grp.V, R.job, 0, SIZE_MAX, false,
                                  each, grp.pub))
      return fail(gc, rc);
    // its scalars, as verify_partial_dev queues them; then the group's event
    // and where the merge finds the group's blocks
    const size_t NGg = 2 * (size_t)C.n_p + 2, gpts = grp.count * R.job->npt;
    auto queue = [&]() -> int {
      bpp_ctx* ctx = gc;  // (BPP_HIP names it)
      JobTerms q;
      BPP_TRY(job_queue_scalars(ctx, *R.job, seed, first, q));
      R.h_dbad = q.h_dbad;
      if (!ctx->vg_ev) BPP_HIP(hipEventCreateWithFlags(&ctx->vg_ev, hipEventDisableTiming));
      BPP_HIP(hipEventRecord(ctx->vg_ev, ctx->stream));
      tab.g[tab.n].blk = q.d_sv;
      tab.g[tab.n].n_p = C.n_p;
      ++tab.n;
      auto seg = [&](const void* src, void* dst, size_t bytes) {
        gt.src[gt.n] = (const uint4*)src;
        gt.dst[gt.n] = (uint4*)dst;
        gt.pre[gt.n + 1] = gt.pre[gt.n] + bytes / 16;
        ++gt.n;
      };
      seg((const uint8_t*)q.d_sv + NGg * 32, (uint8_t*)d_sv + (NG + pt0) * 32, gpts * 32);
      seg(q.d_x, (uint8_t*)d_x + pt0 * prec, gpts * prec);
      return BPP_OK;
    };
    if (int rc = queue()) return fail(gc, rc);
    if (hipStreamWaitEvent(ctx->stream, gc->vg_ev, 0) != hipSuccess) {
      ctx->err = "hipStreamWaitEvent on a group's event failed";
      return fail(nullptr, BPP_ERR_DEVICE);
    }
    first += grp.count;
    pt0 += gpts;
  }
  h25519::ge res;
  auto merged = [&]() -> int {
    BPP_TRY(verify_merge_groups_dev(ctx, tab, n_max, (uint32_t*)d_sv, gt));
    const uint32_t c = msm_choose_c((double)T);  // (every window)
    return verify_msm(ctx, G, n_max, pts, (const uint32_t*)d_sv, (const uint32_t*)d_x, 0, (254 + c - 1) / c, &res,
                      "vg_idx");
  };
  if (int rc = merged()) return fail(nullptr, rc);
  // ctx's stream waited for every group's event and has been synchronised:
  // the group contexts are idle, their pinned verdicts written
  bool rejected = false;
  for (size_t s = 0; s < started; ++s) {
    ctx_mark_idle(run[s].gctx);
    if (async_replay_verdict(ctx, *run[s].job) != BPP_OK || decode_verdict(ctx, *run[s].h_dbad) != BPP_OK)
      rejected = true;
  }
  if (!rejected) {
    if (is_identity(res)) {
      if (each) memset(ok_out, 1, total);
      return BPP_OK;
    }
    ctx->err = "the batch check failed";
  }
  if (!each) return BPP_ERR_VERIFY;
  for (size_t s = 0; s < started; ++s)
    if (int rc = verify_each_dev(run[s].gctx, G, *run[s].job, ok_out + run[s].first)) return fail(run[s].gctx, rc);
  return each_report(ctx, ok_out, total);
}

}  // namespace perm_impl
