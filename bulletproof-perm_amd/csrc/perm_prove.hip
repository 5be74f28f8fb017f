// Permutation proof, prover: the sound-mode arithmetic-circuit batch prover
// over the GPU primitives, and the wipe of the secrets it leaves behind.
//
// Restates ACProof::ArithmeticCircuitProof (bp-perm/src/circuit_lib.rs):
//   create                 :139-253  -> V (fixed-base Pedersen), A_I/A_O/S
//                                       (one 3-MSM batch)
//   challenge_wit_and_const:133-138  -> y, z
//   compute_per_challenges :256-302  -> y^n, y^-n (batch inversion), z^Q W
//                                       (sparse, host)
//   commit_Ts              :304-423  -> t_1..t_6 (host), T_i (fixed-base)
//   random_chall_x         :425-432  -> x
//   blinding_values        :434-476  -> l, r, t_hat, tau_x, mu; the clear
//                                       l, r of :466-467 replaced by an IPA
// (verify :478-585 is perm_verify.hip.)  Transcript order and RNG draw order
// match oracle/bulletproofs.py ac_prove exactly (tests compare proof bytes).
#include <cstdlib>
#include <functional>
#include <thread>

#include "perm_internal.h"
#include "circuit_witness.h"
#include "host/circuit.h"
#include "layout.h"
#include "merlin_dev.h"
#include "poly.h"
#include "verify_dev.h"
#include "witness.h"

using namespace perm_impl;  // (Proof, ProveInputs, Sc)

namespace {

// Small vectors go to pinned host memory the kernels read in place (no copy
// launch, ctx_zc_in); large ones (vector commitments of many terms, whose
// scalars every window lane re-reads) are copied to the device.
#define UPLOAD_ZC_MAX (256u << 10)
int upload_sc(bpp_ctx* ctx, const std::vector<Sc>& v, const char* name, uint32_t** d) {
  static_assert(sizeof(Sc) == 32, "Sc is the 32-byte little-endian scalar");  // canonical Sc == its bytes
  if (v.size() * 32 <= UPLOAD_ZC_MAX) return ctx_zc_in(ctx, name, v.data(), v.size() * 32, d);
  void* p = nullptr;
  BPP_TRY(ctx_ws(ctx, name, v.size() * 32 + 32, &p));
  BPP_TRY(ctx_h2d(ctx, p, v.data(), v.size() * 32));
  *d = (uint32_t*)p;
  return BPP_OK;
}

// Fixed-base commitments v_i*B + g_i*Bb, returned compressed.
// Small batches (<= PED_DOUBLE_MAX) commit with halved scalars and encode
// C = 2 (C / 2) on the host (points_double_encode_p3): one inversion per
// chunk instead of a ~70 us per-point inverse-square-root chain on the GPU.
#define PED_DOUBLE_MAX 2048
int pedersen_host(bpp_ctx* ctx, const bpp_gens* g, const std::vector<Sc>& v, const std::vector<Sc>& gam,
                  std::vector<Enc32>& out) {
  const size_t m = v.size();
  // (encoding the 13 312 V commitments of a 128-proof batch this way too
  // measured slower at 8 batches in flight, 72-77 K vs 80-83 K proofs/s:
  // the host is loaded as well)
  const bool doubled = m <= PED_DOUBLE_MAX;
  uint32_t *d_v, *d_g;
  {
    HostScope hs(ctx, "ped_upload");
    if (doubled) {
      std::vector<Sc> hv(m), hg(m);
      for (size_t i = 0; i < m; ++i) {
        hv[i] = hsc::half(v[i]);
        hg[i] = hsc::half(gam[i]);
      }
      BPP_TRY(upload_sc(ctx, hv, "pp_v", &d_v));
      BPP_TRY(upload_sc(ctx, hg, "pp_g", &d_g));
    } else {
      BPP_TRY(upload_sc(ctx, v, "pp_v", &d_v));
      BPP_TRY(upload_sc(ctx, gam, "pp_g", &d_g));
    }
  }
  out.resize(m);
  if (doubled) {
    uint32_t* h_p3 = nullptr;  // written in place by the kernel (ctx_zc_out)
    BPP_TRY(ctx_zc_out(ctx, "pp_p3_h", m * P3_BYTES, &h_p3));
    {
      HostScope hs(ctx, "ped_kernels");
      BPP_TRY(pedersen_dev(ctx, g, d_v, d_g, m, nullptr, h_p3));
    }
    HostScope hs(ctx, "ped_d2h");
    BPP_TRY(ctx_sync(ctx));
    return points_double_encode_host(ctx, h_p3, m, out[0].data());
  }
  void* d_out = nullptr;
  BPP_TRY(ctx_ws(ctx, "pp_out", m * 32, &d_out));
  {
    HostScope hs(ctx, "ped_kernels");
    BPP_TRY(pedersen_dev(ctx, g, d_v, d_g, m, (uint32_t*)d_out, nullptr));
  }
  HostScope hs(ctx, "ped_d2h");
  BPP_TRY(ctx_d2h(ctx, out.data(), d_out, m * 32));
  return BPP_OK;
}

// The prover's V transcript phase on the device (k_prove_v_transcript,
// BPP_PROVE_DEV_V=1) instead of the host's 8-way lockstep Keccak.  Off:
// measured 244-250 K vs 264-266 K proofs/s at 256 x 12 in flight (three
// interleaved passes, tools/gpu_ab_env_prove.sh) -- the host is not the
// bound (8 of 16 cores busy), and the 4-wave kernel's ~0.3 ms latency
// lands on every batch's critical path.
bool dev_v_transcript() {
  const char* e = getenv("BPP_PROVE_DEV_V");
  return e && atoi(e) != 0;
}

bool deck_host_witness() {
  const char* e = getenv("BPP_DECK_HOST_WITNESS");
  return e && atoi(e) != 0;
}

// BPP_CIRCUIT_HOST_WITNESS=1: a caller-defined circuit's witness on the host
// (circuit::eval, bpp_circuit_eval's code) at every size, for the test that
// compares the two paths
bool circuit_host_witness() {
  const char* e = getenv("BPP_CIRCUIT_HOST_WITNESS");
  return e && atoi(e) != 0;
}

// Per-proof prover state carried between the lockstep phases.  The states
// (and their vectors) persist per driver thread across batches: a host
// profile of 8 batches in flight spent ~20 % of the host CPU in malloc /
// free and arena locks, largely vectors allocated by pool workers and freed
// by the driver thread at the end of every batch.
// Batch-sized host arrays, also reused batch after batch (resize to the same
// size neither allocates nor zero-fills; every element is written before use).
struct ProverScratch {
  std::vector<Enc32> V;
  // A_I/A_O/S MSM terms without the zero padding gates (a_L, a_R, a_O of
  // gates 2k..n_p-1): generator index and source slot in the [P][per]
  // scalar array per term, rebuilt when (P, k, generator set) changes: the
  // indices embed G->n (hidx(i) = n + i, bbidx() = 2n + 1), so one thread
  // proving the same (P, k) against generator sets of different sizes must
  // not reuse them
  std::vector<uint32_t> idx, map, off;
  size_t key_P = 0;
  uint32_t key_k = 0, key_gates = 0, key_np = 0;  // (k, C.n and C.n_p: the circuits of one k differ, a program has k = 0)
  const bpp_gens* key_G = nullptr;
  size_t key_n = 0;
};

struct ProverState {
  merlin::Transcript tr;
  perm::RandomDraws d;  // pi, gamma, alpha, beta, rho, s_L, s_R, tau
  std::vector<Sc> vals, aL, aR, aO;
  std::vector<Sc> cards;  // a caller-supplied deck (k > 768) or a program's inputs, kept for the host witness only
  std::vector<Sc> aux;    // a program's auxiliary values, likewise
  std::vector<Sc> pub;    // a program's public inputs, likewise
  Sc x_perm, w;
  Sc t[7];
};

std::vector<std::unique_ptr<ProverState>>& prover_states_tl() {
  static thread_local std::vector<std::unique_ptr<ProverState>> S;
  return S;
}
std::vector<Proof>& proofs_tl() {
  static thread_local std::vector<Proof> Ps;
  return Ps;
}
ProverScratch& prover_scratch_tl() {
  static thread_local ProverScratch scr;
  return scr;
}

// The device workspaces of kSecretWs zeroed by ONE launch (blockIdx.y = span)
// instead of one hipMemsetAsync (a fill kernel each) per workspace.
#define WIPE_MAX 16
struct WipeSpans {
  uint8_t* p[WIPE_MAX];
  uint64_t n[WIPE_MAX];
};
__global__ void __launch_bounds__(256) k_wipe_spans(WipeSpans w) {
  uint8_t* p = w.p[blockIdx.y];
  const uint64_t n = w.n[blockIdx.y], n16 = n >> 4;  // (hipMalloc'd: 16-B aligned)
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x)
    reinterpret_cast<uint4*>(p)[i] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0 && threadIdx.x < (n & 15)) p[n16 * 16 + threadIdx.x] = 0;
}

}  // namespace

namespace perm_impl BPP_HIDDEN {

// Wipes what the last batch proved on this thread and context left of its
// secrets: the pinned-arena spans the batch staged secrets in
// (draw templates and pi; the witness and blindings on the host-witness path,
// k > 768), the device workspaces holding blindings, witness and the l / r
// vectors, the host buffers of the T-commitment inputs, and the calling
// thread's reused prover states and proof objects (pi).  Called by the
// production entry point (bpp_perm_prove_batch_entropy) on its context, and
// by each sub-batch thread on its child context (BPP_PROVE_STREAMS > 1).
static const char* const kSecretWs[] = {"pb_rng_in", "pb_gamma", "mt_s",  "pv_v",   "pv_g",    "pv_gx",  "poly_vec",
                                        "poly_hf",   "pf_l",     "pf_r",  "ipa_am", "ipa_bm",  "ipa_am1", "ipa_bm1",
                                        "wp_wires",      // (k_witness_program_wide's wires)
                                        "pb_aux_hint",   // (k_hint_aux's derived auxiliary values)
                                        "rs_secret"};    // (the re-shuffle prover's draws, perms, b, d, delta, r Bb)
static const char* const kSecretHost[] = {"pp_v", "pp_g", "ipa_zc_a", "ipa_zc_b"};  // (ipa_zc_*: bpp_ipa_prove zeroes them itself)
int prove_wipe(bpp_ctx* ctx) {
  WipeSpans w = {};
  uint32_t cnt = 0;
  uint64_t most = 0;
  // one launch per WIPE_MAX live workspaces (one, unless a context has proved with every prover)
  auto flush = [&]() -> int {
    if (!cnt) return BPP_OK;
    const uint32_t bx = (uint32_t)std::min<uint64_t>(64, (most / 16 + 255) / 256 + 1);
    hipLaunchKernelGGL(k_wipe_spans, dim3(bx, cnt), dim3(256), 0, ctx->stream, w);
    cnt = 0;
    most = 0;
    return ctx_check_launch(ctx, "k_wipe_spans");
  };
  for (const char* n : kSecretWs) {
    auto it = ctx->ws.find(n);
    if (it == ctx->ws.end() || !it->second.p || !it->second.bytes) continue;
    w.p[cnt] = (uint8_t*)it->second.p;
    w.n[cnt] = it->second.bytes;
    most = std::max<uint64_t>(most, it->second.bytes);
    if (++cnt == WIPE_MAX) BPP_TRY(flush());
  }
  BPP_TRY(flush());
  BPP_TRY(ctx_sync(ctx));
  for (const char* n : kSecretHost) {
    auto it = ctx->host_bufs.find(n);
    if (it != ctx->host_bufs.end() && it->second.first) memset(it->second.first, 0, it->second.second);
  }
  for (auto& st : ctx->secret_stage) memset(st.first, 0, st.second);
  ctx->wiped.swap(ctx->secret_stage);
  ctx->secret_stage.clear();
  for (auto& S : prover_states_tl()) {
    perm::RandomDraws& d = S->d;
    std::fill(d.pi.begin(), d.pi.end(), 0u);
    for (auto* v : {&d.gamma, &d.sL, &d.sR, &d.taus, &S->vals, &S->aL, &S->aR, &S->aO, &S->cards, &S->aux})
      std::fill(v->begin(), v->end(), hsc::zero());
    d.alpha = d.beta = d.rho = hsc::zero();
    for (Sc& t : S->t) t = hsc::zero();
  }
  for (Proof& P : proofs_tl()) std::fill(P.pi.begin(), P.pi.end(), 0u);
  return BPP_OK;
}

// Test hook (bpp_debug_secret_residue): nonzero bytes left in what prove_wipe
// zeroes on ctx and its child contexts (device workspaces, host buffers, the
// arena spans of the last wipe).
int secret_residue(bpp_ctx* ctx, uint64_t* nz) {
  std::vector<uint8_t> h;
  for (const char* n : kSecretWs) {
    auto it = ctx->ws.find(n);
    if (it == ctx->ws.end() || !it->second.p) continue;
    h.resize(it->second.bytes);
    BPP_HIP(hipMemcpy(h.data(), it->second.p, h.size(), hipMemcpyDeviceToHost));
    for (uint8_t b : h) *nz += b != 0;
  }
  for (const char* n : kSecretHost) {
    auto it = ctx->host_bufs.find(n);
    if (it == ctx->host_bufs.end() || !it->second.first) continue;
    const uint8_t* b = (const uint8_t*)it->second.first;
    for (size_t i = 0; i < it->second.second; ++i) *nz += b[i] != 0;
  }
  for (auto& st : ctx->wiped)
    for (size_t i = 0; i < st.second; ++i) *nz += st.first[i] != 0;
  for (bpp_ctx* kid : ctx->children)
    if (kid) BPP_TRY(secret_residue(kid, nz));
  return BPP_OK;
}

}  // namespace perm_impl

namespace {

// One batch of the lockstep prover: what its phases share, and the phases in
// the order prove_batch runs them (each named after its HostScope stage).
struct ProveBatch {
  bpp_ctx* const ctx;
  const bpp_gens* const G;
  const perm::Circuit& C;
  const std::vector<perm::Seed>& seeds;
  const uint8_t* const label;
  const size_t llen;
  std::vector<Proof>& Ps;
  const ProveInputs* const in;  // a caller's witness (nullptr: the seed's own)
  const size_t P = seeds.size();
  const uint32_t k = C.k, n_p = C.n_p, m = C.m;
  const uint32_t nv = C.nv;          // V commitments before x_perm (2k; the deck circuit's k)
  const uint32_t per = 3 + 5 * n_p;  // A_I/A_O/S terms per proof
  // the witness on the device (k_witness, k_witness_deck) while its prefix
  // products fit the workgroup's LDS; the host restatement beyond that
  // (BPP_DECK_HOST_WITNESS=1: the deck circuit's host witness at every k, for
  // the test that compares the two paths)
  // a caller-defined circuit's device witness has no size bound: witness_program_dev
  // picks the kernel by the wires' size and the TILED flag (LDS, or global memory
  // for a large circuit); BPP_CIRCUIT_HOST_WITNESS=1: its host witness at every size
  const bool dev_witness = C.program ? !circuit_host_witness()
                           : C.deck  ? k <= DECK_WITNESS_DEV_MAX && !deck_host_witness()
                                     : k <= perm::chain_witness_dev_max(2);
  // (a plain reference: pool workers must reach THIS thread's states, a
  // thread_local named inside their lambdas would be their own)
  std::vector<std::unique_ptr<ProverState>>& S = prover_states_tl();
  ProverScratch& scr = prover_scratch_tl();
  std::vector<merlin::Transcript*> trs = std::vector<merlin::Transcript*>(P);  // this batch's (lockstep_phase)
  // device arrays: the drawn blindings [P][m], the A_I/A_O/S scalars [P][per], pi, the V phase's values /
  // blindings [P][nv] and gamma_nv / 2 [P] ("pv_v", "pv_g", "pv_gx", taken once), and the IPA inputs
  uint32_t *d_gamma = nullptr, *d_s = nullptr, *d_pi = nullptr;
  uint32_t *d_v = nullptr, *d_g = nullptr, *d_gx_half = nullptr;
  const uint32_t* d_aux = nullptr;  // a program's auxiliary values [P][n_aux]: uploaded, or derived ("pb_aux_hint")
  // no aux rows on a circuit with hints: derived (k_hint_aux; late hints in the witness kernel), and nothing of
  // them is staged or uploaded
  const bool derive_aux = C.program && in && circuit::aux_derived(*C.program, in->aux.p);
  const uint32_t* d_pub = nullptr;  // a program's uploaded public inputs [P][n_pub]
  uint32_t *d_l = nullptr, *d_r = nullptr, *d_hf = nullptr;
  MsmPoints pts;
  std::vector<Sc> zwvg = std::vector<Sc>(P);  // <z^Q W_V, gamma> per proof (k_poly_coef)

  ProveBatch(bpp_ctx* ctx_, const bpp_gens* G_, const perm::Circuit& C_, const std::vector<perm::Seed>& seeds_,
             const uint8_t* label_, size_t llen_, std::vector<Proof>& Ps_, const ProveInputs* in_)
      : ctx(ctx_), G(G_), C(C_), seeds(seeds_), label(label_), llen(llen_), Ps(Ps_), in(in_) {
    while (S.size() < P) S.emplace_back(new ProverState());
    par::for_each(P, [&](size_t p) { S[p]->tr = merlin::Transcript(label, llen); });
    for (size_t p = 0; p < P; ++p) trs[p] = &S[p]->tr;
  }

  int draws_upload();         // pb_rng
  int pedersen_V();           // pb_pedersen_V
  int pedersen_Vx_witness();  // pb_pedersen_Vx_witness
  int msm_AI_AO_S();          // pb_msm_AI_AO_S
  int host_poly();            // pb_host_poly
  int pedersen_T_lr();        // pb_pedersen_T_lr
  int ipa();                  // pb_ipa
};

// the transcript phases' groups run on the host pool (merlin::lockstep_phase)
const auto for_groups = [](size_t n, const std::function<void(size_t)>& f) { par::for_each(n, f); };
// a scalar's 32 canonical bytes, as append_scalar appends them
const uint8_t* sc_bytes(const Sc& s) { return reinterpret_cast<const uint8_t*>(s.v); }

// RNG draws (perm.h draw_prover_randomness): the host makes pi (its short
// SHAKE256 streams, 8-way AVX-512 Keccak) and alpha, beta, rho, tau; the
// GPU makes the 2 n_p + m + 3 indexed scalar draws its kernels use (k_draws:
// gamma -> [P][m], alpha .. s_R -> their slots of the A_I/A_O/S scalar
// array) from per-proof sponge templates written straight into the pinned
// upload arena
int ProveBatch::draws_upload() {
  HostScope hs(ctx, "pb_rng");
  void* dst = nullptr;
  for (const perm::Seed& sd : seeds)
    if (sd.len != seeds[0].len) {
      ctx->err = "prove_batch: seeds of different lengths in one batch";
      return BPP_ERR_ARG;
    }
  if (C.program && !(in && in->values.p && (in->aux.p || !C.program->n_aux || derive_aux) && (in->pub.p || !C.n_pub))) {
    ctx->err = "prove_batch: a caller-defined circuit takes the caller's v, aux and public inputs";
    return BPP_ERR_ARG;
  }
  if (C.deck && !in) {
    ctx->err = "prove_batch: the deck circuit takes a caller's perms";
    return BPP_ERR_ARG;
  }
  BPP_TRY(ctx_ws(ctx, "pb_gamma", (size_t)P * m * 32, (void**)&d_gamma));
  BPP_TRY(ctx_ws(ctx, "mt_s", (size_t)P * per * 32 + 32, (void**)&d_s));
  // one device buffer filled by one copy (the deck circuit's cards are the
  // call's, public: "pb_deck" below)
  const StageLayout L(P, k, in);
  BPP_TRY(ctx_ws(ctx, "pb_rng_in", L.bytes, &dst));
  // (one staging region: a second take could recycle the arena under the first;
  // read in place instead, by k_draws through LDS, measured within noise)
  uint8_t* stage = nullptr;
  BPP_TRY(ctx_h2d_stage(ctx, L.bytes, &stage));
  ctx_secret_span(ctx, stage, L.bytes);  // (prove_wipe)
  memset(stage + L.pad, 0, L.pad_bytes);  // (the alignment gap is uploaded too)
  par::for_each((P + 7) / 8, [&](size_t gi) {
    perm::Seed sd[8];
    perm::RandomDraws* d[8];
    perm::RandomDraws spare;  // a short last group's padding lanes
    for (size_t j = 0; j < 8; ++j) {
      const bool real = 8 * gi + j < P;
      sd[j] = seeds[std::min(8 * gi + j, P - 1)];
      d[j] = real ? &S[8 * gi + j]->d : &spare;
    }
    perm::draw_prover_host_x8(C, sd, d, !in);
    for (size_t j = 0; j < 8 && 8 * gi + j < P; ++j) {
      const size_t i = 8 * gi + j;
      ProverState& st = *S[i];
      if (in) {
        st.d.pi.clear();
        if (in->perms) st.d.pi.assign(in->perms + i * k, in->perms + (i + 1) * k);
        for (const StageLayout::Rows* r : {&L.values, &L.aux, &L.gammas, &L.pub}) r->stage(stage, i);
        if (!dev_witness) {  // the host witness's own copies (canonical Sc == its 32 bytes)
          auto keep = [&](std::vector<Sc>& v, const ScalarRows& src) {
            v.resize(src.p ? src.per : 0);
            if (src.p) memcpy(v.data(), src.at(i), 32 * (size_t)src.per);
          };
          keep(st.cards, in->values);
          keep(st.aux, in->aux);
          keep(st.pub, in->pub);
          if (derive_aux) {  // the host witness's aux from the host hints (with late hints: once x exists)
            st.aux.assign(C.program->n_aux, hsc::zero());
            if (!circuit::has_late_hints(*C.program))
              circuit::hint_eval(*C.program, st.cards.data(), st.pub.data(), st.aux.data());
          }
        }
      }
      perm::transcript_prefix(C, st.tr);
      // (BPP_PROVE_DEV_V=1 replaces this state with the device's, which absorbs the same)
      if (C.n_pub) perm::transcript_pub(C, st.tr, in->pub.at(i));
      uint64_t tm[7];
      draw_template(sd[j], tm);
      memcpy(stage + L.tmpl + i * sizeof tm, tm, sizeof tm);
      if (k) memcpy(stage + L.pi + i * 4 * (size_t)k, st.d.pi.data(), 4 * (size_t)k);
    }
  });
  BPP_TRY(ctx_h2d_staged(ctx, dst, stage, L.bytes));
  ctx_work(ctx, "prove_stage_bytes", L.bytes);
  const uint8_t* base = (const uint8_t*)dst;
  d_pi = (uint32_t*)(base + L.pi);
  BPP_TRY(ctx_ws(ctx, "pv_v", (size_t)P * nv * 32, (void**)&d_v));
  BPP_TRY(ctx_ws(ctx, "pv_g", (size_t)P * nv * 32, (void**)&d_g));
  BPP_TRY(ctx_ws(ctx, "pv_gx", (size_t)P * 32, (void**)&d_gx_half));  // gamma_nv / 2 for V_nv
  const uint64_t* d_tmpl = (const uint64_t*)(base + L.tmpl);
  // the seed's own witness: the V commitments' inputs (values 1..k and pi + 1,
  // gamma copies and gamma_2k / 2) in the draws' launch
  if (!in) return draws_dev(ctx, C, (uint32_t)P, d_tmpl, seeds[0].len, per, d_gamma, d_s, d_pi, d_v, d_g, d_gx_half);
  // a caller's: the draws alone, then the V inputs from the uploaded rows (and
  // the caller's blindings over the drawn gamma_0..nv-1)
  d_aux = L.aux.dev(dst);
  d_pub = L.pub.dev(dst);
  const uint32_t* d_src = L.values.dev(dst);
  if (derive_aux && dev_witness) {  // k_hint_aux over the uploaded v and pub rows, in front of k_witness_program
    uint32_t* d_hint = nullptr;
    BPP_TRY(ctx_ws(ctx, "pb_aux_hint", (size_t)P * C.program->n_aux * 32, (void**)&d_hint));
    BPP_TRY(hint_aux_dev(ctx, C, (uint32_t)P, d_src, d_pub, d_hint));
    d_aux = d_hint;
  }
  if (C.deck) {
    void* d_deck = nullptr;
    BPP_TRY(ctx_ws(ctx, "pb_deck", (size_t)k * 32, &d_deck));
    BPP_TRY(ctx_h2d_const(ctx, "pb_deck", d_deck, C.cards.data(), (size_t)k * 32));
    d_src = (const uint32_t*)d_deck;
  }
  BPP_TRY(draws_dev(ctx, C, (uint32_t)P, d_tmpl, seeds[0].len, per, d_gamma, d_s));
  return v_inputs_dev(ctx, C, (uint32_t)P, d_src, in->values.per, in->perms ? d_pi : nullptr, nv - in->n_perm,
                      L.gammas.dev(dst), d_gamma, d_v, d_g, d_gx_half);
}

// V_0..V_{nv-1} of every proof (nv = 2k, or the deck circuit's k): one
// fixed-base launch over device inputs (values 1..k, pi + 1 and gamma, written
// by k_draws; a caller's, by k_v_inputs), encodings back to the host
int ProveBatch::pedersen_V() {
  HostScope hs(ctx, "pb_pedersen_V");
  const size_t nv = (size_t)P * this->nv;  // (all proofs')
  uint32_t* denc = nullptr;  // encodings written in place by k_compress_p3 (ctx_zc_out)
  BPP_TRY(ctx_zc_out(ctx, "pv_enc_h", nv * 32, &denc));
  // the nv V appends and x_perm on the device (k_prove_v_transcript, one
  // lane per proof; the host's share of a batch was ~10 us of CPU per
  // proof here, its largest transcript phase): encodings to the device,
  // copied back for the proofs, and the transcript states imported after
  const bool dev_v = dev_v_transcript();
  uint8_t* h_st = nullptr;
  uint32_t* h_xp = nullptr;
  {
    HostScope hk(ctx, "ped_kernels");
    void* dvenc = nullptr;
    if (dev_v) BPP_TRY(ctx_ws(ctx, "pv_enc_d", nv * 32, &dvenc));
    // (values 1..k and pi + 1 <= k: the public bound k + 1; a caller's
    // cards are secret full-width scalars: no bound, every digit position
    // walked whatever the value, as for gamma)
    BPP_TRY(pedersen_dev(ctx, G, d_v, d_g, nv, dev_v ? (uint32_t*)dvenc : denc, nullptr,
                         in ? 0 : (uint64_t)k + 1));
    if (dev_v) {
      BPP_HIP(hipMemcpyAsync(denc, dvenc, nv * 32, hipMemcpyDeviceToHost, ctx->stream));
      uint32_t init[52], *h_init = nullptr;
      verify_init_state(C, label, llen, init);  // (the same shared prefix as the verifier's)
      BPP_TRY(ctx_zc_in(ctx, "pv_init", init, sizeof init, &h_init));
      uint32_t* hs_ = nullptr;
      BPP_TRY(ctx_zc_out(ctx, "pv_states", P * MERLIN_DEV_STATE_BYTES, &hs_));
      BPP_TRY(ctx_zc_out(ctx, "pv_xperm", P * 32, &h_xp));
      h_st = (uint8_t*)hs_;
      BPP_TRY(prove_v_transcript_dev(ctx, (uint32_t)P, this->nv, h_init, (const uint32_t*)dvenc, h_st, h_xp, C.n_pub,
                                     d_pub));
    }
  }
  std::vector<Enc32>& V = scr.V;
  V.resize(nv);
  {
    HostScope hd(ctx, "ped_d2h");
    BPP_TRY(ctx_sync(ctx));
    memcpy(V.data(), denc, nv * 32);
  }
  par::for_each(P, [&](size_t p) {
    Ps[p].V.assign(V.begin() + p * this->nv, V.begin() + (p + 1) * this->nv);
    if (dev_v) {
      merlin_state_import(S[p]->tr, h_st + p * MERLIN_DEV_STATE_BYTES);
      memcpy(&S[p]->x_perm, h_xp + 8 * p, 32);  // (canonical Sc == its 32 bytes)
    }
  });
  if (!dev_v) {
    // the nv "V" appends and x_perm of eight proofs at a time in lockstep
    // on the 8-way Keccak (byte-identical; 2.5x on this phase's ~26 us of
    // permutations per proof)
    merlin::lockstep_phase(
        trs, for_groups, this->nv, [](size_t) { return "V"; },
        [&](size_t p, size_t i) { return V[p * this->nv + i].data(); }, 1, [](size_t) { return "x_perm"; },
        [&](size_t p, size_t, const Sc& c) { S[p]->x_perm = c; });
  }
  return BPP_OK;
}

// V_nv = commit(x_perm, gamma_nv): halved scalars (x_perm / 2 from the
// host, gamma_nv / 2 from k_draws), encoded as 2 (C / 2) on the host
int ProveBatch::pedersen_Vx_witness() {
  HostScope hs(ctx, "pb_pedersen_Vx_witness");
  std::vector<Sc> vh(2 * P);  // x_perm / 2 (V_2k), then x_perm (the device witness)
  for (size_t p = 0; p < P; ++p) {
    vh[p] = hsc::half(S[p]->x_perm);
    vh[P + p] = S[p]->x_perm;
  }
  uint32_t* d_vh = nullptr;
  BPP_TRY(upload_sc(ctx, vh, "pv_vx", &d_vh));
  // (a caller's shuffle: both chains' values, as committed)
  uint32_t* h_fail = nullptr;  // a program's failing assert per proof, written in place (ctx_zc_out)
  if (dev_witness && C.program) {
    BPP_TRY(ctx_zc_out(ctx, "wp_fail_h", P * 4, &h_fail));
    BPP_TRY(witness_program_dev(ctx, C, (uint32_t)P, d_v, d_aux, d_vh + 8 * P, per, d_s, h_fail, d_pub, derive_aux));
  } else if (dev_witness) {
    if (C.deck)
      BPP_TRY(witness_deck_dev(ctx, C, (uint32_t)P, d_v, d_vh + 8 * P, per, d_s));
    else
      BPP_TRY(witness_dev(ctx, C, (uint32_t)P, d_pi, d_vh + 8 * P, per, d_s, in ? d_v : nullptr));
  }
  uint32_t* h_p3 = nullptr;  // written in place by the kernel (ctx_zc_out)
  BPP_TRY(ctx_zc_out(ctx, "pv_p3_h", P * P3_BYTES, &h_p3));
  BPP_TRY(pedersen_dev(ctx, G, d_vh, d_gx_half, P, nullptr, h_p3));
  std::vector<Enc32> Vx(P);
  BPP_TRY(ctx_sync(ctx));
  BPP_TRY(points_double_encode_host(ctx, h_p3, P, Vx[0].data()));
  std::vector<uint32_t> bad(P, 0);  // a program's 1 + first failing assert
  if (h_fail) memcpy(bad.data(), h_fail, P * 4);
  par::for_each(P, [&](size_t p) {
    Ps[p].V.push_back(Vx[p]);
    S[p]->tr.append_point("V", Vx[p].data());
    if (!dev_witness) {
      ProverState& st = *S[p];
      if (C.program && derive_aux && circuit::has_late_hints(*C.program))
        circuit::hint_eval_x(*C.program, st.cards.data(), st.pub.data(), st.x_perm, st.aux.data());
      if (C.program)
        circuit::eval(*C.program, n_p, st.cards.data(), st.aux.data(), st.x_perm, st.aL, st.aR, st.aO, &bad[p],
                      st.pub.data());
      else if (C.deck)
        perm::witness_deck(C, st.d.pi, st.x_perm, st.vals, st.aL, st.aR, st.aO);
      else if (in)
        perm::witness(C, st.cards.data(), st.d.pi, st.x_perm, st.vals, st.aL, st.aR, st.aO);
      else
        perm::witness(C, st.d.pi, st.x_perm, st.vals, st.aL, st.aR, st.aO);
    }
  });
  for (size_t p = 0; p < P; ++p)
    if (bad[p]) {
      ctx->err = "circuit proof " + std::to_string((in ? in->first : 0) + p) + ": assert " +
                 std::to_string(bad[p] - 1) + " does not hold";
      return BPP_ERR_ARG;
    }
  return gens_points(ctx, G, &pts);  // (the MSM and IPA phases' points)
}

// A_I, A_O, S of every proof: one batch of 3P MSMs over the [P][per]
// scalar array that k_draws_reduce (alpha, beta, rho, s_L, s_R) and
// k_witness (a_L, a_R, a_O) filled -- or, beyond the device witness's
// size, the host writes its first 3 + 3 n_p scalars.  The MSMs skip the
// padding gates' zero a_L, a_R, a_O (11 % of the terms at k = 52).
int ProveBatch::msm_AI_AO_S() {
  HostScope hs(ctx, "pb_msm_AI_AO_S");
  const uint32_t hostw = 3 + 3 * n_p;  // host-written scalars per proof
  std::vector<uint32_t>&idx = scr.idx, &map = scr.map, &off = scr.off;
  const uint32_t n = C.n;                       // real gates; n_p - n padding gates are zero
  const uint32_t per_c = 3 + 3 * n + 2 * n_p;  // MSM terms per proof
  if (scr.key_P != P || scr.key_k != k || scr.key_gates != n || scr.key_np != n_p || scr.key_G != G || scr.key_n != G->n) {
    idx.resize((size_t)P * per_c);
    map.resize((size_t)P * per_c);
    off.resize(3 * P + 1);
    for (size_t p = 0; p < P; ++p) {
      size_t t = p * per_c;
      const uint32_t b = (uint32_t)(p * per);
      auto term = [&](uint32_t src, uint32_t gen) {
        map[t] = b + src;
        idx[t++] = gen;
      };
      off[3 * p] = (uint32_t)t;
      term(0, G->bbidx());                                                  // alpha
      for (uint32_t i = 0; i < n; ++i) term(1 + i, G->gidx(i));             // a_L
      for (uint32_t i = 0; i < n; ++i) term(1 + n_p + i, G->hidx(i));       // a_R
      off[3 * p + 1] = (uint32_t)t;
      term(1 + 2 * n_p, G->bbidx());                                        // beta
      for (uint32_t i = 0; i < n; ++i) term(2 + 2 * n_p + i, G->gidx(i));   // a_O
      off[3 * p + 2] = (uint32_t)t;
      term(2 + 3 * n_p, G->bbidx());                                        // rho
      for (uint32_t i = 0; i < n_p; ++i) term(3 + 3 * n_p + i, G->gidx(i));  // s_L
      for (uint32_t i = 0; i < n_p; ++i) term(3 + 4 * n_p + i, G->hidx(i));  // s_R
    }
    off[3 * P] = (uint32_t)(P * per_c);
    scr.key_P = P;
    scr.key_k = k;
    scr.key_gates = n;
    scr.key_np = n_p;
    scr.key_G = G;
    scr.key_n = G->n;
  }
  uint8_t* stg = nullptr;  // (host witness only) written in place in the pinned arena
  if (!dev_witness) {
    BPP_TRY(ctx_h2d_stage(ctx, (size_t)P * hostw * 32, &stg));
    ctx_secret_span(ctx, stg, (size_t)P * hostw * 32);  // (prove_wipe)
    par::for_each(P, [&](size_t p) {
      ProverState& st = *S[p];
      Sc* o = reinterpret_cast<Sc*>(stg) + p * hostw;
      o[0] = st.d.alpha;
      std::copy(st.aL.begin(), st.aL.begin() + n_p, o + 1);
      std::copy(st.aR.begin(), st.aR.begin() + n_p, o + 1 + n_p);
      o[1 + 2 * n_p] = st.d.beta;
      std::copy(st.aO.begin(), st.aO.begin() + n_p, o + 2 + 2 * n_p);
      o[2 + 3 * n_p] = st.d.rho;
    });
    BPP_HIP(hipMemcpy2DAsync(d_s, (size_t)per * 32, stg, (size_t)hostw * 32, (size_t)hostw * 32, P,
                             hipMemcpyHostToDevice, ctx->stream));
  }
  void *d_i = nullptr, *d_map = nullptr;
  BPP_TRY(ctx_ws(ctx, "mt_i", idx.size() * 4 + 4, &d_i));
  BPP_TRY(ctx_h2d_const(ctx, "mt_i", d_i, idx.data(), idx.size() * 4));  // generator indices: same every batch
  BPP_TRY(ctx_ws(ctx, "mt_map", map.size() * 4 + 4, &d_map));
  BPP_TRY(ctx_h2d_const(ctx, "mt_map", d_map, map.data(), map.size() * 4));
  // MSMs of the halved, compacted scalars, encoded as 2 * result (msm_multi_enc)
  // (gathered and halved inside the direct-table kernel: d_map)
  std::vector<uint8_t> enc(3 * P * 32);
  BPP_TRY(msm_multi_enc(ctx, d_s, (const uint32_t*)d_i, off, pts, enc.data(), true, (const uint32_t*)d_map));
  par::for_each(P, [&](size_t p) {
    memcpy(Ps[p].AI.data(), &enc[96 * p], 32);
    memcpy(Ps[p].AO.data(), &enc[96 * p + 32], 32);
    memcpy(Ps[p].S.data(), &enc[96 * p + 64], 32);
  });
  return BPP_OK;
}

// challenges y, z (host transcripts), then the t(X) coefficients and
// tau_x's <z^Q W_V, gamma> of every proof in one device launch (poly.hip)
int ProveBatch::host_poly() {
  HostScope hs(ctx, "pb_host_poly");
  std::vector<Sc> yinv(P), ch((size_t)P * 3), tco;
  static const char* const lab[3] = {"A_I", "A_O", "S"};
  merlin::lockstep_phase(
      trs, for_groups, 3, [](size_t i) { return lab[i]; },
      [&](size_t p, size_t i) { return (i == 0 ? Ps[p].AI : i == 1 ? Ps[p].AO : Ps[p].S).data(); }, 2,
      [](size_t c) { return c ? "z" : "y"; },
      [&](size_t p, size_t c, const Sc& v) {
        if (c == 0) yinv[p] = v;
        ch[3 * p + 2 * c] = v;  // (y, 1 / y, z)
      });
  hsc::batch_invert(yinv, false, true);  // (y: public challenges)
  for (size_t p = 0; p < P; ++p) ch[3 * p + 1] = yinv[p];
  BPP_TRY(poly_coef_dev(ctx, C, (uint32_t)P, d_s, per, d_gamma, ch, tco));
  for (size_t p = 0; p < P; ++p) {
    for (int j = 0; j < 6; ++j) S[p]->t[1 + j] = tco[7 * p + j];
    zwvg[p] = tco[7 * p + 6];
  }
  return BPP_OK;
}

// T1, T3..T6 of every proof: one fixed-base launch; then x, the l / r
// vectors and t_hat on the device, tau_x and mu on the host, and w
int ProveBatch::pedersen_T_lr() {
  HostScope hs(ctx, "pb_pedersen_T_lr");
  static const int ti[5] = {1, 3, 4, 5, 6};
  std::vector<Sc> v(5 * P), g(5 * P);
  for (size_t p = 0; p < P; ++p)
    for (int i = 0; i < 5; ++i) {
      v[5 * p + i] = S[p]->t[ti[i]];
      g[5 * p + i] = S[p]->d.taus[i];
    }
  std::vector<Enc32> T;
  {
    HostScope hs2(ctx, "pbT_pedersen");
    BPP_TRY(pedersen_host(ctx, G, v, g, T));
  }
  HostScope hs3(ctx, "pbT_host");
  std::vector<Sc> xs(P), t_hat;
  static const char* const Tlab[5] = {"T1", "T3", "T4", "T5", "T6"};
  for (size_t p = 0; p < P; ++p)
    for (int i = 0; i < 5; ++i) Ps[p].T[i] = T[5 * p + i];
  merlin::lockstep_phase(
      trs, for_groups, 5, [](size_t i) { return Tlab[i]; }, [&](size_t p, size_t i) { return Ps[p].T[i].data(); }, 1,
      [](size_t) { return "x"; }, [&](size_t p, size_t, const Sc& c) { xs[p] = c; });
  BPP_TRY(poly_x_dev(ctx, C, (uint32_t)P, xs, &d_l, &d_r, &d_hf, t_hat));
  par::for_each(P, [&](size_t p) {
    ProverState& st = *S[p];
    Proof& Pf = Ps[p];
    const Sc x = xs[p];
    Sc xp[7];
    xp[0] = hsc::one();
    for (int i = 1; i < 7; ++i) xp[i] = hsc::mul(xp[i - 1], x);
    using hsc::add;
    Sc tau_x = hsc::mul(xp[2], zwvg[p]);
    for (int i = 0; i < 5; ++i) tau_x = add(tau_x, hsc::mul(st.d.taus[i], xp[ti[i]]));
    Pf.tau_x = tau_x;
    Pf.mu = add(add(hsc::mul(st.d.alpha, x), hsc::mul(st.d.beta, xp[2])), hsc::mul(st.d.rho, xp[3]));
    Pf.t_hat = t_hat[p];
  });
  static const char* const slab[3] = {"TX", "mu", "t"};
  merlin::lockstep_phase(
      trs, for_groups, 3, [](size_t i) { return slab[i]; },
      [&](size_t p, size_t i) { return sc_bytes(i == 0 ? Ps[p].tau_x : i == 1 ? Ps[p].mu : Ps[p].t_hat); }, 1,
      [](size_t) { return "w"; }, [&](size_t p, size_t, const Sc& c) { S[p]->w = c; });
  return BPP_OK;
}

// IPA of every proof in lockstep
int ProveBatch::ipa() {
  HostScope hs(ctx, "pb_ipa");
  std::vector<Sc> qmul(P);
  for (size_t p = 0; p < P; ++p) qmul[p] = S[p]->w;
  IpaGens ig;
  ig.pts = pts;
  ig.gbase = 0;
  ig.hbase = (uint32_t)G->n;
  ig.qidx = G->bidx();
  static thread_local std::vector<IpaProofHost> ipas;
  BPP_TRY(ipa_prove_batch_dev(ctx, trs, ig, n_p, nullptr, d_hf, d_l, d_r, qmul, ipas));
  for (size_t p = 0; p < P; ++p) std::swap(Ps[p].ipa, ipas[p]);  // (both keep their capacity)
  for (size_t p = 0; p < P; ++p) Ps[p].pi.assign(S[p]->d.pi.begin(), S[p]->d.pi.end());
  return BPP_OK;
}

}  // namespace

namespace perm_impl BPP_HIDDEN {

// Proves `seeds.size()` permutation proofs in lockstep: every GPU step
// (Pedersen V, Pedersen V_2k, the A_I/A_O/S MSMs, Pedersen T, each IPA
// round) is ONE launch sequence for the whole batch, and the per-proof host
// work between them (transcripts, challenges, polynomial coefficients) runs
// on a thread pool.  Outputs are identical to proving one at a time.
// The statement is C's and the witness the seed's or, with `in`, the caller's
// (no pi stream is read then, and the V commitments take full-width values);
// every step but these is the same launch sequence:
//   statement         transcript starts  V inputs (nv)                    witness
//   two-half, seeded  k                  k_draws: 1..k, pi + 1 (2k)       k_witness / perm::witness
//   two-half, `in`    k                  k_v_inputs: cards, cards[perm]   k_witness_cards / perm::witness
//   deck              deck digest        k_v_inputs: deck[perm] (k)       k_witness_deck / perm::witness_deck
//   circuit           program digest,    k_v_inputs: v (m_in)             k_witness_program / circuit::eval;
//                     then in->pub                                        an assert that does not hold ends
//                                                                         the batch with BPP_ERR_ARG
int prove_batch(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const std::vector<perm::Seed>& seeds,
                const uint8_t* label, size_t llen, std::vector<Proof>& Ps, const ProveInputs* in) {
  const size_t P = seeds.size();
  Ps.resize(P);
  if (!P) return BPP_OK;
  // A small batch is a latency chain (a config-4 job's sub-batches): its
  // syncs spin before sleeping; the throughput shape (384 proofs, 32 in
  // flight) keeps the sleeping wait that frees the host cores
  constexpr size_t spin_batch = 128;  // the largest batch that spins
  SyncSpin spin(ctx, P <= spin_batch ? 300u : ctx->sync_spin_us);
  ProveBatch b(ctx, G, C, seeds, label, llen, Ps, in);
  BPP_TRY(b.draws_upload());
  BPP_TRY(b.pedersen_V());
  BPP_TRY(b.pedersen_Vx_witness());
  BPP_TRY(b.msm_AI_AO_S());
  BPP_TRY(b.host_poly());
  BPP_TRY(b.pedersen_T_lr());
  return b.ipa();
}

// wipe: prove_wipe after the batch, on ctx (this thread) and on every child
// context inside its sub-batch thread (whose prover states are its own)
int prove_batch_api(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, const std::vector<perm::Seed>& seeds,
                    const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out, bool wipe,
                    const ProveInputs* in) {
  const size_t count = seeds.size();
  if (!count) return BPP_OK;
  BPP_TRY(gens_cover(ctx, G, C.n_p));
  BPP_HIP(hipSetDevice(ctx->device));
  const size_t pl = perm::proof_len(C);
  std::vector<Proof>& Ps = proofs_tl();  // reused batch after batch (ProverState note; the workers see this thread's)
  Ps.resize(count);
  // Sub-batches in flight on S streams (child contexts), one host thread
  // each: while one sub-batch waits on transcripts / challenges on the host,
  // the others' MSM and Pedersen kernels fill the GPU (a lockstep batch of
  // 128 proofs leaves most SIMDs idle in its latency-bound launch tails).
  // (default 1 until the concurrent path measures faster)
  size_t S = 1;
  if (const char* e = getenv("BPP_PROVE_STREAMS")) S = std::max<size_t>(1, std::min<size_t>(count, atoi(e)));
  {
    MsmPoints warm;  // build the window tables once, before the threads
    BPP_TRY(gens_points(ctx, G, &warm));
  }
  if (S <= 1) {
    BPP_TRY(prove_batch(ctx, G, C, seeds, label, llen, Ps, in));
  } else {
    std::vector<bpp_ctx*> kids(S);
    for (size_t s = 0; s < S; ++s) BPP_TRY(ctx_child(ctx, s, &kids[s]));
    std::vector<int> rcs(S, BPP_OK);
    std::vector<std::thread> th;
    for (size_t s = 0; s < S; ++s)
      th.emplace_back([&, s] {
        const size_t b = count * s / S, e = count * (s + 1) / S;
        bpp_ctx* kc = kids[s];
        kc->prof = ctx->prof;
        if (hipSetDevice(ctx->device) != hipSuccess) {
          rcs[s] = BPP_ERR_DEVICE;
          return;
        }
        std::vector<Proof> sub;
        std::vector<perm::Seed> part(seeds.begin() + b, seeds.begin() + e);
        const ProveInputs sub_in = in ? in->slice(b) : ProveInputs();  // this sub-batch's rows
        rcs[s] = prove_batch(kc, G, C, part, label, llen, sub, in ? &sub_in : nullptr);
        if (rcs[s] == BPP_OK)
          for (size_t i = b; i < e; ++i) Ps[i] = std::move(sub[i - b]);
        if (wipe) {
          for (perm::Seed& x : part) memset(x.b, 0, sizeof x.b);
          for (Proof& q : sub) std::fill(q.pi.begin(), q.pi.end(), 0u);
          const int w = prove_wipe(kc);
          if (rcs[s] == BPP_OK) rcs[s] = w;
        }
      });
    for (auto& t : th) t.join();
    // (the children's stage times fold into ctx's on its next profile query)
    for (size_t s = 0; s < S; ++s)
      if (rcs[s] != BPP_OK) {
        ctx->err = kids[s]->err;
        return rcs[s];
      }
  }
  par::for_each(count, [&](size_t p) {
    serialize(C, Ps[p], proofs_out + p * pl);
    for (uint32_t j = 0; j < C.m; ++j) memcpy(V_out + (p * C.m + j) * 32, Ps[p].V[j].data(), 32);
  });
  return BPP_OK;
}


// The entropy-seeded provers' common tail (bpp_perm_prove_batch_entropy,
// bpp_perm_prove_shuffle_batch): 32 bytes per proof from the caller or the OS
// CSPRNG (the reference's thread_rng(), circuit_lib.rs:175), the batch proved
// with its wipe, then the entropy and the seeds zeroed -- they live on this
// stack and heap, where bpp_debug_secret_residue does not look -- and ctx's
// own wipe.
int prove_batch_entropy(bpp_ctx* ctx, const bpp_gens* G, const perm::Circuit& C, size_t count, const uint8_t* seeds32,
                        const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out, const ProveInputs* in) {
  std::vector<uint8_t> ent;
  if (!seeds32 && count) {
    ent.resize(32 * count);
    if (!perm::os_entropy(ent.data(), ent.size())) return no_entropy(ctx);
    seeds32 = ent.data();
  }
  std::vector<perm::Seed> sd(count);
  for (size_t i = 0; i < count; ++i) sd[i] = perm::Seed::bytes32(seeds32 + 32 * i);
  const int rc = prove_batch_api(ctx, G, C, sd, label, llen, proofs_out, V_out, true, in);
  if (!ent.empty()) memset(ent.data(), 0, ent.size());
  for (perm::Seed& x : sd) memset(x.b, 0, sizeof x.b);
  const int wrc = prove_wipe(ctx);
  return rc ? rc : wrc;
}

}  // namespace perm_impl
