// Re-shuffle proofs, blind and masked: the C ABI (bpp_reshuffle_* and
// bpp_masked_reshuffle_*, include/bpperm.h), the one prover's and the one
// verifier's launch sequence over reshuffle.hip, written over a kind's data
// (RsKind, reshuffle.h: a card of H points, a key in front or none), and the
// shuffle_of_public(k) program the inner proof runs on.  The inner proof is the
// circuit prover and verifier of perm_prove.hip / perm_verify.hip, unchanged.
// DESIGN.md "Protocol: blind re-shuffle" and "Protocol: masked re-shuffle".
#include <map>
#include <mutex>
#include <string>

#include "gens.h"
#include "host/circuit.h"
#include "layout.h"
#include "merlin_dev.h"
#include "perm_internal.h"
#include "reshuffle.h"

using namespace perm_impl;

// declared in points.hip
__global__ void k_decompress(const uint32_t* __restrict__ enc, size_t n, uint32_t* __restrict__ tbl,
                             unsigned long long* __restrict__ bad);

namespace {
constexpr uint32_t kMaxK = 342;  // 2k - 2 gates within the plain circuit bound of 682
constexpr uint32_t lab(char a, char b = 0) { return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8; }

// gadgets.shuffle_of_public(k), array for array: a chain prod (v_j - x) over
// gates 0..k-2, a chain prod (u_j - x) over gates k-1..2k-3, one assert on the
// difference of their ends.  Compiled once per k and kept.
const perm::Circuit* rs_circuit(uint32_t k) {
  static std::mutex mu;
  static std::map<uint32_t, std::unique_ptr<perm::Circuit>> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto& slot = cache[k];
  if (slot) return slot.get();
  const uint32_t n = 2 * k - 2, X = circuit::var_x(k);
  std::vector<uint32_t> side_aux(2 * n, circuit::SIDE_LC), off{0}, var;
  std::vector<Sc> coef;
  const Sc one = hsc::one(), neg = hsc::sub(hsc::zero(), one);
  auto emit = [&](std::initializer_list<std::pair<uint32_t, Sc>> ts) {
    for (auto& t : ts) {
      var.push_back(t.first);
      coef.push_back(t.second);
    }
    off.push_back((uint32_t)var.size());
  };
  for (uint32_t ch = 0; ch < 2; ++ch) {
    auto lin = [&](uint32_t i) {  // w_i - x, ids ascending
      if (ch == 0)
        emit({{circuit::var_v(i), one}, {X, neg}});
      else
        emit({{X, neg}, {circuit::var_pub(k, i), one}});
    };
    lin(0);
    lin(1);
    for (uint32_t i = 2; i < k; ++i) {
      const uint32_t g = ch * (k - 1) + i - 1;
      emit({{circuit::var_wire(k, g - 1, 2, k), one}});
      lin(i);
    }
  }
  emit({{circuit::var_wire(k, k - 2, 2, k), one}, {circuit::var_wire(k, 2 * k - 3, 2, k), neg}});
  circuit::Desc d = {k, n, 0, 1, side_aux.data(), off.data(), var.data(), (const uint8_t*)coef.data()};
  d.n_pub = k;
  std::unique_ptr<perm::Circuit> C(new perm::Circuit());
  std::string err;
  if (circuit::compile(d, *C, err) != circuit::OK) return nullptr;
  slot = std::move(C);
  return slot.get();
}

size_t rs_inner_len(uint32_t k) {
  uint32_t n_p = 4, lg = 2;
  for (; n_p < 2 * k - 2; n_p *= 2) ++lg;
  return 32 * (13 + 2 * (size_t)lg);
}

// "k is a size this argument takes": BPP_ERR_ARG below 2, BPP_ERR_LEN past 342
int rs_k_check(bpp_ctx* ctx, uint32_t k) {
  if (k < 2) return BPP_ERR_ARG;
  if (k > kMaxK) {
    if (ctx) ctx->err = "reshuffle: k > 342 (the inner circuit's 2k - 2 gates pass the plain bound of 682)";
    return BPP_ERR_LEN;
  }
  return BPP_OK;
}

// the 52 words every proof's transcript starts from: Transcript(label), the
// kind's dom-sep, k, and the key where there is one
void init_state(const RsKind& kd, uint32_t k, const uint8_t* key, const uint8_t* label, size_t llen, uint32_t out[52]) {
  merlin::Transcript tr(label, llen);
  tr.append("dom-sep", (const uint8_t*)kd.dom, strlen(kd.dom));
  tr.append_u64("k", k);
  if (kd.keys) tr.append("K", key, 32);
  memcpy(out, tr.s.st, 200);
  out[50] = tr.s.pos;
  out[51] = tr.s.pos_begin;
}

// k_decompress over n encodings with its verdict word reset (bad: 8 bytes, ~0
// or the first index that does not decode)
int rs_decompress_dev(bpp_ctx* ctx, const uint32_t* d_enc, size_t n, uint32_t* d_tbl, void* d_bad) {
  const unsigned long long init = ~0ull;
  BPP_TRY(ctx_h2d(ctx, d_bad, &init, 8));
  {
    ProfScope ps(ctx, "decompress");
    hipLaunchKernelGGL(k_decompress, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_enc, n, d_tbl,
                       (unsigned long long*)d_bad);
  }
  return ctx_check_launch(ctx, "k_decompress");
}

size_t rs_proof_len(const RsKind& kd, uint32_t k) {
  return k >= 2 && k <= kMaxK ? 32 * (5 * (size_t)k + 2 + kd.H) + rs_inner_len(k) : 0;
}

// proofs per launch sequence: a few million lanes, indices well below 2^31
uint32_t chunk_of(const RsKind& kd, uint32_t k, size_t count) {
  return (uint32_t)std::min<size_t>(count, std::max<size_t>(1, ((size_t)1 << 22) / rs_points(kd.H, k)));
}

// The key of a kind that has none: no bytes, at an address that is not null, so
// the sequences read kd.keys points at `key` whatever the kind.
const uint8_t kNoKey[1] = {0};

// point j of a proof's rs_points(H, k), for an error text
std::string point_name(const RsKind& kd, uint32_t k, size_t j) {
  const size_t deck = (size_t)kd.H * k;
  if (j < 2 * deck)
    return std::string(kd.half[j % kd.H]) + (j < deck ? "input" : "output") + " card " + std::to_string(j % deck / kd.H);
  j -= 2 * deck;
  if (j < 3 * (size_t)k) return std::string(j < k ? "A " : j < 2 * (size_t)k ? "E " : "T ") + std::to_string(j % k);
  return kd.tsum[j - 3 * (size_t)k];
}
int key_undecodable(bpp_ctx* ctx, const RsKind& kd) {
  ctx->err = std::string(kd.name) + ": the key does not decode";
  return BPP_ERR_DECOMPRESS;
}

// s_i times the kind's fixed base -> out [n] extended, by pedersen_dev's walk:
// without a key the cards are re-blinded, s_i Bb as the blinding of the value 0
// (below the public bound 1); with one they are masked, s_i B as the value (no
// public bound) under a zero blinding.
int fixed_base_dev(bpp_ctx* ctx, const bpp_gens* G, const RsKind& kd, const uint32_t* s, const uint32_t* zero, size_t n,
                   uint32_t* out) {
  return kd.keys ? pedersen_dev(ctx, G, s, zero, n, nullptr, out) : pedersen_dev(ctx, G, zero, s, n, nullptr, out, 1);
}

// The three transcript phases over per-proof rows of encodings: the cards in
// [k][H], the cards out [k][H], A -> x; E -> y; Ti, the H sums -> c.  s_* : words
// between two proofs' rows.
struct Rows {
  const uint32_t *C, *Co, *A, *E, *Ti, *T;
  uint32_t s_C, s_Co, s_A, s_E, s_Ti, s_T;
};
RsPhase phase_x(uint32_t H, uint32_t k, const Rows& r) {
  return {{r.C, r.Co, r.A},       {H * k, H * k, k}, {r.s_C, r.s_Co, r.s_A}, {lab('C'), lab('C', '\''), lab('A')},
          {1, 2, 1}, lab('x'), 1};
}
RsPhase phase_y(uint32_t k, const Rows& r) {
  return {{r.E, nullptr, nullptr}, {k, 0, 0}, {r.s_E, 0, 0}, {lab('E'), 0, 0}, {1, 0, 0}, lab('y'), 1};
}
RsPhase phase_c(uint32_t H, uint32_t k, const Rows& r) {
  return {{r.Ti, r.T, nullptr}, {k, H, 0}, {r.s_Ti, r.s_T, 0}, {lab('T', 'i'), lab('T'), 0}, {2, 1, 0}, lab('c'), 1};
}

// ---------------------------------------------------------------- the prover

// One launch sequence for P proofs, then the inner proofs through the circuit
// prover's host-input seam.  Secrets live in "rs_secret" (prove_wipe) and in
// recorded spans of the pinned arena; the caller wipes.
int prove_chunk(bpp_ctx* ctx, const bpp_gens* G, const RsKind& kd, const perm::Circuit& C, uint32_t k, uint32_t P,
                const uint8_t* key, const uint8_t* cards_in, const uint32_t* perms, const uint8_t* blinds,
                const uint8_t* seeds32, const uint8_t* label, size_t llen, uint8_t* cards_out, uint8_t* proofs_out) {
  const uint32_t H = kd.H;
  const size_t n = (size_t)P * k, S = 32, n_in = kd.keys + H * n;  // n_in: the key | cards_in, one run of encodings
  // public device arrays, one workspace: offsets in bytes
  const size_t o_in = 0, o_cout = o_in + n_in * S, o_A = o_cout + H * n * S, o_E = o_A + n * S, o_Ti = o_E + n * S,
               o_T = o_Ti + n * S, o_resp = o_T + H * P * S, o_u = o_resp + (size_t)P * (2 * k + 1) * S,
               o_ch = o_u + n * S, o_st = o_ch + 3 * (size_t)P * S, pub_bytes = o_st + (size_t)P * MERLIN_DEV_STATE_BYTES;
  // secret device arrays, one workspace: the draws, pi, 0, b, d, delta; r times the fixed base [n]; with a key
  // r K [n] | t_R K [P]; t times the output cards' rows [Hn] | t_R times the fixed base [P]; the staged inputs
  const size_t o_dr = 0, o_piv = o_dr + (5 * n + P) * S, o_zero = o_piv + n * S, o_b = o_zero + n * S,
               o_d = o_b + n * S, o_dl = o_d + n * S, o_rB = o_dl + n * S, o_rK = o_rB + n * P3_BYTES,
               o_prod = o_rK + kd.keys * (n + P) * P3_BYTES, o_tRB = o_prod + H * n * P3_BYTES,
               o_sin = o_tRB + P * P3_BYTES, in_bytes = n * 4 + (size_t)P * 32 + (blinds ? n * S : 0),
               sec_bytes = o_sin + in_bytes;
  uint8_t *pub = nullptr, *sec = nullptr;
  void *d_tin = nullptr, *d_tout = nullptr, *d_bad = nullptr, *d_res = nullptr;
  BPP_TRY(ctx_ws(ctx, "rs_pub", pub_bytes, (void**)&pub));
  BPP_TRY(ctx_ws(ctx, "rs_secret", sec_bytes, (void**)&sec));
  BPP_TRY(ctx_ws(ctx, "rs_tin", n_in * MSM_NIELS_WORDS * 4, &d_tin));
  BPP_TRY(ctx_ws(ctx, "rs_tout", H * n * MSM_NIELS_WORDS * 4, &d_tout));
  BPP_TRY(ctx_ws(ctx, "rs_bad", 8, &d_bad));
  BPP_TRY(ctx_ws(ctx, "rs_ts_res", (size_t)H * P * P3_BYTES, &d_res));
  auto W = [](uint8_t* base, size_t off) { return (uint32_t*)(base + off); };
  uint32_t *d_in = W(pub, o_in), *d_cin = d_in + 8 * kd.keys, *d_cout = W(pub, o_cout), *d_A = W(pub, o_A),
           *d_E = W(pub, o_E), *d_Ti = W(pub, o_Ti), *d_T = W(pub, o_T), *d_resp = W(pub, o_resp), *d_u = W(pub, o_u),
           *d_x = W(pub, o_ch), *d_y = d_x + 8 * (size_t)P, *d_c = d_y + 8 * (size_t)P;
  uint8_t* d_st = pub + o_st;
  uint32_t *d_dr = W(sec, o_dr), *d_piv = W(sec, o_piv), *d_zero = W(sec, o_zero), *d_b = W(sec, o_b),
           *d_d = W(sec, o_d), *d_dl = W(sec, o_dl), *d_rB = W(sec, o_rB), *d_rK = W(sec, o_rK),
           *d_prod = W(sec, o_prod), *d_tRB = W(sec, o_tRB);
  // (blinds | seeds | perms: the scalars first, at 32-byte offsets)
  const size_t bl_bytes = blinds ? n * S : 0;
  uint32_t *d_blinds = blinds ? W(sec, o_sin) : nullptr, *d_seeds = W(sec, o_sin + bl_bytes), *d_perms = d_seeds + 8 * (size_t)P;
  uint32_t *d_r = d_dr, *d_alpha = d_dr + 8 * n, *d_beta = d_dr + 16 * n, *d_t = d_dr + 24 * n, *d_w = d_dr + 32 * n,
           *d_tR = d_dr + 40 * n;
  const uint32_t* d_tK = (const uint32_t*)d_tin;                         // the key's table row, where there is one
  const uint32_t* d_tcards = d_tK + kd.keys * MSM_NIELS_WORDS;           // the cards' rows, H per card

  // the key and the cards first: uploaded, decoded and checked before any secret is staged or any other kernel runs
  {
    uint8_t* stage = nullptr;
    BPP_TRY(ctx_h2d_stage(ctx, n_in * S, &stage));
    memcpy(stage, key, kd.keys * S);
    ctx_stage_copy(stage + kd.keys * S, cards_in, H * n * S);
    BPP_TRY(ctx_h2d_staged(ctx, d_in, stage, n_in * S));
  }
  BPP_TRY(rs_decompress_dev(ctx, d_in, n_in, (uint32_t*)d_tin, d_bad));
  {
    unsigned long long bad = ~0ull;
    BPP_TRY(ctx_d2h(ctx, &bad, d_bad, 8));
    if (bad < kd.keys) return key_undecodable(ctx, kd);
    if (bad != ~0ull) {
      const size_t j = bad - kd.keys, deck = (size_t)H * k;  // (among the cards' points)
      ctx->err = std::string(kd.name) + " " + std::to_string(j / deck) + ": " + point_name(kd, k, j % deck) + " does not decode";
      return BPP_ERR_DECOMPRESS;
    }
  }
  // blinds | seeds | perms through one recorded span
  {
    uint8_t* stage = nullptr;
    BPP_TRY(ctx_h2d_stage(ctx, in_bytes, &stage));
    ctx_secret_span(ctx, stage, in_bytes);
    if (blinds) memcpy(stage, blinds, bl_bytes);
    memcpy(stage + bl_bytes, seeds32, (size_t)P * 32);
    memcpy(stage + bl_bytes + (size_t)P * 32, perms, n * 4);
    BPP_TRY(ctx_h2d_staged(ctx, sec + o_sin, stage, in_bytes));
  }
  uint32_t init[52], *h_init = nullptr;
  init_state(kd, k, key, label, llen, init);
  BPP_TRY(ctx_zc_in(ctx, "rs_init", init, sizeof init, &h_init));

  const Rows rows = {d_cin, d_cout, d_A, d_E, d_Ti, d_T, 8 * H * k, 8 * H * k, 8 * k, 8 * k, 8 * k, 8 * H};
  BPP_TRY(rs_draws_dev(ctx, P, k, d_seeds, d_blinds, d_perms, d_dr, d_piv, d_zero));
  // r_i times the fixed base by the walk; with a key r_i K and t_R K by double-and-add-always; then the output
  // cards and their table
  BPP_TRY(fixed_base_dev(ctx, G, kd, d_r, d_zero, n, d_rB));
  if (kd.keys) BPP_TRY(mrs_key_mul_dev(ctx, P, k, d_dr, d_tK, d_rK));
  BPP_TRY(rs_outputs_dev(ctx, H, P, k, d_tcards, d_perms, d_rB, d_rK, d_cout, (uint32_t*)d_tout));
  BPP_TRY(pedersen_dev(ctx, G, d_piv, d_alpha, n, d_A, nullptr, k));  // (pi(i) < k, public)
  BPP_TRY(rs_transcript_dev(ctx, P, h_init, d_st, phase_x(H, k, rows), d_x));
  BPP_TRY(rs_exponents_dev(ctx, P, k, d_x, d_perms, d_b));
  BPP_TRY(pedersen_dev(ctx, G, d_b, d_beta, n, d_E, nullptr));
  BPP_TRY(rs_transcript_dev(ctx, P, nullptr, d_st, phase_y(k, rows), d_y));
  BPP_TRY(pedersen_dev(ctx, G, d_t, d_w, n, d_Ti, nullptr));
  // the H sums with no scalar-derived scratch: t_R times the fixed base by the walk, t_i times the output cards'
  // points by double-and-add-always (the bucket engine would sort the secret nonces' digits into workspaces
  // nothing wipes)
  BPP_TRY(fixed_base_dev(ctx, G, kd, d_tR, d_zero, P, d_tRB));
  BPP_TRY(rs_tsum_dev(ctx, H, P, k, d_dr, (const uint32_t*)d_tout, d_prod, d_tRB, d_rK + n * P3_WORDS, (uint32_t*)d_res));
  BPP_TRY(points_compress_p3_dev(ctx, (const uint32_t*)d_res, (size_t)H * P, (uint8_t*)d_T));
  BPP_TRY(rs_transcript_dev(ctx, P, nullptr, d_st, phase_c(H, k, rows), d_c));
  BPP_TRY(rs_responses_dev(ctx, P, k, d_dr, d_perms, d_b, d_x, d_y, d_c, d_resp, d_d, d_dl, d_u));

  // back to the host: what the proofs are made of, and d | delta for the inner
  // prover's host-input seam (through a recorded span; the copies are wiped below)
  const size_t out_bytes = o_ch - o_cout;  // cout .. u
  std::vector<uint8_t> h_pub(out_bytes), h_sec(2 * n * S);
  {
    uint8_t* stage = nullptr;
    BPP_TRY(ctx_h2d_stage(ctx, 2 * n * S + out_bytes, &stage));
    ctx_secret_span(ctx, stage, 2 * n * S);
    BPP_HIP(hipMemcpyAsync(stage, d_d, 2 * n * S, hipMemcpyDeviceToHost, ctx->stream));  // (d and delta are adjacent)
    BPP_HIP(hipMemcpyAsync(stage + 2 * n * S, pub + o_cout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    BPP_TRY(ctx_sync(ctx));
    memcpy(h_sec.data(), stage, 2 * n * S);
    memcpy(h_pub.data(), stage + 2 * n * S, out_bytes);
    memset(stage, 0, 2 * n * S);
  }
  auto wipe_host = [&] { memset(h_sec.data(), 0, h_sec.size()); };
  const uint8_t *h_cout = h_pub.data(), *h_A = h_pub.data() + (o_A - o_cout), *h_T = h_pub.data() + (o_T - o_cout),
                *h_resp = h_pub.data() + (o_resp - o_cout), *h_u = h_pub.data() + (o_u - o_cout);

  // the inner proofs: shuffle_of_public(k) with v = d, gammas = delta, pub = u
  const size_t il = perm::proof_len(C), hd = 3 * (size_t)k + H, pl = (hd + 2 * k + 2) * S + il;  // hd: A E Ti and the sums
  std::vector<uint8_t> iseed((size_t)P * 32), iproofs((size_t)P * il), iV((size_t)P * (k + 1) * 32);
  for (uint32_t p = 0; p < P; ++p) {
    merlin::Shake256 sh;
    sh.update((const uint8_t*)"bpperm-reshuffle-inner", 22);
    sh.update(seeds32 + 32 * (size_t)p, 32);
    sh.read(iseed.data() + 32 * (size_t)p, 32);
  }
  ProveInputs in;
  in.values = {h_sec.data(), k};
  in.gammas = {h_sec.data() + n * S, k};
  in.pub = {h_u, k};
  const int rc = prove_batch_entropy(ctx, G, C, P, iseed.data(), label, llen, iproofs.data(), iV.data(), &in);
  wipe_host();
  memset(iseed.data(), 0, iseed.size());
  BPP_TRY(rc);

  memcpy(cards_out, h_cout, H * n * S);
  par::for_each(P, [&](size_t p) {
    uint8_t* o = proofs_out + p * pl;
    for (int part = 0; part < 3; ++part)  // A | E | Ti
      memcpy(o + part * k * S, h_A + (part * n + p * k) * S, k * S);
    memcpy(o + 3 * k * S, h_T + H * p * S, H * S);  // T_S, or T_U | T_W
    memcpy(o + hd * S, h_resp + p * (2 * k + 1) * S, (2 * k + 1) * S);
    memcpy(o + (hd + 2 * k + 1) * S, iV.data() + (p * (k + 1) + k) * S, S);
    memcpy(o + (hd + 2 * k + 2) * S, iproofs.data() + p * il, il);
  });
  return BPP_OK;
}

// The prove entry's body.  key: kd.keys encodings (kNoKey: none).
int prove_call(const RsKind& kd, bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* key,
               const uint8_t* cards_in, const uint32_t* perms, const uint8_t* blinds, const uint8_t* seeds32,
               const uint8_t* label, size_t llen, uint8_t* cards_out, uint8_t* proofs_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (((!key || !cards_in || !perms || !cards_out || !proofs_out) && count) || (!label && llen) || k < 2 ||
        k > (1u << 20))
      return BPP_ERR_ARG;
    // the witness is checked before any device work and before any output byte
    // is written: every perm a bijection on [0, k), every supplied blind a
    // canonical scalar (neither needs ctx or g)
    std::vector<int> bad(count, BPP_OK);
    check_perms(perms, count, k, bad);
    check_canonical(blinds, k, count, bad);
    if (const size_t p = first_bad(bad, BPP_ERR_ARG); p != SIZE_MAX) {
      if (ctx) ctx->err = std::string(kd.name) + " " + std::to_string(p) + ": perm is not a bijection on [0, k)";
      return BPP_ERR_ARG;
    }
    if (const size_t p = first_bad(bad); p != SIZE_MAX) {
      if (ctx) ctx->err = std::string(kd.name) + " " + std::to_string(p) + ": non-canonical blind";
      return bad[p];
    }
    BPP_TRY(rs_k_check(ctx, k));
    if (!ctx || !G) return BPP_ERR_ARG;
    if (!count) return BPP_OK;
    const perm::Circuit* C = rs_circuit(k);
    if (!C) return BPP_ERR_DEVICE;
    BPP_TRY(gens_cover(ctx, G, C->n_p));
    BPP_HIP(hipSetDevice(ctx->device));
    std::vector<uint8_t> ent;
    if (!seeds32) {
      ent.resize(32 * count);
      if (!perm::os_entropy(ent.data(), ent.size())) return no_entropy(ctx);
      seeds32 = ent.data();
    }
    // every chunk is proved into the caller's buffers only once it is whole; a
    // failed call leaves no card or proof of a chunk it did not finish
    const size_t pl = rs_proof_len(kd, k), cb = 32 * (size_t)kd.H * k;  // cb: the bytes of a proof's cards
    const uint32_t per = chunk_of(kd, k, count);
    int rc = BPP_OK;
    for (size_t p0 = 0; p0 < count && rc == BPP_OK; p0 += per) {
      const uint32_t P = (uint32_t)std::min<size_t>(per, count - p0);
      rc = prove_chunk(ctx, G, kd, *C, k, P, key, cards_in + p0 * cb, perms + p0 * k,
                       blinds ? blinds + p0 * k * 32 : nullptr, seeds32 + p0 * 32, label, llen, cards_out + p0 * cb,
                       proofs_out + p0 * pl);
    }
    if (!ent.empty()) memset(ent.data(), 0, ent.size());
    const int wrc = prove_wipe(ctx);
    return rc ? rc : wrc;
  });
}

// --------------------------------------------------------------- the verifiers

struct VerifyArgs {
  const RsKind& kd;
  bpp_ctx* ctx;
  const bpp_gens* G;
  uint32_t k;
  const uint8_t *key, *label;  // key: kd.keys encodings (kNoKey: none)
  size_t llen, count;
  const uint8_t *cards_in, *cards_out, *proofs;
  uint8_t* ok_out;  // null: one verdict for the call
};

// P proofs, the call's proofs [first, first + P): BPP_OK, BPP_ERR_VERIFY (ok:
// null, or the proofs' verdicts), or an error.
int verify_chunk(const VerifyArgs& a, const perm::Circuit& C, const uint8_t seed[32], size_t first, uint32_t P,
                 uint8_t* ok) {
  bpp_ctx* ctx = a.ctx;
  const bpp_gens* G = a.G;
  const RsKind& kd = a.kd;
  const uint32_t H = kd.H, k = a.k, npt = rs_points(H, k), nsc = 2 * k + 1, terms = rs_terms(H, k);
  const size_t n = (size_t)P * k, S = 32, il = perm::proof_len(C), cb = S * H * k, hd = 3 * (size_t)k + H,
               pl = (hd + nsc + 1) * S + il;  // cb: the bytes of a proof's cards; hd: its A E Ti and sums
  const uint32_t n0 = (uint32_t)(2 * G->n + 2);  // the first table point behind the generators': the key's, or the first proof's
  const size_t NP = (size_t)P * npt + kd.keys, TP = (size_t)terms + H + 1, T1 = (size_t)P * terms + H + 1;
  // one workspace, offsets in bytes: enc the key | [P][npt] | resp [P][2k+1] | D enc | u | x y c rho | states
  const size_t o_enc = 0, o_resp = o_enc + NP * S, o_D = o_resp + (size_t)P * nsc * S, o_u = o_D + n * S,
               o_ch = o_u + n * S, o_st = o_ch + 4 * (size_t)P * S, bytes = o_st + (size_t)P * MERLIN_DEV_STATE_BYTES;
  uint8_t* base = nullptr;
  void *d_tbl = nullptr, *d_bad = nullptr, *d_Dp3 = nullptr, *d_s = nullptr, *d_idx = nullptr, *d_off = nullptr,
       *d_scr = nullptr;
  BPP_TRY(ctx_ws(ctx, "rs_v", bytes, (void**)&base));
  BPP_TRY(ctx_ws(ctx, "rs_v_tbl", NP * MSM_NIELS_WORDS * 4, &d_tbl));
  BPP_TRY(ctx_ws(ctx, "rs_bad", 8, &d_bad));
  BPP_TRY(ctx_ws(ctx, "rs_v_Dp3", n * P3_BYTES, &d_Dp3));
  BPP_TRY(ctx_ws(ctx, "rs_v_s", ((size_t)P * TP + H + 1) * S, &d_s));
  BPP_TRY(ctx_ws(ctx, "rs_v_idx", ((size_t)P * TP + H + 1) * 4, &d_idx));
  BPP_TRY(ctx_ws(ctx, "rs_v_off", ((size_t)P + 1) * 4, &d_off));
  BPP_TRY(ctx_ws(ctx, "rs_v_scr", (2 * n + (H + 1) * (size_t)P) * S, &d_scr));
  auto W = [&](size_t off) { return (uint32_t*)(base + off); };
  uint32_t *d_enc = W(o_enc), *d_resp = W(o_resp), *d_D = W(o_D), *d_u = W(o_u), *d_x = W(o_ch),
           *d_y = d_x + 8 * (size_t)P, *d_c = d_y + 8 * (size_t)P, *d_rho = d_c + 8 * (size_t)P;
  uint8_t* d_st = base + o_st;
  {
    // the key, then per proof: the cards in | the cards out | A E Ti and the sums (the proof's first hd fields);
    // then z | om | z_R
    uint8_t* stage = nullptr;
    BPP_TRY(ctx_h2d_stage(ctx, o_D, &stage));
    memcpy(stage, a.key, kd.keys * S);
    par::for_each(P, [&](size_t p) {
      const size_t q = first + p;
      uint8_t* e = stage + (kd.keys + p * npt) * S;
      memcpy(e, a.cards_in + q * cb, cb);
      memcpy(e + cb, a.cards_out + q * cb, cb);
      memcpy(e + 2 * cb, a.proofs + q * pl, hd * S);
      memcpy(stage + o_resp + p * nsc * S, a.proofs + q * pl + hd * S, nsc * S);
    });
    BPP_TRY(ctx_h2d_staged(ctx, base, stage, o_D));
  }
  uint32_t init[52], *h_init = nullptr, *h_seed = nullptr;
  init_state(kd, k, a.key, a.label, a.llen, init);
  BPP_TRY(ctx_zc_in(ctx, "rs_init", init, sizeof init, &h_init));
  BPP_TRY(ctx_zc_in(ctx, "rs_seed", seed, 32, &h_seed));
  const uint32_t st = 8 * npt, cw = 8 * H * k;  // words between two proofs' rows, and of a proof's cards
  const uint32_t* e0 = d_enc + 8 * kd.keys;    // the first proof's row
  const Rows rows = {e0, e0 + cw, e0 + 2 * cw, e0 + 2 * cw + 8 * k, e0 + 2 * cw + 16 * k, e0 + 2 * cw + 24 * k,
                     st, st, st, st, st, st};
  BPP_TRY(rs_decompress_dev(ctx, d_enc, NP, (uint32_t*)d_tbl, d_bad));
  // A point that does not decode, looked for before anything else runs: the
  // key refuses the call; any other refuses the call too, or in _each fails its
  // proof alone -- the scan goes on behind that proof until it finds no more
  // (the table holds the identity in a bad point's place, so the other proofs'
  // checks run as they would alone).
  std::vector<uint8_t> undec(P, 0);
  {
    unsigned long long bad = ~0ull;
    BPP_TRY(ctx_d2h(ctx, &bad, d_bad, 8));
    if (bad < kd.keys) return key_undecodable(ctx, kd);
    for (size_t from = 0; bad != ~0ull;) {
      const size_t at = from + bad - kd.keys, q = at / npt, j = at % npt;  // (among the proofs' points)
      if (!ok) {
        ctx->err = std::string(kd.name) + " " + std::to_string(first + q) + ": " + point_name(kd, k, j) + " does not decode";
        return BPP_ERR_DECOMPRESS;
      }
      undec[q] = 1;
      from = kd.keys + (q + 1) * npt;
      if (from >= NP) break;
      BPP_TRY(rs_decompress_dev(ctx, d_enc + 8 * from, NP - from, (uint32_t*)d_tbl + from * MSM_NIELS_WORDS, d_bad));
      BPP_TRY(ctx_d2h(ctx, &bad, d_bad, 8));
    }
  }
  const uint32_t* d_rows = (const uint32_t*)d_tbl + kd.keys * MSM_NIELS_WORDS;  // the first proof's table row
  BPP_TRY(rs_transcript_dev(ctx, P, h_init, d_st, phase_x(H, k, rows), d_x));
  BPP_TRY(rs_transcript_dev(ctx, P, nullptr, d_st, phase_y(k, rows), d_y));
  BPP_TRY(rs_transcript_dev(ctx, P, nullptr, d_st, phase_c(H, k, rows), d_c));
  BPP_TRY(rs_D_dev(ctx, H, P, k, d_rows, d_y, (uint32_t*)d_Dp3));
  BPP_TRY(points_compress_p3_dev(ctx, (const uint32_t*)d_Dp3, n, (uint8_t*)d_D));
  BPP_TRY(rs_weights_dev(ctx, P, h_seed, first, d_c, d_rho));
  // checks (i) and (ii) of every proof in one MSM: `terms` points per proof, the H + 1 shared bases once
  BPP_TRY(rs_sigma_terms_dev(ctx, H, P, k, false, d_resp, d_x, d_y, d_c, d_rho, n0, G->bidx(), G->bbidx(),
                             (uint32_t*)d_s, (uint32_t*)d_idx, (uint32_t*)d_off, d_u, (uint32_t*)d_scr));
  h25519::ge res;
  {
    const uint32_t c = msm_choose_c((double)T1);
    BPP_TRY(msm_single_dev(ctx, (const uint32_t*)d_s, (const uint32_t*)d_idx, G->d_tbl, T1, c, 0, (254 + c - 1) / c,
                           &res, (const uint32_t*)d_tbl, n0));
  }
  const bool sigma_ok = is_identity(res);

  std::vector<uint8_t> h_Du(2 * n * S), ok_s(P, 1);
  BPP_TRY(ctx_d2h(ctx, h_Du.data(), d_D, 2 * n * S));  // (D and u are adjacent; synchronises)
  if (!sigma_ok && ok) {
    // each proof's own checks (i) and (ii): P MSMs of TP terms over the same
    // table and weights, in passes as verify_each_dev's
    const uint32_t c = msm_choose_c((double)TP);
    const size_t per = std::min<size_t>(P, std::max<size_t>(1, each_pass_proofs(TP, c)));
    void *d_res = nullptr, *d_renc = nullptr;
    BPP_TRY(ctx_ws(ctx, "rs_v_res", (size_t)P * P3_BYTES, &d_res));
    BPP_TRY(ctx_ws(ctx, "rs_v_renc", (size_t)P * 32, &d_renc));
    BPP_TRY(rs_sigma_terms_dev(ctx, H, P, k, true, d_resp, d_x, d_y, d_c, d_rho, n0, G->bidx(), G->bbidx(),
                               (uint32_t*)d_s, (uint32_t*)d_idx, (uint32_t*)d_off, d_u, (uint32_t*)d_scr));
    for (size_t p0 = 0; p0 < P; p0 += per) {  // (off[j] = j TP serves every pass)
      const uint32_t M = (uint32_t)std::min(per, P - p0);
      BPP_TRY(msm_multi_dev(ctx, (const uint32_t*)d_s + 8 * p0 * TP, (const uint32_t*)d_idx + p0 * TP,
                            (const uint32_t*)d_off, M, (uint32_t)(M * TP), c, G->d_tbl, (const uint32_t*)d_tbl, n0,
                            (uint32_t*)d_res + p0 * P3_WORDS));
    }
    BPP_TRY(points_compress_p3_dev(ctx, (const uint32_t*)d_res, P, (uint8_t*)d_renc));
    std::vector<uint8_t> renc((size_t)P * 32);
    BPP_TRY(ctx_d2h(ctx, renc.data(), d_renc, renc.size()));
    static const uint8_t zero[32] = {0};  // (the results come back encoded)
    for (uint32_t p = 0; p < P; ++p) ok_s[p] = memcmp(renc.data() + 32 * (size_t)p, zero, 32) == 0;
  }
  if (!sigma_ok && !ok) return BPP_ERR_VERIFY;

  // check (iii): the circuit verifier on V = (D_0..D_{k-1}, V_k), pub = u
  std::vector<uint8_t> iV((size_t)P * (k + 1) * S), iproofs((size_t)P * il);
  par::for_each(P, [&](size_t p) {
    const uint8_t* pf = a.proofs + (first + p) * pl;
    memcpy(iV.data() + p * (k + 1) * S, h_Du.data() + p * k * S, k * S);
    memcpy(iV.data() + (p * (k + 1) + k) * S, pf + (hd + nsc) * S, S);
    memcpy(iproofs.data() + p * il, pf + (hd + nsc + 1) * S, il);
  });
  const uint8_t* h_u = h_Du.data() + n * S;
  const int rc = verify_batch(ctx, G, C, a.label, a.llen, P, iproofs.data(), iV.data(), ok, h_u);
  if (!ok || (rc != BPP_OK && rc != BPP_ERR_VERIFY)) return rc;
  bool all = true;
  for (uint32_t p = 0; p < P; ++p) all &= (ok[p] = ok[p] && ok_s[p] && !undec[p]) != 0;
  return all ? BPP_OK : BPP_ERR_VERIFY;
}

int verify_call(const VerifyArgs& a, bool each, bool len_ok) {
  bpp_ctx* const ctx = a.ctx;
  const RsKind& kd = a.kd;
  uint8_t* const ok_out = each ? a.ok_out : nullptr;
  ok_clear(ok_out, a.count);
  const int rc = bpp_guard(ctx, [&]() -> int {
    // in the prover's order: the arrays and k, then the proofs' own scalars
    // (neither needs ctx or g), then the null handles
    if (((!a.key || !a.cards_in || !a.cards_out || !a.proofs || (each && !a.ok_out)) && a.count) ||
        (!a.label && a.llen))
      return BPP_ERR_ARG;
    BPP_TRY(rs_k_check(ctx, a.k));
    const uint32_t k = a.k;
    if (a.count && len_ok) {
      // z, om, z_R of every proof are canonical scalars
      const size_t pl = rs_proof_len(kd, k);
      std::vector<int> bad(a.count, BPP_OK);
      par::for_each(a.count, [&](size_t p) {
        Sc t;
        const uint8_t* s = a.proofs + p * pl + 32 * (3 * (size_t)k + kd.H);
        for (uint32_t i = 0; i < 2 * k + 1; ++i)
          if (!hsc::from_canonical(t, s + 32 * (size_t)i)) bad[p] = BPP_ERR_NONCANONICAL;
      });
      if (const size_t p = first_bad(bad); p != SIZE_MAX) {
        if (ctx) ctx->err = std::string(kd.name) + " " + std::to_string(p) + ": a response scalar is not canonical";
        return BPP_ERR_NONCANONICAL;
      }
    }
    if (!ctx || !a.G) return BPP_ERR_ARG;
    if (!a.count) return BPP_OK;
    if (!len_ok) return BPP_ERR_VERIFY;
    const perm::Circuit* C = rs_circuit(k);
    if (!C) return BPP_ERR_DEVICE;
    BPP_TRY(gens_cover(ctx, a.G, C->n_p));
    BPP_HIP(hipSetDevice(ctx->device));
    uint8_t seed[32];
    BPP_TRY(verify_seed_or_err(ctx, seed));
    const uint32_t per = chunk_of(kd, k, a.count);
    bool failed = false;  // (each) some chunk's proof
    for (size_t p0 = 0; p0 < a.count; p0 += per) {
      const uint32_t P = (uint32_t)std::min<size_t>(per, a.count - p0);
      const int crc = verify_chunk(a, *C, seed, p0, P, each ? a.ok_out + p0 : nullptr);
      if (crc == BPP_ERR_VERIFY && each)
        failed = true;
      else if (crc != BPP_OK)
        return crc;
    }
    // (a chunk answers BPP_ERR_VERIFY only after clearing one of its ok bytes,
    // so each_report's "no single proof failed" branch is not reachable here)
    return failed ? each_report(ctx, a.ok_out, a.count) : BPP_OK;
  });
  return ok_settle(rc, ok_out, a.count);
}

}  // namespace

extern "C" {

size_t bpp_reshuffle_proof_len(uint32_t k) { return rs_proof_len(kRsBlind, k); }
size_t bpp_masked_reshuffle_proof_len(uint32_t k) { return rs_proof_len(kRsMasked, k); }

int bpp_reshuffle_prove_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* cards_in,
                              const uint32_t* perms, const uint8_t* blinds, const uint8_t* seeds32, const uint8_t* label,
                              size_t llen, uint8_t* cards_out, uint8_t* proofs_out) {
  return prove_call(kRsBlind, ctx, G, k, count, kNoKey, cards_in, perms, blinds, seeds32, label, llen, cards_out,
                    proofs_out);
}

int bpp_masked_reshuffle_prove_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* key,
                                     const uint8_t* cards_in, const uint32_t* perms, const uint8_t* blinds,
                                     const uint8_t* seeds32, const uint8_t* label, size_t llen, uint8_t* cards_out,
                                     uint8_t* proofs_out) {
  return prove_call(kRsMasked, ctx, G, k, count, key, cards_in, perms, blinds, seeds32, label, llen, cards_out,
                    proofs_out);
}

int bpp_reshuffle_verify(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, const uint8_t* label, size_t llen,
                         const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proof, size_t proof_len) {
  return verify_call({kRsBlind, ctx, G, k, kNoKey, label, llen, 1, cards_in, cards_out, proof, nullptr}, false,
                     proof_len == rs_proof_len(kRsBlind, k));
}

int bpp_masked_reshuffle_verify(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, const uint8_t* key, const uint8_t* label,
                                size_t llen, const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proof,
                                size_t proof_len) {
  return verify_call({kRsMasked, ctx, G, k, key, label, llen, 1, cards_in, cards_out, proof, nullptr}, false,
                     proof_len == rs_proof_len(kRsMasked, k));
}

int bpp_reshuffle_verify_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* label,
                               size_t llen, const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proofs) {
  return verify_call({kRsBlind, ctx, G, k, kNoKey, label, llen, count, cards_in, cards_out, proofs, nullptr}, false, true);
}

int bpp_masked_reshuffle_verify_batch(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* key,
                                      const uint8_t* label, size_t llen, const uint8_t* cards_in,
                                      const uint8_t* cards_out, const uint8_t* proofs) {
  return verify_call({kRsMasked, ctx, G, k, key, label, llen, count, cards_in, cards_out, proofs, nullptr}, false, true);
}

int bpp_reshuffle_verify_batch_each(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count, const uint8_t* label,
                                    size_t llen, const uint8_t* cards_in, const uint8_t* cards_out,
                                    const uint8_t* proofs, uint8_t* ok_out) {
  return verify_call({kRsBlind, ctx, G, k, kNoKey, label, llen, count, cards_in, cards_out, proofs, ok_out}, true, true);
}

int bpp_masked_reshuffle_verify_batch_each(bpp_ctx* ctx, const bpp_gens* G, uint32_t k, size_t count,
                                           const uint8_t* key, const uint8_t* label, size_t llen,
                                           const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proofs,
                                           uint8_t* ok_out) {
  return verify_call({kRsMasked, ctx, G, k, key, label, llen, count, cards_in, cards_out, proofs, ok_out}, true, true);
}

}  // extern "C"
