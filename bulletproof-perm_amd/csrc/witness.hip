// The prover's inputs and the built-in circuits' witnesses on the GPU: the
// blinding draws (k_draws), the V commitments' inputs from a caller's values
// (k_v_inputs), and the chain witnesses of the two-half shuffle and the deck
// circuit (k_witness, k_witness_cards, k_witness_deck).  Declared in witness.h;
// a caller-defined circuit's witness is circuit_witness.hip.
#include <cstring>

#include "ctx.h"
#include "witness.h"
#include "keccak_dev.cuh"
#include "sc25519.cuh"

// The prover's wide random draws reduced on the device.  stream = [P][len]
// bytes of each proof's SHAKE256 stream (host/perm.h draw order: pi's u64s,
// gamma[m], alpha beta rho, s_L[n_p], s_R[n_p], tau[5]); the host parses pi,
// alpha, beta, rho and tau itself and never needs gamma, s_L, s_R: gamma goes
// to [P][m] (V commitments, tau_x), s_L / s_R straight into their slots of the
// A_I/A_O/S scalar array ([P][per], per = 3 + 5 n_p: s_L at 3 + 3 n_p).
// The blinding draws (perm.h draw_scalar) of P proofs, one thread per draw:
// draw j's sponge block is the proof's template (tmpl [P][7] u64, host-built:
// domain || seed with the 0x1F pad byte after the index) plus le32 j at byte
// jo and the 0x80 that closes the 136-byte rate; one Keccak-f yields the 64
// bytes that from_wide reduces.  gamma -> [P][m]; alpha, beta, rho, s_L, s_R
// -> their slots of the A_I/A_O/S scalar array ([alpha, a_L, a_R, beta, a_O,
// rho, s_L, s_R], per words x 8 a proof); the host draws tau itself.
// With v (non-null) it also writes the V commitments' inputs (gamma_j's
// thread, j <= 2k): v[p][i] = i + 1 (i < k) or pi_p[i - k] + 1 (k <= i < 2k),
// g[p][i] = gamma_i, gx_half[p] = gamma_2k / 2 (V_2k is committed with halved
// scalars and encoded as 2 (C / 2) on the host) -- no launch of its own.
__global__ void __launch_bounds__(256) k_draws(uint32_t P, uint32_t m, uint32_t n_p, uint32_t per, uint32_t jo,
                                              const uint64_t* __restrict__ tmpl, uint32_t* __restrict__ gamma,
                                              uint32_t* __restrict__ sc_out, uint32_t k,
                                              const uint32_t* __restrict__ pi, uint32_t* __restrict__ v,
                                              uint32_t* __restrict__ g, uint32_t* __restrict__ gx_half) {
  const uint32_t nw = m + 3 + 2 * n_p;  // gamma[m], alpha, beta, rho, s_L[n_p], s_R[n_p]
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * nw) return;
  const uint32_t p = (uint32_t)(t / nw), j = (uint32_t)(t % nw);
  uint64_t a[25];
  _Pragma("unroll") for (int i = 0; i < 25; ++i) a[i] = i < 7 ? tmpl[7 * (size_t)p + i] : 0ull;
  a[16] ^= 0x8000000000000000ull;
  const uint32_t li = jo >> 3, sh = 8 * (jo & 7);
  _Pragma("unroll") for (uint32_t i = 0; i < 7; ++i) {  // (static indices: no scratch)
    if (i == li) a[i] ^= (uint64_t)j << sh;
    if (i == li + 1 && sh > 32) a[i] ^= (uint64_t)j >> (64 - sh);
  }
  keccak_f1600_dev(a);
  uint32_t w[16];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) {
    w[2 * i] = (uint32_t)a[i];
    w[2 * i + 1] = (uint32_t)(a[i] >> 32);
  }
  const sc x = sc_from_wide_w(w);
  if (j < m) {
    sc_store(gamma + 8 * ((size_t)p * m + j), x);
    if (v) {
      if (j == 2 * k) {
        sc_store(gx_half + 8 * (size_t)p, sc_half(x));
      } else if (j < 2 * k) {
        sc vv = sc_zero();
        vv.v[0] = j < k ? j + 1 : pi[(size_t)p * k + (j - k)] + 1;
        sc_store(v + 8 * ((size_t)p * 2 * k + j), vv);
        sc_store(g + 8 * ((size_t)p * 2 * k + j), x);
      }
    }
    return;
  }
  const uint32_t q = j - m;
  const uint32_t pos = q == 0 ? 0u : q == 1 ? 1 + 2 * n_p : q == 2 ? 2 + 3 * n_p : 3 + 3 * n_p + (q - 3);
  sc_store(sc_out + 8 * ((size_t)p * per + pos), x);
}

int draws_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint64_t* d_tmpl, uint32_t seed_len,
              uint32_t per, uint32_t* d_gamma, uint32_t* d_sc, const uint32_t* d_pi, uint32_t* d_v, uint32_t* d_g,
              uint32_t* d_gx_half) {
  if (!P) return BPP_OK;
  if (seed_len > 32) {
    ctx->err = "draws_dev: seed longer than 32 bytes";
    return BPP_ERR_ARG;
  }
  const size_t nt = (size_t)P * (C.m + 3 + 2 * C.n_p);
  hipLaunchKernelGGL(k_draws, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, ctx->stream, P, C.m, C.n_p, per,
                     (uint32_t)(BPP_DRAW_DOMAIN_LEN + seed_len), d_tmpl, d_gamma, d_sc, C.k, d_pi, d_v, d_g,
                     d_gx_half);
  return ctx_check_launch(ctx, "k_draws");
}

void draw_template(const perm::Seed& seed, uint64_t tmpl[7]) {
  uint8_t b[56] = {0};
  memcpy(b, BPP_DRAW_DOMAIN, BPP_DRAW_DOMAIN_LEN);
  memcpy(b + BPP_DRAW_DOMAIN_LEN, seed.b, seed.len);
  b[BPP_DRAW_DOMAIN_LEN + seed.len + 4] = 0x1F;  // SHAKE's pad byte after le32 j
  memcpy(tmpl, b, 56);
}

// The V phase's inputs from a caller's values, one lane per commitment input
// (P x m lanes, m = nv + 1, after k_draws with v = nullptr on the same stream):
// v[p][j] = src[p * src_stride + index(j)] for j < nv, with index(j) = j for the
// n_id leading identity entries and perm[p][j - n_id] after them (perm [P][nv -
// n_id], each a bijection checked by the entry point before any device work --
// the index is clamped all the same; perm = nullptr: the identity).
//   two-half shuffle  src = cards [P][k], stride k, perm, n_id = k: cards, cards[perm]
//   deck circuit      src = the call's deck [k], stride 0, perm, n_id = 0: deck[perm]
//   circuit           src = the caller's v [P][m_in], stride m_in, no perm
// g[p][j] = the blinding of V_j: the drawn gamma[p][j], or the caller's
// gammas[p][j] ([P][nv]), which then also replaces gamma[p][j] (k_poly_coef
// reads it for tau_x); gx_half[p] = gamma_nv / 2 (always drawn; V_nv is
// committed with halved scalars).  src, gammas, gamma [P][m]: canonical.
__global__ void __launch_bounds__(256) k_v_inputs(uint32_t P, uint32_t nv, uint32_t n_id,
                                                 const uint32_t* __restrict__ src, uint32_t src_stride,
                                                 const uint32_t* __restrict__ perm,
                                                 const uint32_t* __restrict__ gammas, uint32_t* __restrict__ gamma,
                                                 uint32_t* __restrict__ v, uint32_t* __restrict__ g,
                                                 uint32_t* __restrict__ gx_half) {
  const uint32_t m = nv + 1, np = nv - n_id;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * m) return;
  const uint32_t p = (uint32_t)(t / m), j = (uint32_t)(t % m);
  uint32_t* gm = gamma + 8 * ((size_t)p * m + j);
  if (j == nv) {
    sc_store(gx_half + 8 * (size_t)p, sc_half(sc_load(gm)));
    return;
  }
  const uint32_t idx = j < n_id || !perm ? j : min(perm[(size_t)p * np + (j - n_id)], np - 1);
  const size_t o = 8 * ((size_t)p * nv + j);
  sc_store(v + o, sc_load(src + 8 * ((size_t)p * src_stride + idx)));
  sc x;
  if (gammas) {
    x = sc_load(gammas + o);
    sc_store(gm, x);
  } else {
    x = sc_load(gm);
  }
  sc_store(g + o, x);
}

int v_inputs_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_src, uint32_t src_stride,
                 const uint32_t* d_perm, uint32_t n_id, const uint32_t* d_gammas, uint32_t* d_gamma, uint32_t* d_v,
                 uint32_t* d_g, uint32_t* d_gx_half) {
  if (!P) return BPP_OK;
  const size_t nt = (size_t)P * C.m;
  hipLaunchKernelGGL(k_v_inputs, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, ctx->stream, P, C.nv, n_id, d_src,
                     src_stride, d_perm, d_gammas, d_gamma, d_v, d_g, d_gx_half);
  return ctx_check_launch(ctx, "k_v_inputs");
}

// The inclusive prefix products of NC chains of k elements each, one proof
// per workgroup: pref = lds [NC][k] holds them canonical on return (after a
// barrier).  dd(c, i) is element i of chain c, canonical.  Per-lane chunks
// (lane t owns elements [i0, i1) of every chain; nch lanes own any; the rest
// an empty range), then a Hillis-Steele scan of the chunk products in the
// ping-pong buffers [2][NC][blockDim] behind pref, then each chunk times the
// product of the chunks before it.  dynamic LDS = perm::chain_witness_lds.
template <uint32_t NC, class Fetch>
FE_INLINE void chain_prefix_products(uint32_t* lds, uint32_t k, const sc& one, const Fetch& dd) {
  uint32_t* pref = lds;
  uint32_t* scan = lds + 8 * NC * k;
  const uint32_t nt = blockDim.x, t = threadIdx.x;
  const sc oneR = sc_to_mont(one);
  const uint32_t C = (k + nt - 1) / nt, nch = (k + C - 1) / C, i0 = min(t * C, k), i1 = min(i0 + C, k);
  sc run[NC];
  _Pragma("unroll") for (uint32_t c = 0; c < NC; ++c) run[c] = oneR;
  for (uint32_t i = i0; i < i1; ++i)
    _Pragma("unroll") for (uint32_t c = 0; c < NC; ++c) {
      run[c] = sc_mont(run[c], sc_to_mont(dd(c, i)));
      sc_store(pref + 8 * (c * k + i), run[c]);
    }
  // inclusive Hillis-Steele scan of the chunk products, ping-pong buffers
  uint32_t cur = 0;
  _Pragma("unroll") for (uint32_t c = 0; c < NC; ++c) sc_store(scan + 8 * (c * nt + t), run[c]);
  __syncthreads();
  for (uint32_t d = 1; d < nch; d <<= 1) {
    const uint32_t* src = scan + 8 * NC * nt * cur;
    uint32_t* dst = scan + 8 * NC * nt * (cur ^ 1);
    if (t < nch)
      _Pragma("unroll") for (uint32_t c = 0; c < NC; ++c) {
        sc a = sc_load(src + 8 * (c * nt + t));
        if (t >= d) a = sc_mont(sc_load(src + 8 * (c * nt + t - d)), a);
        sc_store(dst + 8 * (c * nt + t), a);
      }
    cur ^= 1;
    __syncthreads();
  }
  // canonical prefixes: mont(e, P) for the canonical product e of the
  // earlier chunks and Montgomery P is e P canonical (one multiply each)
  if (t < nch)
    _Pragma("unroll") for (uint32_t c = 0; c < NC; ++c) {
      const sc e = t > 0 ? sc_from_mont(sc_load(scan + 8 * NC * nt * cur + 8 * (c * nt + t - 1))) : one;
      for (uint32_t i = i0; i < i1; ++i) sc_store(pref + 8 * (c * k + i), sc_mont(e, sc_load(pref + 8 * (c * k + i))));
    }
  __syncthreads();
}

// gate g's a_L, a_R, a_O into their slots of the proof's A_I/A_O/S scalars o
FE_INLINE void witness_gate_store(uint32_t* o, uint32_t n_p, uint32_t g, const sc& aL, const sc& aR, const sc& aO) {
  sc_store(o + 8 * (1 + g), aL);
  sc_store(o + 8 * (1 + n_p + g), aR);
  sc_store(o + 8 * (2 + 2 * n_p + g), aO);
}

// The sound create_a witness of one proof per workgroup (host restatement
// host/perm_circuit.cpp witness, weights.rs:63-113 fixed as SURVEY Q3):
// with d_A[i] = (i + 1) - x and d_B[i] = (pi_i + 1) - x (i < k) and their
// inclusive prefix products A, B (chain_prefix_products<2>), gates g < k - 1
// are (A[g], d_A[g+1], A[g+1]), gates k-1+g' (g' < k-1) are (B[g'], d_B[g'+1],
// B[g'+1]), gate 2k-2 is (B[k-1], -1, -B[k-1]) and gate 2k-1 is (A[k-1] -
// B[k-1], 1, same); padding gates are zero.  a_L, a_R, a_O go straight into
// the A_I/A_O/S scalar array.
//
// CARDS (bpp_perm_prove_shuffle_batch): both chains' values are the caller's
// cards, read from vals ([P][2k] canonical, the V commitments' inputs that
// k_v_inputs wrote: cards then cards[perm]) instead of synthesised from pi;
// the values stay in global memory, the LDS budget is the same.
template <bool CARDS>
FE_INLINE void witness_body(uint32_t* lds, uint32_t k, uint32_t n_p, uint32_t per, const uint32_t* __restrict__ pi,
                            const uint32_t* __restrict__ vals, const uint32_t* __restrict__ xs,
                            uint32_t* __restrict__ sc_out) {
  const uint32_t p = blockIdx.x, nt = blockDim.x, t = threadIdx.x;
  const sc x = sc_load(xs + 8 * (size_t)p);
  sc one = sc_zero();
  one.v[0] = 1;
  auto dd = [&](uint32_t c, uint32_t i) {  // v_i - x: v = i + 1 (A) or pi(i) + 1 (B); or the cards
    sc v = sc_zero();
    if constexpr (CARDS)
      v = sc_load(vals + 8 * ((size_t)p * 2 * k + c * k + i));
    else
      v.v[0] = c == 0 ? i + 1 : pi[(size_t)p * k + i] + 1;
    return sc_sub(v, x);
  };
  chain_prefix_products<2>(lds, k, one, dd);
  uint32_t* o = sc_out + 8 * (size_t)p * per;
  auto pr = [&](uint32_t c, uint32_t i) { return sc_load(lds + 8 * (c * k + i)); };
  for (uint32_t g = t; g < n_p; g += nt) {
    sc aL = sc_zero(), aR = sc_zero(), aO = sc_zero();
    if (g + 1 < k) {
      aL = pr(0, g);
      aR = dd(0, g + 1);
      aO = pr(0, g + 1);
    } else if (g + 2 < 2 * k) {
      const uint32_t h = g - (k - 1);
      aL = pr(1, h);
      aR = dd(1, h + 1);
      aO = pr(1, h + 1);
    } else if (g == 2 * k - 2) {
      aL = pr(1, k - 1);
      aR = sc_neg(one);
      aO = sc_neg(aL);
    } else if (g == 2 * k - 1) {
      aL = sc_sub(pr(0, k - 1), pr(1, k - 1));
      aR = one;
      aO = aL;
    }
    witness_gate_store(o, n_p, g, aL, aR, aO);
  }
}

__global__ void __launch_bounds__(256) k_witness(uint32_t k, uint32_t n_p, uint32_t per, const uint32_t* __restrict__ pi,
                                                const uint32_t* __restrict__ xs, uint32_t* __restrict__ sc_out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_body<false>(lds, k, n_p, per, pi, nullptr, xs, sc_out);
}

__global__ void __launch_bounds__(256) k_witness_cards(uint32_t k, uint32_t n_p, uint32_t per,
                                                      const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ xs, uint32_t* __restrict__ sc_out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_body<true>(lds, k, n_p, per, nullptr, vals, xs, sc_out);
}

// The deck circuit's witness (perm.h build_deck; host restatement
// witness_deck), one proof per workgroup, ONE chain: with d[i] = vals[p][i] -
// x (vals [P][k] canonical: the values the V phase commits, deck[perm], written
// by k_v_inputs) and their inclusive prefix products A
// (chain_prefix_products<1>), gate g < k - 1 is (A[g], d[g+1], A[g+1]); padding
// gates are zero.  Half the two-chain kernels' LDS, so the device witness
// reaches twice their k (perm::chain_witness_dev_max); the host witness beyond.
__global__ void __launch_bounds__(256) k_witness_deck(uint32_t k, uint32_t n_p, uint32_t per,
                                                     const uint32_t* __restrict__ vals,
                                                     const uint32_t* __restrict__ xs, uint32_t* __restrict__ sc_out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t p = blockIdx.x, nt = blockDim.x, t = threadIdx.x;
  const sc x = sc_load(xs + 8 * (size_t)p);
  sc one = sc_zero();
  one.v[0] = 1;
  const uint32_t* vp = vals + 8 * (size_t)p * k;
  auto dd = [&](uint32_t, uint32_t i) { return sc_sub(sc_load(vp + 8 * (size_t)i), x); };
  chain_prefix_products<1>(lds, k, one, dd);
  uint32_t* o = sc_out + 8 * (size_t)p * per;
  for (uint32_t g = t; g < n_p; g += nt) {
    sc aL = sc_zero(), aR = sc_zero(), aO = sc_zero();
    if (g + 1 < k) {
      aL = sc_load(lds + 8 * g);
      aR = dd(0, g + 1);
      aO = sc_load(lds + 8 * (g + 1));
    }
    witness_gate_store(o, n_p, g, aL, aR, aO);
  }
}

int witness_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_pi, const uint32_t* d_x,
                uint32_t per, uint32_t* d_sc, const uint32_t* d_vals) {
  if (!P) return BPP_OK;
  const unsigned nt = perm::chain_witness_lanes(2, C.k);
  const size_t lds = perm::chain_witness_lds(2, C.k);
  if (d_vals) {
    {
      ProfScope ps(ctx, "witness_cards");
      hipLaunchKernelGGL(k_witness_cards, dim3(P), dim3(nt), lds, ctx->stream, C.k, C.n_p, per, d_vals, d_x, d_sc);
    }
    return ctx_check_launch(ctx, "k_witness_cards");
  }
  hipLaunchKernelGGL(k_witness, dim3(P), dim3(nt), lds, ctx->stream, C.k, C.n_p, per, d_pi, d_x, d_sc);
  return ctx_check_launch(ctx, "k_witness");
}

int witness_deck_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_vals, const uint32_t* d_x,
                     uint32_t per, uint32_t* d_sc) {
  if (!P) return BPP_OK;
  if (C.k > DECK_WITNESS_DEV_MAX) {
    ctx->err = "witness_deck_dev: k beyond the kernel's LDS budget";
    return BPP_ERR_LEN;
  }
  hipLaunchKernelGGL(k_witness_deck, dim3(P), dim3(perm::chain_witness_lanes(1, C.k)),
                     perm::chain_witness_lds(1, C.k), ctx->stream, C.k, C.n_p, per, d_vals, d_x, d_sc);
  return ctx_check_launch(ctx, "k_witness_deck");
}
