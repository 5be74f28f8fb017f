// Re-shuffle proofs, the device steps: one lane per element (a card, a table
// row, a proof or a sum of a proof), 64-wide workgroups, over the field, point
// and scalar arithmetic of fe25519.cuh, ge25519.cuh and sc25519.cuh, the helpers
// of rs_dev.cuh and the Merlin lanes of merlin_lane.cuh.  k_rs_*: the blind
// re-shuffle's kernels and those both kinds run as they are; k_mrs_*: the steps
// a card of two points needs.  The protocols are DESIGN.md "Protocol: blind
// re-shuffle" and "Protocol: masked re-shuffle"; the host sequences are
// reshuffle_api.hip.
#include "reshuffle.h"

#include "ge_io.cuh"
#include "merlin_dev.h"
#include "merlin_lane.cuh"
#include "rs_dev.cuh"
#include "sc25519.cuh"

namespace {

unsigned grid_for(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// One-block SHAKE256 inputs, byte by byte into the zeroed state (every index a
// compile-time constant once unrolled).
FE_INLINE void shake_put(uint64_t a[25], int i, uint32_t byte) { a[i >> 3] ^= (uint64_t)(byte & 0xffu) << (8 * (i & 7)); }
FE_INLINE void shake_put_word(uint64_t a[25], int i, uint32_t w) {
  _Pragma("unroll") for (int b = 0; b < 4; ++b) shake_put(a, i + b, w >> (8 * b));
}
// pads a message of n < 136 bytes, permutes, and reduces the first 64 bytes
FE_INLINE sc shake_wide_scalar(uint64_t a[25], int n) {
  shake_put(a, n, 0x1f);
  shake_put(a, 135, 0x80);
  keccak_f1600_dev(a);
  uint32_t w[16];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) {
    w[2 * i] = (uint32_t)a[i];
    w[2 * i + 1] = (uint32_t)(a[i] >> 32);
  }
  return sc_from_wide_w(w);
}

// merlin's append_message(label, 32 bytes) and challenge_scalar(label) with the
// label packed in a word
FE_INLINE void lane_label(LaneStrobe& s, uint32_t lab, uint32_t ln, uint32_t n) {
  s.begin_op(16u | 2u);  // FLAG_M | FLAG_A
  for (uint32_t i = 0; i < ln; ++i) s.absorb_byte((lab >> (8 * i)) & 0xffu);
  s.absorb_le32(n);
}
FE_INLINE void lane_append32(LaneStrobe& s, uint32_t lab, uint32_t ln, const uint32_t w[8]) {
  lane_label(s, lab, ln, 32);
  s.begin_op(2u);
  s.absorb32(w);
}
FE_INLINE sc lane_challenge(LaneStrobe& s, uint32_t lab, uint32_t ln) {
  lane_label(s, lab, ln, 64);
  s.begin_op(1u | 2u | 4u);  // FLAG_I | FLAG_A | FLAG_C: leaves pos = 0
  uint32_t* d = reinterpret_cast<uint32_t*>(s.st);
  uint32_t w[16];
  _Pragma("unroll") for (int i = 0; i < 16; ++i) {
    w[i] = d[i];
    d[i] = 0;
  }
  s.pos = 64;
  return sc_from_wide_w(w);
}

}  // namespace

// Lane (p, j): draw j of proof p, "bpperm-reshuffle-sc" || seed || le32 j (55
// bytes, one sponge block); the caller's blind in its place for j < k.
__global__ void __launch_bounds__(64) k_rs_draws(uint32_t P, uint32_t k, const uint32_t* __restrict__ seeds,
                                                 const uint32_t* __restrict__ blinds,
                                                 const uint32_t* __restrict__ perms, uint32_t* __restrict__ draws,
                                                 uint32_t* __restrict__ piv, uint32_t* __restrict__ zero) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nd = 5 * k + 1;
  if (t >= (size_t)P * nd) return;
  const uint32_t p = (uint32_t)(t / nd), j = (uint32_t)(t % nd);
  if (j < k) {
    const size_t e = (size_t)p * k + j;
    sc_store(piv + 8 * e, sc_from_u32(perms[e]));
    sc_store(zero + 8 * e, sc_zero());
    if (blinds) {
      sc_store(draws + 8 * e, sc_load(blinds + 8 * e));
      return;
    }
  }
  // section-major: r, alpha, beta, t, w as [P][k] each (pedersen_dev's inputs), then t_R [P]
  const size_t o = j < 5 * k ? (size_t)(j / k) * P * k + (size_t)p * k + j % k : (size_t)5 * P * k + p;
  uint64_t a[25];
  _Pragma("unroll") for (int i = 0; i < 25; ++i) a[i] = 0;
  const char dom[20] = "bpperm-reshuffle-sc";
  _Pragma("unroll") for (int i = 0; i < 19; ++i) shake_put(a, i, (uint8_t)dom[i]);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) shake_put_word(a, 19 + 4 * i, seeds[8 * (size_t)p + i]);
  shake_put_word(a, 51, j);
  sc_store(draws + 8 * o, shake_wide_scalar(a, 55));
}

// Lane (p, i): C'_i = C_perm[i] + r_i Bb.
__global__ void __launch_bounds__(64) k_rs_outputs(uint32_t P, uint32_t k, const uint32_t* __restrict__ tbl_in,
                                                   const uint32_t* __restrict__ perms, const uint32_t* __restrict__ rB,
                                                   uint32_t* __restrict__ out_enc, uint32_t* __restrict__ out_tbl) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k);
  const uint32_t src = perms[t];
  if (src >= k) return;  // (refused by the entry point; never an index out of the table)
  const ge_p3 S = ge_madd(load_p3(rB, t), load_niels(tbl_in, p * k + src));
  uint32_t w[8];
  ge_ristretto_encode(S, w);
  uint4* o = reinterpret_cast<uint4*>(out_enc + 8 * t);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
  store_niels(out_tbl, (uint32_t)t, ge_to_niels(S));
}

// One Merlin lane per proof: the phase's messages, then its challenge.
__global__ void __launch_bounds__(64) k_rs_transcript(uint32_t P, const uint32_t* __restrict__ init,
                                                      uint8_t* __restrict__ states, RsPhase ph,
                                                      uint32_t* __restrict__ ch_out) {
  __shared__ __attribute__((aligned(16))) uint8_t st_lds[64 * LANE_ST_BYTES];
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;  // (no LDS or shuffle shared between lanes)
  LaneStrobe s;
  s.st = st_lds + threadIdx.x * LANE_ST_BYTES;
  uint8_t* g = states + (size_t)p * MERLIN_DEV_STATE_BYTES;
  if (init) {
    uint32_t* d = reinterpret_cast<uint32_t*>(s.st);
    for (int i = 0; i < 50; ++i) d[i] = init[i];
    s.pos = init[50];
    s.pos_begin = init[51];
  } else {
    const uint2* src = reinterpret_cast<const uint2*>(g);
    uint2* dst = reinterpret_cast<uint2*>(s.st);
    for (int i = 0; i < 25; ++i) dst[i] = src[i];
    const uint32_t w = reinterpret_cast<const uint32_t*>(g)[50];
    s.pos = w & 0xffu;
    s.pos_begin = (w >> 8) & 0xffu;
  }
  for (int r = 0; r < 3; ++r) {
    const uint32_t* m = ph.seg[r] + (size_t)p * ph.stride[r];
    for (uint32_t j = 0; j < ph.n[r]; ++j) {
      const uint4 a = reinterpret_cast<const uint4*>(m + 8 * j)[0], b = reinterpret_cast<const uint4*>(m + 8 * j)[1];
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      lane_append32(s, ph.lab[r], ph.ln[r], w);
    }
  }
  const sc ch = lane_challenge(s, ph.ch, ph.chn);
  const uint2* src = reinterpret_cast<const uint2*>(s.st);
  uint2* dst = reinterpret_cast<uint2*>(g);
  for (int i = 0; i < 25; ++i) dst[i] = src[i];
  reinterpret_cast<uint32_t*>(g)[50] = s.pos | (s.pos_begin << 8) | ((1u | 2u | 4u) << 16);
  sc_store(ch_out + 8 * (size_t)p, ch);
}

// Lane (p, i): b_i = x^(perm[i] + 1).
__global__ void __launch_bounds__(64) k_rs_exponents(uint32_t P, uint32_t k, const uint32_t* __restrict__ x,
                                                     const uint32_t* __restrict__ perms, uint32_t* __restrict__ b) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k);
  const sc xR = sc_to_mont(sc_load(x + 8 * (size_t)p));
  sc_store(b + 8 * t, sc_from_mont(sc_pow_mont(xR, perms[t] + 1)));
}

// Lane (p, i): t_i C'_i for the secret nonce t_i, in constant time (ge_ct_mul).
__global__ void __launch_bounds__(64) k_rs_tsum_mul(uint32_t P, uint32_t k, const uint32_t* __restrict__ draws,
                                                    const uint32_t* __restrict__ tbl_out, uint32_t* __restrict__ prod) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)P * k;
  if (t >= n) return;
  const ge_niels A = load_niels(tbl_out, (uint32_t)t);
  const uint32_t* ts = draws + 8 * (3 * n + t);  // (a word per 32 bits: no register array indexed by the bit)
  ge_p3 acc = ge_identity();
  _Pragma("nounroll") for (int bit = 252; bit >= 0; --bit) acc = ge_ct_step(acc, A, (ts[bit >> 5] >> (bit & 31)) & 1u);
  store_p3(prod, t, acc);
}

// Lane p: T_S = sum_i t_i C'_i - t_R Bb.
__global__ void __launch_bounds__(64) k_rs_tsum_sum(uint32_t P, uint32_t k, const uint32_t* __restrict__ prod,
                                                    const uint32_t* __restrict__ tRB, uint32_t* __restrict__ res) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  ge_p3 acc = ge_neg(load_p3(tRB, p));
  _Pragma("nounroll") for (uint32_t i = 0; i < k; ++i) acc = ge_add(acc, load_p3(prod, (size_t)p * k + i));
  store_p3(res, p, acc);
}

// Lane (p, i): z_i, om_i, d_i, delta_i, u_i; lane (p, 0) also z_R.
__global__ void __launch_bounds__(64) k_rs_responses(uint32_t P, uint32_t k, const uint32_t* __restrict__ draws,
                                                     const uint32_t* __restrict__ perms, const uint32_t* __restrict__ b,
                                                     const uint32_t* __restrict__ x, const uint32_t* __restrict__ y,
                                                     const uint32_t* __restrict__ c, uint32_t* __restrict__ resp,
                                                     uint32_t* __restrict__ d, uint32_t* __restrict__ delta,
                                                     uint32_t* __restrict__ u) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k), i = (uint32_t)(t % k);
  const size_t n = (size_t)P * k;
  const sc cR = sc_to_mont(sc_load(c + 8 * (size_t)p)), yR = sc_to_mont(sc_load(y + 8 * (size_t)p));
  const sc bi = sc_load(b + 8 * t);
  const sc alpha = sc_load(draws + 8 * (n + t)), beta = sc_load(draws + 8 * (2 * n + t));
  const sc ti = sc_load(draws + 8 * (3 * n + t)), wi = sc_load(draws + 8 * (4 * n + t));
  uint32_t* rp = resp + 8 * (size_t)p * (2 * k + 1);
  sc_store(rp + 8 * (size_t)i, sc_add(ti, sc_mont(cR, bi)));
  sc_store(rp + 8 * (size_t)(k + i), sc_add(wi, sc_mont(cR, beta)));
  sc_store(d + 8 * t, sc_add(sc_mont(yR, sc_from_u32(perms[t])), bi));
  sc_store(delta + 8 * t, sc_add(sc_mont(yR, alpha), beta));
  const sc xR = sc_to_mont(sc_load(x + 8 * (size_t)p));
  sc_store(u + 8 * t, sc_add(sc_mont(yR, sc_from_u32(i)), sc_from_mont(sc_pow_mont(xR, i + 1))));
  if (i == 0) {
    sc R = sc_zero();  // sum_j b_j r_j
    for (uint32_t j = 0; j < k; ++j) R = sc_add(R, sc_mul(sc_load(b + 8 * (t + j)), sc_load(draws + 8 * (t + j))));
    sc_store(rp + 8 * (size_t)(2 * k), sc_add(sc_load(draws + 8 * (5 * n + p)), sc_mont(cR, R)));
  }
}

// Lane (p, i): D_i = y A_i + E_i by double-and-add over y's bits (y is public).
__global__ void __launch_bounds__(64) k_rs_D(uint32_t P, uint32_t k, const uint32_t* __restrict__ tbl,
                                             const uint32_t* __restrict__ y, uint32_t* __restrict__ out_p3) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k), i = (uint32_t)(t % k);
  const uint32_t base = p * (5 * k + 1);
  const ge_niels A = load_niels(tbl, base + 2 * k + i);
  const uint32_t* ys = y + 8 * (size_t)p;  // (read a word at a time: no register array indexed by the bit)
  ge_p3 acc = ge_identity();
  _Pragma("nounroll") for (int bit = 252; bit >= 0; --bit) {
    acc = ge_dbl(acc);
    if ((ys[bit >> 5] >> (bit & 31)) & 1u) acc = ge_madd(acc, A);
  }
  store_p3(out_p3, t, ge_madd(acc, load_niels(tbl, base + 3 * k + i)));
}

// Lane p: the proof's batch weight, 91 bytes in one sponge block.
__global__ void __launch_bounds__(64) k_rs_weights(uint32_t P, const uint32_t* __restrict__ seed, uint64_t first,
                                                   const uint32_t* __restrict__ c, uint32_t* __restrict__ rho) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  uint64_t a[25];
  _Pragma("unroll") for (int i = 0; i < 25; ++i) a[i] = 0;
  const char dom[20] = "bpperm-reshuffle-wt";
  _Pragma("unroll") for (int i = 0; i < 19; ++i) shake_put(a, i, (uint8_t)dom[i]);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) shake_put_word(a, 19 + 4 * i, seed[i]);
  const uint64_t idx = first + p;
  shake_put_word(a, 51, (uint32_t)idx);
  shake_put_word(a, 55, (uint32_t)(idx >> 32));
  _Pragma("unroll") for (int i = 0; i < 8; ++i) shake_put_word(a, 59 + 4 * i, c[8 * (size_t)p + i]);
  sc_store(rho + 8 * (size_t)p, shake_wide_scalar(a, 91));
}

// Lane (p, i): the weighted terms of T_i, E_i, C'_i, C_i (lane (p, 0): T_S
// too), rho^(i+1) z_i and rho^(i+1) om_i for the sums, and u_i.
__global__ void __launch_bounds__(64) k_rs_sigma_terms(uint32_t P, uint32_t k, uint32_t stride,
                                                       const uint32_t* __restrict__ resp, const uint32_t* __restrict__ x,
                                                       const uint32_t* __restrict__ y, const uint32_t* __restrict__ c,
                                                       const uint32_t* __restrict__ rho, uint32_t n0,
                                                       uint32_t* __restrict__ scal, uint32_t* __restrict__ idx,
                                                       uint32_t* __restrict__ u, uint32_t* __restrict__ wz,
                                                       uint32_t* __restrict__ ww) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k), i = (uint32_t)(t % k);
  const sc rhoR = sc_to_mont(sc_load(rho + 8 * (size_t)p)), xR = sc_to_mont(sc_load(x + 8 * (size_t)p));
  const sc cR = sc_to_mont(sc_load(c + 8 * (size_t)p)), yR = sc_to_mont(sc_load(y + 8 * (size_t)p));
  const sc rpR = sc_pow_mont(rhoR, i + 1), rkR = sc_pow_mont(rhoR, k + 1), eR = sc_pow_mont(xR, i + 1);
  const uint32_t* rs = resp + 8 * (size_t)p * (2 * k + 1);
  const sc z = sc_load(rs + 8 * (size_t)i), om = sc_load(rs + 8 * (size_t)(k + i));
  const size_t row = (size_t)p * stride;
  const uint32_t pt = n0 + p * (5 * k + 1);  // the proof's first table point
  const sc rp = sc_from_mont(rpR);
  sc_store(scal + 8 * (row + i), sc_neg(rp));                    // T_i
  idx[row + i] = pt + 4 * k + i;
  sc_store(scal + 8 * (row + k + i), sc_neg(sc_mont(cR, rp)));   // E_i
  idx[row + k + i] = pt + 3 * k + i;
  sc_store(scal + 8 * (row + 2 * k + i), sc_mont(rkR, z));       // C'_i
  idx[row + 2 * k + i] = pt + k + i;
  const sc rkc = sc_mont(rkR, sc_from_mont(cR));                 // rho^(k+1) c
  sc_store(scal + 8 * (row + 3 * k + i), sc_neg(sc_mont(eR, rkc)));  // C_i
  idx[row + 3 * k + i] = pt + i;
  if (i == 0) {
    sc_store(scal + 8 * (row + 4 * k), sc_neg(sc_from_mont(rkR)));  // T_S
    idx[row + 4 * k] = pt + 5 * k;
  }
  sc_store(wz + 8 * t, sc_mont(rpR, z));
  sc_store(ww + 8 * t, sc_mont(rpR, om));
  sc_store(u + 8 * t, sc_add(sc_mont(yR, sc_from_u32(i)), sc_from_mont(eR)));
}

// Lane p: the proof's B and Bb scalars, sum_i rho^(i+1) z_i and sum_i
// rho^(i+1) om_i - rho^(k+1) z_R -> pp [P][2]; with `rows` (stride 4k + 3) also
// into the proof's own row with the generators' indices, and off.
__global__ void __launch_bounds__(64) k_rs_sigma_sums(uint32_t P, uint32_t k, const uint32_t* __restrict__ resp,
                                                      const uint32_t* __restrict__ rho, const uint32_t* __restrict__ wz,
                                                      const uint32_t* __restrict__ ww, uint32_t* __restrict__ pp,
                                                      uint32_t rows, uint32_t bidx, uint32_t bbidx,
                                                      uint32_t* __restrict__ scal, uint32_t* __restrict__ idx,
                                                      uint32_t* __restrict__ off) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  sc sB = sc_zero(), sBb = sc_zero();
  for (uint32_t i = 0; i < k; ++i) {
    sB = sc_add(sB, sc_load(wz + 8 * ((size_t)p * k + i)));
    sBb = sc_add(sBb, sc_load(ww + 8 * ((size_t)p * k + i)));
  }
  const sc rkR = sc_pow_mont(sc_to_mont(sc_load(rho + 8 * (size_t)p)), k + 1);
  sBb = sc_sub(sBb, sc_mont(rkR, sc_load(resp + 8 * ((size_t)p * (2 * k + 1) + 2 * k))));
  sc_store(pp + 16 * (size_t)p, sB);
  sc_store(pp + 16 * (size_t)p + 8, sBb);
  if (rows) {
    const size_t row = (size_t)p * (4 * k + 3);
    sc_store(scal + 8 * (row + 4 * k + 1), sB);
    idx[row + 4 * k + 1] = bidx;
    sc_store(scal + 8 * (row + 4 * k + 2), sBb);
    idx[row + 4 * k + 2] = bbidx;
    off[p] = (uint32_t)row;
    if (p + 1 == P) off[P] = (uint32_t)(row + 4 * k + 3);
  }
}

// One wave: the batch's B and Bb scalars behind the last proof's terms.
__global__ void __launch_bounds__(64) k_rs_sigma_merge(uint32_t P, const uint32_t* __restrict__ pp, uint32_t bidx,
                                                       uint32_t bbidx, uint32_t* __restrict__ scal,
                                                       uint32_t* __restrict__ idx) {
  sc sB = sc_zero(), sBb = sc_zero();
  for (uint32_t p = threadIdx.x; p < P; p += 64) {
    sB = sc_add(sB, sc_load(pp + 16 * (size_t)p));
    sBb = sc_add(sBb, sc_load(pp + 16 * (size_t)p + 8));
  }
  sB = sc_wave_sum(sB);  // (sums of canonical scalars; lane 0 holds the result)
  sBb = sc_wave_sum(sBb);
  if (threadIdx.x == 0) {
    sc_store(scal, sB);
    idx[0] = bidx;
    sc_store(scal + 8, sBb);
    idx[1] = bbidx;
  }
}

// Lane t < Pk: r_t K; lane Pk + p: t_R K of proof p.  Every lane walks the same
// point; which scalar a lane reads depends on its index alone.
__global__ void __launch_bounds__(64) k_mrs_key_mul(uint32_t P, uint32_t k, const uint32_t* __restrict__ draws,
                                                    const uint32_t* __restrict__ key, uint32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)P * k;
  if (t >= n + P) return;
  const uint32_t* s = draws + 8 * (t < n ? t : 5 * n + (t - n));
  store_p3(out, t, ge_ct_mul(s, load_niels(key, 0)));
}

// Lane (p, i): U'_i = U_perm[i] + r_i B, then W'_i = W_perm[i] + r_i K (one
// half after the other: the registers of one mixed addition and one encoding).
__global__ void __launch_bounds__(64) k_mrs_outputs(uint32_t P, uint32_t k, const uint32_t* __restrict__ tbl_in,
                                                    const uint32_t* __restrict__ perms, const uint32_t* __restrict__ rB,
                                                    const uint32_t* __restrict__ rK, uint32_t* __restrict__ out_enc,
                                                    uint32_t* __restrict__ out_tbl) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k);
  const uint32_t src = perms[t];
  if (src >= k) return;  // (refused by the entry point; never an index out of the table)
  _Pragma("nounroll") for (uint32_t h = 0; h < 2; ++h) {
    const ge_p3 S = ge_madd(load_p3(h ? rK : rB, t), load_niels(tbl_in, 2 * (p * k + src) + h));
    uint32_t w[8];
    ge_ristretto_encode(S, w);
    uint4* o = reinterpret_cast<uint4*>(out_enc + 16 * t + 8 * h);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    store_niels(out_tbl, (uint32_t)(2 * t + h), ge_to_niels(S));
  }
}

// Lane (p, i, h): t_i U'_i (h = 0) or t_i W'_i (h = 1), a lane per table row of
// the output cards: both halves walk the bits of the same t_i.
__global__ void __launch_bounds__(64) k_mrs_tsum_mul(uint32_t P, uint32_t k, const uint32_t* __restrict__ draws,
                                                     const uint32_t* __restrict__ tbl_out, uint32_t* __restrict__ prod) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)P * k;
  if (t >= 2 * n) return;
  store_p3(prod, t, ge_ct_mul(draws + 8 * (3 * n + t / 2), load_niels(tbl_out, (uint32_t)t)));
}

// Lane (p, h): T_U = sum_i t_i U'_i - t_R B (h = 0), T_W = sum_i t_i W'_i -
// t_R K (h = 1).
__global__ void __launch_bounds__(64) k_mrs_tsum_sum(uint32_t P, uint32_t k, const uint32_t* __restrict__ prod,
                                                     const uint32_t* __restrict__ tRB, const uint32_t* __restrict__ tRK,
                                                     uint32_t* __restrict__ res) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * (size_t)P) return;
  const size_t p = t / 2, h = t % 2;
  ge_p3 acc = ge_neg(load_p3(h ? tRK : tRB, p));
  _Pragma("nounroll") for (uint32_t i = 0; i < k; ++i) acc = ge_add(acc, load_p3(prod, 2 * (p * k + i) + h));
  store_p3(res, t, acc);
}

// Lane (p, i): D_i = y A_i + E_i by double-and-add over y's bits (y is public),
// A and E at rows 4k + i and 5k + i of the proof's 7k + 2.
__global__ void __launch_bounds__(64) k_mrs_D(uint32_t P, uint32_t k, const uint32_t* __restrict__ tbl,
                                              const uint32_t* __restrict__ y, uint32_t* __restrict__ out_p3) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k), i = (uint32_t)(t % k);
  const uint32_t base = p * (7 * k + 2);
  const ge_niels A = load_niels(tbl, base + 4 * k + i);
  const uint32_t* ys = y + 8 * (size_t)p;  // (read a word at a time: no register array indexed by the bit)
  ge_p3 acc = ge_identity();
  _Pragma("nounroll") for (int bit = 252; bit >= 0; --bit) {
    acc = ge_dbl(acc);
    if ((ys[bit >> 5] >> (bit & 31)) & 1u) acc = ge_madd(acc, A);
  }
  store_p3(out_p3, t, ge_madd(acc, load_niels(tbl, base + 5 * k + i)));
}

// Lane (p, i): the weighted terms of T_i, E_i, U'_i, W'_i, U_i, W_i (lane (p,
// 0): T_U and T_W too), rho^(i+1) z_i and rho^(i+1) om_i for the sums, and u_i.
__global__ void __launch_bounds__(64) k_mrs_sigma_terms(uint32_t P, uint32_t k, uint32_t stride,
                                                        const uint32_t* __restrict__ resp, const uint32_t* __restrict__ x,
                                                        const uint32_t* __restrict__ y, const uint32_t* __restrict__ c,
                                                        const uint32_t* __restrict__ rho, uint32_t n0,
                                                        uint32_t* __restrict__ scal, uint32_t* __restrict__ idx,
                                                        uint32_t* __restrict__ u, uint32_t* __restrict__ wz,
                                                        uint32_t* __restrict__ ww) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P * k) return;
  const uint32_t p = (uint32_t)(t / k), i = (uint32_t)(t % k);
  const sc rhoR = sc_to_mont(sc_load(rho + 8 * (size_t)p)), xR = sc_to_mont(sc_load(x + 8 * (size_t)p));
  const sc cR = sc_to_mont(sc_load(c + 8 * (size_t)p)), yR = sc_to_mont(sc_load(y + 8 * (size_t)p));
  const sc rpR = sc_pow_mont(rhoR, i + 1), ruR = sc_pow_mont(rhoR, k + 1), eR = sc_pow_mont(xR, i + 1);
  const sc rwR = sc_mont(ruR, rhoR);  // rho^(k+2), Montgomery form
  const uint32_t* rs = resp + 8 * (size_t)p * (2 * k + 1);
  const sc z = sc_load(rs + 8 * (size_t)i), om = sc_load(rs + 8 * (size_t)(k + i));
  const size_t row = (size_t)p * stride;
  const uint32_t pt = n0 + 1 + p * (7 * k + 2);  // the proof's first table point
  const sc rp = sc_from_mont(rpR);
  const sc ce = sc_mont(eR, sc_from_mont(cR));  // c e_i
  sc_store(scal + 8 * (row + i), sc_neg(rp));                          // T_i
  idx[row + i] = pt + 6 * k + i;
  sc_store(scal + 8 * (row + k + i), sc_neg(sc_mont(cR, rp)));         // E_i
  idx[row + k + i] = pt + 5 * k + i;
  sc_store(scal + 8 * (row + 2 * k + i), sc_mont(ruR, z));             // U'_i
  idx[row + 2 * k + i] = pt + 2 * k + 2 * i;
  sc_store(scal + 8 * (row + 3 * k + i), sc_mont(rwR, z));             // W'_i
  idx[row + 3 * k + i] = pt + 2 * k + 2 * i + 1;
  sc_store(scal + 8 * (row + 4 * k + i), sc_neg(sc_mont(ruR, ce)));    // U_i
  idx[row + 4 * k + i] = pt + 2 * i;
  sc_store(scal + 8 * (row + 5 * k + i), sc_neg(sc_mont(rwR, ce)));    // W_i
  idx[row + 5 * k + i] = pt + 2 * i + 1;
  if (i == 0) {
    sc_store(scal + 8 * (row + 6 * k), sc_neg(sc_from_mont(ruR)));      // T_U
    idx[row + 6 * k] = pt + 7 * k;
    sc_store(scal + 8 * (row + 6 * k + 1), sc_neg(sc_from_mont(rwR)));  // T_W
    idx[row + 6 * k + 1] = pt + 7 * k + 1;
  }
  sc_store(wz + 8 * t, sc_mont(rpR, z));
  sc_store(ww + 8 * t, sc_mont(rpR, om));
  sc_store(u + 8 * t, sc_add(sc_mont(yR, sc_from_u32(i)), sc_from_mont(eR)));
}

// Lane p: the proof's B, Bb and K scalars, sum_i rho^(i+1) z_i - rho^(k+1) z_R,
// sum_i rho^(i+1) om_i and -rho^(k+2) z_R -> pp [P][3]; with `rows` (stride
// 6k + 5) also into the proof's own row with the three points' indices, and off.
__global__ void __launch_bounds__(64) k_mrs_sigma_sums(uint32_t P, uint32_t k, const uint32_t* __restrict__ resp,
                                                       const uint32_t* __restrict__ rho, const uint32_t* __restrict__ wz,
                                                       const uint32_t* __restrict__ ww, uint32_t* __restrict__ pp,
                                                       uint32_t rows, uint32_t bidx, uint32_t bbidx, uint32_t kidx,
                                                       uint32_t* __restrict__ scal, uint32_t* __restrict__ idx,
                                                       uint32_t* __restrict__ off) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  sc sB = sc_zero(), sBb = sc_zero();
  for (uint32_t i = 0; i < k; ++i) {
    sB = sc_add(sB, sc_load(wz + 8 * ((size_t)p * k + i)));
    sBb = sc_add(sBb, sc_load(ww + 8 * ((size_t)p * k + i)));
  }
  const sc rhoR = sc_to_mont(sc_load(rho + 8 * (size_t)p));
  const sc ruR = sc_pow_mont(rhoR, k + 1), rwR = sc_mont(ruR, rhoR);
  const sc zR = sc_load(resp + 8 * ((size_t)p * (2 * k + 1) + 2 * k));
  sB = sc_sub(sB, sc_mont(ruR, zR));
  const sc sK = sc_neg(sc_mont(rwR, zR));
  sc_store(pp + 24 * (size_t)p, sB);
  sc_store(pp + 24 * (size_t)p + 8, sBb);
  sc_store(pp + 24 * (size_t)p + 16, sK);
  if (rows) {
    const size_t row = (size_t)p * (6 * k + 5);
    sc_store(scal + 8 * (row + 6 * k + 2), sB);
    idx[row + 6 * k + 2] = bidx;
    sc_store(scal + 8 * (row + 6 * k + 3), sBb);
    idx[row + 6 * k + 3] = bbidx;
    sc_store(scal + 8 * (row + 6 * k + 4), sK);
    idx[row + 6 * k + 4] = kidx;
    off[p] = (uint32_t)row;
    if (p + 1 == P) off[P] = (uint32_t)(row + 6 * k + 5);
  }
}

// One wave: the batch's B, Bb and K scalars behind the last proof's terms.
__global__ void __launch_bounds__(64) k_mrs_sigma_merge(uint32_t P, const uint32_t* __restrict__ pp, uint32_t bidx,
                                                        uint32_t bbidx, uint32_t kidx, uint32_t* __restrict__ scal,
                                                        uint32_t* __restrict__ idx) {
  sc sB = sc_zero(), sBb = sc_zero(), sK = sc_zero();
  for (uint32_t p = threadIdx.x; p < P; p += 64) {
    sB = sc_add(sB, sc_load(pp + 24 * (size_t)p));
    sBb = sc_add(sBb, sc_load(pp + 24 * (size_t)p + 8));
    sK = sc_add(sK, sc_load(pp + 24 * (size_t)p + 16));
  }
  sB = sc_wave_sum(sB);  // (sums of canonical scalars; lane 0 holds the result)
  sBb = sc_wave_sum(sBb);
  sK = sc_wave_sum(sK);
  if (threadIdx.x == 0) {
    sc_store(scal, sB);
    idx[0] = bidx;
    sc_store(scal + 8, sBb);
    idx[1] = bbidx;
    sc_store(scal + 16, sK);
    idx[2] = kidx;
  }
}

// ------------------------------------------------------------ the step layer

// One step: the kernel over n lanes (none: nothing) under its profile name, and
// its launch checked.
#define RS_STEP(name, kern, n, ...)                                                                \
  do {                                                                                             \
    if (n) {                                                                                       \
      {                                                                                            \
        ProfScope ps(ctx, name);                                                                   \
        hipLaunchKernelGGL(kern, dim3(grid_for((n), 64)), dim3(64), 0, ctx->stream, __VA_ARGS__);  \
      }                                                                                            \
      BPP_TRY(ctx_check_launch(ctx, #kern));                                                       \
    }                                                                                              \
  } while (0)

int rs_draws_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* seeds, const uint32_t* blinds,
                 const uint32_t* perms, uint32_t* draws, uint32_t* piv, uint32_t* zero) {
  RS_STEP("rs_draws", k_rs_draws, (size_t)P * rs_draws(k), P, k, seeds, blinds, perms, draws, piv, zero);
  return BPP_OK;
}

int mrs_key_mul_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* key, uint32_t* out) {
  RS_STEP("mrs_key_mul", k_mrs_key_mul, (size_t)P * k + P, P, k, draws, key, out);
  return BPP_OK;
}

int rs_outputs_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, const uint32_t* tbl_in, const uint32_t* perms,
                   const uint32_t* rB, const uint32_t* rK, uint32_t* out_enc, uint32_t* out_tbl) {
  if (H == 1)
    RS_STEP("rs_outputs", k_rs_outputs, (size_t)P * k, P, k, tbl_in, perms, rB, out_enc, out_tbl);
  else
    RS_STEP("mrs_outputs", k_mrs_outputs, (size_t)P * k, P, k, tbl_in, perms, rB, rK, out_enc, out_tbl);
  return BPP_OK;
}

int rs_transcript_dev(bpp_ctx* ctx, uint32_t P, const uint32_t* init, uint8_t* states, const RsPhase& ph,
                      uint32_t* ch_out) {
  RS_STEP("rs_transcript", k_rs_transcript, (size_t)P, P, init, states, ph, ch_out);
  return BPP_OK;
}

int rs_exponents_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* x, const uint32_t* perms, uint32_t* b) {
  RS_STEP("rs_exponents", k_rs_exponents, (size_t)P * k, P, k, x, perms, b);
  return BPP_OK;
}

int rs_tsum_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* tbl_out,
                uint32_t* prod, const uint32_t* tRB, const uint32_t* tRK, uint32_t* res) {
  if (H == 1) {
    RS_STEP("rs_tsum_mul", k_rs_tsum_mul, (size_t)P * k, P, k, draws, tbl_out, prod);
    RS_STEP("rs_tsum_sum", k_rs_tsum_sum, (size_t)P, P, k, (const uint32_t*)prod, tRB, res);
  } else {
    RS_STEP("mrs_tsum_mul", k_mrs_tsum_mul, 2 * (size_t)P * k, P, k, draws, tbl_out, prod);
    RS_STEP("mrs_tsum_sum", k_mrs_tsum_sum, 2 * (size_t)P, P, k, (const uint32_t*)prod, tRB, tRK, res);
  }
  return BPP_OK;
}

int rs_responses_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* perms,
                     const uint32_t* b, const uint32_t* x, const uint32_t* y, const uint32_t* c, uint32_t* resp,
                     uint32_t* d, uint32_t* delta, uint32_t* u) {
  RS_STEP("rs_responses", k_rs_responses, (size_t)P * k, P, k, draws, perms, b, x, y, c, resp, d, delta, u);
  return BPP_OK;
}

int rs_D_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, const uint32_t* tbl, const uint32_t* y,
             uint32_t* out_p3) {
  if (H == 1)
    RS_STEP("rs_D", k_rs_D, (size_t)P * k, P, k, tbl, y, out_p3);
  else
    RS_STEP("mrs_D", k_mrs_D, (size_t)P * k, P, k, tbl, y, out_p3);
  return BPP_OK;
}

int rs_weights_dev(bpp_ctx* ctx, uint32_t P, const uint32_t* seed, uint64_t first, const uint32_t* c, uint32_t* rho) {
  RS_STEP("rs_weights", k_rs_weights, (size_t)P, P, seed, first, c, rho);
  return BPP_OK;
}

int rs_sigma_terms_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, bool each, const uint32_t* resp,
                       const uint32_t* x, const uint32_t* y, const uint32_t* c, const uint32_t* rho, uint32_t n0,
                       uint32_t bidx, uint32_t bbidx, uint32_t* scal, uint32_t* idx, uint32_t* off, uint32_t* u,
                       uint32_t* scratch) {
  if (!P) return BPP_OK;
  uint32_t *wz = scratch, *ww = wz + 8 * (size_t)P * k, *pp = ww + 8 * (size_t)P * k;
  const uint32_t rows = each, stride = rs_terms(H, k) + (each ? H + 1 : 0);
  // (the merge: one wave, its two or three sums behind the last proof's terms)
  uint32_t *const end_s = scal + 8 * (size_t)P * stride, *const end_i = idx + (size_t)P * stride;
  if (H == 1) {
    RS_STEP("rs_sigma_terms", k_rs_sigma_terms, (size_t)P * k, P, k, stride, resp, x, y, c, rho, n0, scal, idx, u, wz, ww);
    RS_STEP("rs_sigma_sums", k_rs_sigma_sums, (size_t)P, P, k, resp, rho, (const uint32_t*)wz, (const uint32_t*)ww, pp,
            rows, bidx, bbidx, scal, idx, off);
    if (!each) RS_STEP("rs_sigma_merge", k_rs_sigma_merge, 64, P, (const uint32_t*)pp, bidx, bbidx, end_s, end_i);
  } else {
    RS_STEP("mrs_sigma_terms", k_mrs_sigma_terms, (size_t)P * k, P, k, stride, resp, x, y, c, rho, n0, scal, idx, u, wz,
            ww);
    RS_STEP("mrs_sigma_sums", k_mrs_sigma_sums, (size_t)P, P, k, resp, rho, (const uint32_t*)wz, (const uint32_t*)ww, pp,
            rows, bidx, bbidx, n0, scal, idx, off);
    if (!each) RS_STEP("mrs_sigma_merge", k_mrs_sigma_merge, 64, P, (const uint32_t*)pp, bidx, bbidx, n0, end_s, end_i);
  }
  return BPP_OK;
}
