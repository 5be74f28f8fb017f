// Masked re-shuffle proof, the device steps that the blind re-shuffle does not
// already have (reshuffle.hip): one lane per element (a card, a table row or a
// sum of a proof), 64-wide workgroups, over the helpers of rs_dev.cuh.  The
// protocol is DESIGN.md "Protocol: masked re-shuffle"; the host sequences are
// masked_reshuffle_api.hip.
#include "masked_reshuffle.h"

#include "rs_dev.cuh"

namespace {

unsigned grid_for(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

}  // namespace

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

#define MRS_STEP(name, kern, n, ...)                                                             \
  do {                                                                                           \
    {                                                                                            \
      ProfScope ps(ctx, name);                                                                   \
      hipLaunchKernelGGL(kern, dim3(grid_for((n), 64)), dim3(64), 0, ctx->stream, __VA_ARGS__);  \
    }                                                                                            \
    BPP_TRY(ctx_check_launch(ctx, #kern));                                                       \
  } while (0)

int mrs_key_mul_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* key, uint32_t* out) {
  if (!P) return BPP_OK;
  MRS_STEP("mrs_key_mul", k_mrs_key_mul, (size_t)P * k + P, P, k, draws, key, out);
  return BPP_OK;
}

int mrs_outputs_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* tbl_in, const uint32_t* perms,
                    const uint32_t* rB, const uint32_t* rK, uint32_t* out_enc, uint32_t* out_tbl) {
  if (!P) return BPP_OK;
  MRS_STEP("mrs_outputs", k_mrs_outputs, (size_t)P * k, P, k, tbl_in, perms, rB, rK, out_enc, out_tbl);
  return BPP_OK;
}

int mrs_tsum_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* tbl_out, uint32_t* prod,
                 const uint32_t* tRB, const uint32_t* tRK, uint32_t* res) {
  if (!P) return BPP_OK;
  MRS_STEP("mrs_tsum_mul", k_mrs_tsum_mul, 2 * (size_t)P * k, P, k, draws, tbl_out, prod);
  MRS_STEP("mrs_tsum_sum", k_mrs_tsum_sum, 2 * (size_t)P, P, k, (const uint32_t*)prod, tRB, tRK, res);
  return BPP_OK;
}

int mrs_D_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* tbl, const uint32_t* y, uint32_t* out_p3) {
  if (!P) return BPP_OK;
  MRS_STEP("mrs_D", k_mrs_D, (size_t)P * k, P, k, tbl, y, out_p3);
  return BPP_OK;
}

int mrs_sigma_terms_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, uint32_t stride, const uint32_t* resp,
                        const uint32_t* x, const uint32_t* y, const uint32_t* c, const uint32_t* rho, uint32_t n0,
                        uint32_t bidx, uint32_t bbidx, uint32_t* scal, uint32_t* idx, uint32_t* off, uint32_t* u,
                        uint32_t* scratch) {
  if (!P) return BPP_OK;
  uint32_t *wz = scratch, *ww = wz + 8 * (size_t)P * k, *pp = ww + 8 * (size_t)P * k;
  const uint32_t rows = stride == 6 * k + 5;
  MRS_STEP("mrs_sigma_terms", k_mrs_sigma_terms, (size_t)P * k, P, k, stride, resp, x, y, c, rho, n0, scal, idx, u, wz,
           ww);
  MRS_STEP("mrs_sigma_sums", k_mrs_sigma_sums, (size_t)P, P, k, resp, rho, (const uint32_t*)wz, (const uint32_t*)ww, pp,
           rows, bidx, bbidx, n0, scal, idx, off);
  if (rows) return BPP_OK;
  {
    ProfScope ps(ctx, "mrs_sigma_merge");
    hipLaunchKernelGGL(k_mrs_sigma_merge, dim3(1), dim3(64), 0, ctx->stream, P, (const uint32_t*)pp, bidx, bbidx, n0,
                       scal + 8 * (size_t)P * stride, idx + (size_t)P * stride);
  }
  return ctx_check_launch(ctx, "k_mrs_sigma_merge");
}
