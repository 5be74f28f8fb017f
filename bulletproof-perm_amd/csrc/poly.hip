// Vector-polynomial stage of the batched permutation prover on the GPU
// (the reference's vm_mult / mv_mult /
// inner_product / VecPoly3 work, util.rs:6-94, poly.rs:39-76, batched over
// the proofs of a lockstep batch).  Host side: the transcript challenges
// (y, z, x) and scalar bookkeeping only.
//
// Per proof (one workgroup; lane i handles gates i, i + 256, ...; Montgomery domain,
// R = 2^256 as in sc25519.cuh and host/scalar.h):
//   k_poly_coef  y^i, y^-i, z^(q+1) (LDS), the sparse column sums
//                zW_L, zW_R, zW_O (column-CSR of the circuit matrices), the
//                coefficient vectors of l(X) = l1 X + l2 X^2 + l3 X^3 and
//                r(X) = r0 + r1 X + r3 X^3, and the six t_i = inner products
//                (workgroup reduction) -> host for the T commitments; also
//                <z^Q W_V, gamma> (the V columns of the same CSR against the
//                proof's blindings) -> host for tau_x
//   k_poly_x     l = l(x), r = r(x) straight into the IPA's input arrays,
//                t_hat = <l, r> -> host
// Identical values to the host formulas they replace (perm_prove.hip history;
// oracle/bulletproofs.py prove()), hence identical proof bytes (tests).
#include <algorithm>
#include <cstring>

#include "ctx.h"
#include "poly.h"
#include "host/circuit.h"
#include "sc_poly.cuh"

// grid = P proofs, block = poly_block(max(n_p, m)); dynamic LDS = (Q + 1 + 2 min(n_p, POW_LO)) * 32 + (POLY_T / 64) * 7 * 32
// t_out[p] = t_1..t_6, <z^Q W_V, gamma_p> (gamma: [P][m] canonical)
// (the kernel's text: poly_coef_kernel.inc)
#define POLY_COEF_KERNEL k_poly_coef
#define POLY_COEF_SPLIT false
#include "poly_coef_kernel.inc"
// the row table in two (RowPow): large circuits, or TILED
#define POLY_COEF_KERNEL k_poly_coef_tiled
#define POLY_COEF_SPLIT true
#include "poly_coef_kernel.inc"

// grid = P, block = poly_block(n_p)
__global__ void __launch_bounds__(POLY_T) k_poly_x(uint32_t n_p, const uint32_t* __restrict__ xs,
                                                const uint32_t* __restrict__ vec, uint32_t* __restrict__ l_out,
                                                uint32_t* __restrict__ r_out, uint32_t* __restrict__ that_out) {
  __shared__ __attribute__((aligned(16))) uint32_t red[(POLY_T / 64) * 8];
  const uint32_t p = blockIdx.x;
  const sc xR = sc_to_mont(sc_load(xs + 8 * p));
  const sc x2R = sc_mont(xR, xR);
  sc th[1] = {sc_zero()};
  for (uint32_t i = threadIdx.x; i < n_p; i += blockDim.x) {
    const uint32_t* v = vec + ((size_t)p * n_p + i) * POLY_SLOTS * 8;
    const sc l1 = sc_load(v), r0 = sc_load(v + 8), r1 = sc_load(v + 16), r3 = sc_load(v + 24), l2 = sc_load(v + 32),
             l3 = sc_load(v + 40);
    const sc l = sc_mont(sc_add(l1, sc_mont(sc_add(l2, sc_mont(l3, xR)), xR)), xR);
    const sc r = sc_add(r0, sc_mont(sc_add(r1, sc_mont(r3, x2R)), xR));
    th[0] = sc_add(th[0], sc_mont(l, r));
    sc_store(l_out + ((size_t)p * n_p + i) * 8, sc_from_mont(l));
    sc_store(r_out + ((size_t)p * n_p + i) * 8, sc_from_mont(r));
  }
  sc_block_sum<1>(th, red);
  if (threadIdx.x == 0) sc_store(that_out + 8 * p, sc_from_mont(th[0]));
}

// Column-CSR of WL, WR, WO over the n_p gate columns: cp[3][n_p + 1],
// entries (q, valR[8]) as 9 words; with_v appends WV over its m columns at
// cp[3 (n_p + 1)] (m + 1 offsets, the verifier's V scalars), then the count
// and list of its heavy columns.
void build_csr(const perm::Circuit& C, std::vector<uint32_t>& cp, std::vector<uint32_t>& ce, bool with_v = false) {
  const uint32_t n_p = C.n_p;
  cp.assign(3 * (n_p + 1) + (with_v ? C.m + 1 : 0), 0);
  ce.clear();
  const std::vector<perm::Entry>* Ws[4] = {&C.WL, &C.WR, &C.WO, &C.WV};
  uint32_t total = 0;
  for (int w = 0; w < (with_v ? 4 : 3); ++w) {
    const uint32_t ncol = w == 3 ? C.m : n_p;
    std::vector<std::vector<const perm::Entry*>> cols(ncol);
    for (const perm::Entry& e : *Ws[w]) cols[e.col].push_back(&e);
    for (uint32_t c = 0; c < ncol; ++c) {
      cp[w * (n_p + 1) + c] = total;
      for (const perm::Entry* e : cols[c]) {
        ce.push_back(e->q);
        uint32_t words[8];
        memcpy(words, e->valR.v, 32);
        ce.insert(ce.end(), words, words + 8);
        ++total;
      }
    }
    cp[w * (n_p + 1) + ncol] = total;
  }
  if (with_v) {  // then the V columns too long for one lane (col_sum_block)
    const uint32_t* cpv = &cp[3 * (n_p + 1)];
    std::vector<uint32_t> heavy;
    for (uint32_t j = 0; j < C.m; ++j)
      if (cpv[j + 1] - cpv[j] > HEAVY_COL) heavy.push_back(j);
    cp.push_back((uint32_t)heavy.size());
    cp.insert(cp.end(), heavy.begin(), heavy.end());
  }
}

unsigned poly_block(uint32_t n_p) { return n_p < 64 ? 64u : (n_p > POLY_T ? POLY_T : n_p); }
// lanes per proof of k_poly_coef / k_verify_scalars; the deck circuit's and a
// caller-defined circuit's in whole waves (the deck's m = k + 1 reaches n_p + 2,
// a program's m exceeds n_p by any amount)
unsigned poly_block(const perm::Circuit& C) {
  const unsigned nt = poly_block(std::max(C.n_p, C.m));
  return C.deck || C.program ? std::min<unsigned>(POLY_T, (nt + 63) & ~63u) : nt;
}

int poly_coef_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_sc, uint32_t per,
                  const uint32_t* d_gamma, const std::vector<hsc::Sc>& ch, std::vector<hsc::Sc>& t) {
  std::vector<uint32_t> cp, ce;
  build_csr(C, cp, ce, true);
  void *d_cp, *d_ce, *d_ch, *d_vec, *d_hf, *d_t;
  BPP_TRY(ctx_ws(ctx, "poly_cp", cp.size() * 4, &d_cp));
  BPP_TRY(ctx_ws(ctx, "poly_ce", ce.size() * 4 + 4, &d_ce));

  BPP_TRY(ctx_ws(ctx, "poly_vec", (size_t)P * C.n_p * POLY_SLOTS * 32, &d_vec));
  BPP_TRY(ctx_ws(ctx, "poly_hf", (size_t)P * C.n_p * 32, &d_hf));
  {  // challenges in, t out: pinned host memory the kernel reads / writes in place
    uint32_t *hc = nullptr, *ht = nullptr;
    BPP_TRY(ctx_zc_in(ctx, "poly_ch_h", ch.data(), ch.size() * 32, &hc));
    BPP_TRY(ctx_zc_out(ctx, "poly_t_h", (size_t)P * POLY_NT * 32, &ht));
    d_ch = hc;
    d_t = ht;
  }
  BPP_TRY(ctx_h2d_const(ctx, "poly_cp", d_cp, cp.data(), cp.size() * 4));  // the circuit: same every batch
  BPP_TRY(ctx_h2d_const(ctx, "poly_ce", d_ce, ce.data(), ce.size() * 4));
  const unsigned nt = poly_block(C);
  const bool split = C.program && circuit::poly_coef_split(C);  // (a large circuit's row table, or TILED)
  const size_t lds = split ? perm::split_tables_lds(C.Q, C.n_p, POLY_NT) : perm::poly_coef_lds(C.Q, C.n_p);
  {
    ProfScope ps(ctx, "poly_coef");
    hipLaunchKernelGGL(split ? k_poly_coef_tiled : k_poly_coef, dim3(P), dim3(nt), lds, ctx->stream, C.n_p, C.m, C.Q, per, d_sc,
                       (const uint32_t*)d_ch, (const uint32_t*)d_cp, (const uint32_t*)d_ce, d_gamma,
                       (uint32_t*)d_vec, (uint32_t*)d_hf, (uint32_t*)d_t);
  }
  BPP_TRY(ctx_check_launch(ctx, split ? "k_poly_coef_tiled" : "k_poly_coef"));
  t.resize((size_t)P * POLY_NT);
  BPP_TRY(ctx_sync(ctx));
  memcpy(t.data(), d_t, (size_t)P * POLY_NT * 32);
  return BPP_OK;
}

int poly_x_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const std::vector<hsc::Sc>& x, uint32_t** d_l,
               uint32_t** d_r, uint32_t** d_hf, std::vector<hsc::Sc>& t_hat) {
  void *d_x, *d_vec, *d_lo, *d_ro, *d_th, *hf;

  BPP_TRY(ctx_ws(ctx, "poly_vec", (size_t)P * C.n_p * POLY_SLOTS * 32, &d_vec));
  BPP_TRY(ctx_ws(ctx, "poly_hf", (size_t)P * C.n_p * 32, &hf));
  BPP_TRY(ctx_ws(ctx, "pf_l", (size_t)P * C.n_p * 32 + 32, &d_lo));
  BPP_TRY(ctx_ws(ctx, "pf_r", (size_t)P * C.n_p * 32 + 32, &d_ro));
  {  // x in, t_hat out: in place in pinned host memory
    uint32_t *hx = nullptr, *hth = nullptr;
    BPP_TRY(ctx_zc_in(ctx, "poly_x_h", x.data(), (size_t)P * 32, &hx));
    BPP_TRY(ctx_zc_out(ctx, "poly_that_h", (size_t)P * 32, &hth));
    d_x = hx;
    d_th = hth;
  }
  {
    ProfScope ps(ctx, "poly_x");
    hipLaunchKernelGGL(k_poly_x, dim3(P), dim3(poly_block(C.n_p)), 0, ctx->stream, C.n_p, (const uint32_t*)d_x,
                       (const uint32_t*)d_vec, (uint32_t*)d_lo, (uint32_t*)d_ro, (uint32_t*)d_th);
  }
  BPP_TRY(ctx_check_launch(ctx, "k_poly_x"));
  t_hat.resize(P);
  BPP_TRY(ctx_sync(ctx));
  memcpy(t_hat.data(), d_th, (size_t)P * 32);
  *d_l = (uint32_t*)d_lo;
  *d_r = (uint32_t*)d_ro;
  *d_hf = (uint32_t*)hf;
  return BPP_OK;
}
