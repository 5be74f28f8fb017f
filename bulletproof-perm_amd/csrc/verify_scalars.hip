// The batch verifier's MSM scalars on the GPU: k_verify_consts (each proof's
// batch weight and its constants), k_verify_scalars and its variants (the gate
// and V columns) and k_verify_merge (the generator scalars summed over the
// proofs).  Declared in verify_dev.h; the tables and column sums it shares with
// the prover's polynomial kernels are sc_poly.cuh, the column-CSR poly.h.
#include <cstring>
#include <vector>

#include "ctx.h"
#include "poly.h"
#include "host/circuit.h"
#include "verify_dev.h"
#include "keccak_dev.cuh"
#include "sc_poly.cuh"

// Batch verifier's MSM scalars on the GPU (the verifier side of the same
// circuit algebra, circuit_lib.rs:478-585 in sound form; host restatement
// perm_verify.hip verify_expand, which bpp_perm_verify_scalars still uses).
// One workgroup per proof; rec[p] = VREC_N canonical scalars:
// (VREC_* slots: verify_dev.h)
// Writes wt * (generator scalars) to gen[p][2 n_p + 2] (summed over proofs by
// k_verify_merge) and wt * (proof-point scalars) to sc_out[NG + p npt + j]
// (V_0..V_{m-1}, A_I, A_O, S, T1 T3 T4 T5 T6, L_0.., R_0..), canonical.
#ifdef VS_TIMING  // phase stamps of k_verify_scalars (timing variant only: tools/vs_phases.py)
__device__ unsigned long long vs_dbg[8192 * 8];
#define VS_T(k) \
  if (threadIdx.x == 0 && blockIdx.x < 8192) vs_dbg[blockIdx.x * 8 + (k)] = clock64()
extern "C" int bpp_debug_vs_timing(unsigned long long* out, size_t n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(vs_dbg), n * 8) == hipSuccess ? 0 : 1;
}
#else
#define VS_T(k)
#endif
// Per-proof constants of k_verify_scalars (Montgomery form, VK_N x 8 words
// a proof): every product of two workgroup-uniform values is formed here, on
// the vector unit.  Inside k_verify_scalars such products ran on the scalar
// unit (uniform operands): 21 K SALU instructions per wave next to 15 K VALU,
// ~400 spilled SGPRs, and the CU's one scalar unit shared by its waves (r04
// PMC, tools/vs_phases.py).
//
// No inverses: proof p's check is scaled by F = U^2 Y, U = prod u_j, Y =
// y^(n_p - 1) (nonzero: a zero y or u_j rejects the proof in the replay), so
// that with s_i / s_0 = prod over the bits of i of u^2 (st below) and yr_i =
// y^(n_p - 1 - i):
//   G_i: st[i] U Y a - x zWR_i U^2 yr_i
//   H_i: st[n_p-1-i] U b yr_i - (x zWL_i + zWO_i) U^2 yr_i + F
//   B:   r F t_hat - r x^2 (delta' + F <z^Q, c>) + w F (a b - t_hat),
//        delta' = sum_i U^2 yr_i zWR_i zWL_i
//   B~:  F (r tau_x + mu)
//   V_j: -r x^2 F zWV_j;  A_I A_O S: -F x^(1,2,3);  T_k: -F r x^k
//   L_j: -F u_j^2;  R_j: -Y prod_{k != j} u_k^2
// (F times bulletproofs' verification_scalars / the t-check), all times the
// proof's batch weight w_p = perm::batch_weight(seed, first + p, r_p).
#define VK_Z 0       // z
#define VK_Y 1       // y
#define VK_X 2       // x
#define VK_WT 3      // w_p, the proof's batch weight
#define VK_UYA 4     // w_p U Y a
#define VK_UB 5      // w_p U b
#define VK_WRX2 6    // w_p r x^2
#define VK_WRFT 7    // w_p r F t_hat
#define VK_IB 8      // w_p w F (a b - t_hat)
#define VK_BB 9      // w_p F (r tau_x + mu)
#define VK_R 10      // r
#define VK_NXP 11    // -x_perm
#define VK_U2 12     // U^2
#define VK_F 13      // F
#define VK_WTF 14    // w_p F
#define VK_WRX2F 15  // w_p r x^2 F
#define VK_XU2 16    // w_p x U^2
#define VK_U2W 17    // w_p U^2
#define VK_N 18      // constants a proof

// k_verify_consts works on 16 lanes a proof, 4 proofs a wave, VC_W such
// waves and one Keccak wave a workgroup.  One lane a proof (round 5's first
// version) ran every product of a proof on one lane: ~100 dependent scalar
// multiplies plus the sponge, 67 us for 4096 proofs on 64 waves.  Here the
// proof's multiplies are spread over its 16 lanes in dependency levels: the
// R_j products prod_{k != j} u_k^2, U = prod u_k and Y = y^(2^lg - 1) as one
// lg-step loop (one lane each), the named constants in four levels of at most
// 10 independent products (a table of (op, dst, a, b) per lane), and the
// batch weight's SHAKE256 on the Keccak wave while the loop runs.  Values
// travel through LDS slots (VC_*), the first VK_N of which are the VK_*
// outputs.  The proof-point scalars that are per-proof constants -- A_I,
// A_O, S: -w F x^(1,2,3); T_k: -w F r x^k (k = 1, 3..6); L_j: -w F u_j^2;
// R_j: -w Y prod_{k != j} u_k^2 -- are finished here too and written
// straight to their MSM slots (sc_out[NG + p npt + m + j], canonical), so
// k_verify_scalars is left with the gate and V columns.
#define VC_W 2
#define VC_P (4 * VC_W)  // proofs a workgroup
#define VC_LGMAX 32
#define VC_T_U 18
#define VC_T_YR 19
#define VC_T_A 20
#define VC_T_B 21
#define VC_T_TH 22
#define VC_T_W 23
#define VC_T_TAUX 24
#define VC_T_MU 25
#define VC_T_WR 26
#define VC_T_X2 27
#define VC_T_AB 28
#define VC_T_RT 29
#define VC_T_WU 30
#define VC_T_WY 31
#define VC_T_WX 32
#define VC_T_RTH 33
#define VC_T_ABT 34
#define VC_T_RTM 35
#define VC_T_NWY 36
#define VC_T_WUA 37
#define VC_T_IBT 38
#define VC_NV 39
enum : uint8_t { VC_NOP = 0, VC_MUL, VC_ADD, VC_SUB, VC_NEG };
// level l, lane k: {op, dst, a, b}
__constant__ uint8_t vc_prog[4][16][4] = {
    {{VC_MUL, VK_U2, VC_T_U, VC_T_U},
     {VC_MUL, VC_T_WR, VK_WT, VK_R},
     {VC_MUL, VC_T_X2, VK_X, VK_X},
     {VC_MUL, VC_T_AB, VC_T_A, VC_T_B},
     {VC_MUL, VC_T_RT, VK_R, VC_T_TAUX},
     {VC_MUL, VC_T_WU, VK_WT, VC_T_U},
     {VC_MUL, VC_T_WY, VK_WT, VC_T_YR},
     {VC_MUL, VC_T_WX, VK_WT, VK_X},
     {VC_MUL, VC_T_RTH, VK_R, VC_T_TH}},
    {{VC_MUL, VK_F, VK_U2, VC_T_YR},
     {VC_MUL, VK_WRX2, VC_T_WR, VC_T_X2},
     {VC_MUL, VC_T_WUA, VC_T_WU, VC_T_A},
     {VC_MUL, VK_UB, VC_T_WU, VC_T_B},
     {VC_MUL, VK_XU2, VC_T_WX, VK_U2},
     {VC_MUL, VK_U2W, VK_WT, VK_U2},
     {VC_MUL, VK_WTF, VC_T_WY, VK_U2},
     {VC_SUB, VC_T_ABT, VC_T_AB, VC_T_TH},
     {VC_ADD, VC_T_RTM, VC_T_RT, VC_T_MU},
     {VC_NEG, VC_T_NWY, VC_T_WY, 0}},
    {{VC_MUL, VK_UYA, VC_T_WUA, VC_T_YR},
     {VC_MUL, VK_WRFT, VK_WTF, VC_T_RTH},
     {VC_MUL, VC_T_IBT, VC_T_W, VC_T_ABT},
     {VC_MUL, VK_BB, VK_WTF, VC_T_RTM},
     {VC_MUL, VK_WRX2F, VK_WRX2, VK_F}},
    {{VC_MUL, VK_IB, VK_WTF, VC_T_IBT}},
};
// (record slot, value slot) of the loaded proof values
__constant__ uint8_t vc_load[11][2] = {{VREC_Z, VK_Z},     {VREC_Y, VK_Y},         {VREC_X, VK_X},
                                       {VREC_R, VK_R},     {VREC_XPERM, VK_NXP},   {VREC_A, VC_T_A},
                                       {VREC_B, VC_T_B},   {VREC_THAT, VC_T_TH},   {VREC_W, VC_T_W},
                                       {VREC_TAUX, VC_T_TAUX}, {VREC_MU, VC_T_MU}};
__global__ void __launch_bounds__(64 * (VC_W + 1)) k_verify_consts(uint32_t count, uint32_t lg, uint64_t first,
                                                                   const uint32_t* __restrict__ seed,
                                                                   const uint32_t* __restrict__ rec,
                                                                   uint32_t* __restrict__ kc, uint32_t NG, uint32_t m,
                                                                   uint32_t npt, uint32_t* __restrict__ sc_out) {
  __builtin_amdgcn_s_setprio(3);  // (latency chain; the decompression runs beside it)
  __shared__ __attribute__((aligned(16))) uint32_t vs[VC_P][VC_NV * 8];
  __shared__ __attribute__((aligned(16))) uint32_t ut[VC_P][VC_LGMAX * 8], u2t[VC_P][VC_LGMAX * 8],
      pjt[VC_P][VC_LGMAX * 8];
  const uint32_t nrec = VREC_U + lg;
  const bool kwave = threadIdx.x >= 64 * VC_W;
  const uint32_t g = (threadIdx.x >> 4) & (VC_P - 1), l = threadIdx.x & 15u;
  const uint32_t p = blockIdx.x * VC_P + g;
  const bool live = !kwave && p < count;
  const uint32_t* R = rec + (size_t)p * nrec * 8;
  uint32_t* V = vs[g];
  const sc oneR = sc_one_mont();
  auto ldv = [&](uint32_t k) { return sc_load(V + 8 * k); };
  if (live) {
    if (l < 11) {
      sc v = sc_to_mont(sc_load(R + 8 * vc_load[l][0]));
      if (vc_load[l][1] == VK_NXP) v = sc_neg(v);
      sc_store(V + 8 * vc_load[l][1], v);
    }
    for (uint32_t j = l; j < lg; j += 16) {
      const sc u = sc_to_mont(sc_load(R + 8 * (VREC_U + j)));
      sc_store(ut[g] + 8 * j, u);
      sc_store(u2t[g] + 8 * j, sc_mont(u, u));
    }
  }
  __syncthreads();
  if (live) {
    // lanes j < lg: prod_{k != j} u_k^2; lane lg: U; lane lg + 1: Y
    const sc yR = ldv(VK_Y);
    for (uint32_t jj = l; jj < lg + 2; jj += 16) {
      const bool isY = jj == lg + 1, isU = jj == lg;
      sc v = oneR;
      for (uint32_t k = 0; k < lg; ++k) {
        const sc f = isY ? v : isU ? sc_load(ut[g] + 8 * k) : k == jj ? oneR : sc_load(u2t[g] + 8 * k);
        v = sc_mont(v, f);
        if (isY) v = sc_mont(v, yR);
      }
      sc_store(isY ? V + 8 * VC_T_YR : isU ? V + 8 * VC_T_U : pjt[g] + 8 * jj, v);
    }
  } else if (kwave && (threadIdx.x & 63u) < VC_P && blockIdx.x * VC_P + (threadIdx.x & 63u) < count) {
    // w_p = from_wide(SHAKE256("bp-perm-batch-wt" || seed || le64(first + p) ||
    // r_p)[0..64]): 88 bytes, one sponge block (perm::batch_weight)
    const uint32_t q = threadIdx.x & 63u, pq = blockIdx.x * VC_P + q;
    uint64_t a[25];
    _Pragma("unroll") for (int i = 0; i < 25; ++i) a[i] = 0;
    a[0] = 0x6d7265702d7062ull | (0x2dull << 56);  // "bp-perm-"
    a[1] = 0x74772d6863746162ull;                 // "batch-wt"
    _Pragma("unroll") for (int i = 0; i < 4; ++i) a[2 + i] = (uint64_t)seed[2 * i] | ((uint64_t)seed[2 * i + 1] << 32);
    a[6] = first + pq;
    const uint32_t* rp = rec + ((size_t)pq * nrec + VREC_R) * 8;
    _Pragma("unroll") for (int i = 0; i < 4; ++i) a[7 + i] = (uint64_t)rp[2 * i] | ((uint64_t)rp[2 * i + 1] << 32);
    a[11] = 0x1full;        // SHAKE domain byte at 88
    a[16] = 0x80ull << 56;  // last byte of the 136-byte rate
    keccak_f1600_dev(a);
    uint32_t o[16];
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {
      o[2 * i] = (uint32_t)a[i];
      o[2 * i + 1] = (uint32_t)(a[i] >> 32);
    }
    sc_store(vs[q] + 8 * VK_WT, sc_to_mont(sc_from_wide_w(o)));
  }
  __syncthreads();
  for (uint32_t lv = 0; lv < 4; ++lv) {
    if (live && vc_prog[lv][l][0] != VC_NOP) {
      const uint8_t op = vc_prog[lv][l][0];
      const sc x = ldv(vc_prog[lv][l][2]), y = ldv(vc_prog[lv][l][3]);
      const sc r = op == VC_MUL ? sc_mont(x, y) : op == VC_ADD ? sc_add(x, y) : op == VC_SUB ? sc_sub(x, y) : sc_neg(x);
      sc_store(V + 8 * vc_prog[lv][l][1], r);
    }
    __syncthreads();
  }
  if (live) {
    uint32_t* K = kc + (size_t)p * VK_N * 8;
    for (uint32_t w = l; w < VK_N * 8; w += 16) K[w] = V[w];
    // the proof-point scalars after V_0..V_{m-1}
    uint32_t* out = sc_out + 8 * ((size_t)NG + (size_t)p * npt + m);
    const sc xR = ldv(VK_X), nwtf = sc_neg(ldv(VK_WTF));
    for (uint32_t j = l; j < 8 + 2 * lg; j += 16) {
      sc v;
      if (j >= 8 + lg) {
        v = sc_mont(sc_load(pjt[g] + 8 * (j - 8 - lg)), ldv(VC_T_NWY));
      } else {
        if (j < 3) {
          v = sc_pow_small(xR, j + 1, oneR);
        } else if (j < 8) {
          v = sc_mont(ldv(VK_R), sc_pow_small(xR, j == 3 ? 1u : j - 1, oneR));  // T1, T3, T4, T5, T6
        } else {
          v = sc_load(u2t[g] + 8 * (j - 8));
        }
        v = sc_mont(v, nwtf);
      }
      sc_store(out + 8 * j, sc_from_mont(v));
    }
  }
}

// (at 4 waves per SIMD: 128 VGPRs instead of 148, 108 B of spills, 8
// workgroups per CU instead of 6 -- 2 rounds for 4096 proofs instead of 2.7;
// three interleaved passes 0.281-0.283 vs 0.294-0.297 ms with the constants
// and the merge, 0.309-0.312 at 5, profiles/r04_verify_vs_ab.txt)
#ifndef VS_WPE
#define VS_WPE 4
#endif
//
// DECK (the deck circuit, perm.h build_deck): the circuit's second per-proof
// constant c[Q-2] = D = prod_i (deck_i - x_perm) over the call's public deck
// (deck [k] canonical scalars in device memory, once per call): per-lane
// strided partial products, then a tree over the workgroup in LDS (blockDim
// more scalars behind the reduction scratch), added to <z^Q, c> by lane 0.
//
// PUB (a circuit with public inputs, circuit.h): the proof's constant vector is
// c + W_U u_p, so <z^Q, c_p> takes sum_e z^(q_e + 1) W_U.val_e u_{p, col_e} more.
// Entry-parallel over the workgroup (lane t: entries t, t + blockDim, ..., of
// the flat list wu = [n_wu][q, col] then, from a multiple of 8 words, [n_wu]
// Montgomery values), added to the lane's own acc[1] before the block sum: no
// barrier, no reduction and no LDS of its own, and a public input read by many
// rows costs what its entries cost.  pub: [count][n_pub][8] words, canonical.
//
// SPLIT (the _tiled kernels; large circuits): the row table in two (RowPow);
// dynamic LDS = perm::split_tables_lds(Q, n_p, 2).
template <bool DECK, bool PUB = false, bool SPLIT = false>
FE_INLINE void verify_scalars_body(uint32_t* lds, uint32_t n_p, uint32_t m, uint32_t Q, uint32_t lg,
                                   const uint32_t* __restrict__ rec, const uint32_t* __restrict__ kc,
                                   const uint32_t* __restrict__ cp, const uint32_t* __restrict__ ce,
                                   const uint32_t* __restrict__ cR, uint32_t* __restrict__ gen,
                                   uint32_t* __restrict__ sc_out, uint32_t NG, uint32_t npt,
                                   const uint32_t* __restrict__ deck, uint32_t k,
                                   const uint32_t* __restrict__ wu = nullptr, uint32_t n_wu = 0,
                                   const uint32_t* __restrict__ pub = nullptr, uint32_t n_pub = 0) {
  __builtin_amdgcn_s_setprio(2);  // (ahead of the proof-point decompression beside it)
  const uint32_t NY = min(n_p, (uint32_t)POW_LO);
  const uint32_t NZ = SPLIT ? (uint32_t)ROW_LO : Q + 1, NH = SPLIT ? (Q >> ROW_LO_LG) + 1 : 0u;
  uint32_t* zt = lds;                // [Q + 1] z^e, Montgomery; SPLIT: [ROW_LO] z^i
  uint32_t* zh = zt + 8 * NZ;        // SPLIT: [NH] z^(ROW_LO j)
  uint32_t* yt = zh + 8 * NH;        // [NY] y^e
  uint32_t* st = yt + 8 * NY;        // [NY] s_i / s_0 (below)
  uint32_t* red = st + 8 * NY;       // reduction scratch
  const RowPow<SPLIT> zp = {SPLIT ? zt : zt + 8, zh};  // z^(q+1)
  const uint32_t p = blockIdx.x, nrec = VREC_U + lg;
  const uint32_t* R = rec + (size_t)p * nrec * 8;
  const uint32_t* K = kc + (size_t)p * VK_N * 8;
  const sc oneR = sc_one_mont();
  auto ldm = [&](uint32_t k) { return sc_to_mont(sc_load(R + 8 * k)); };
  auto ldk = [&](uint32_t k) { return sc_load(K + 8 * k); };
  VS_T(0);
  // s_i = s_0 prod_{bit k of i} u_{lg-1-k}^2 (bulletproofs
  // verification_scalars): st[i] = s_i / s_0 for i < NY as a doubling table
  // over the factors u_{lg-1-k}^2, the bits from POW_LO_LG up per lane
  if (threadIdx.x == 0) {
    sc_table_pow_init(zt, NZ, ldk(VK_Z), oneR);
    sc_table_pow_init(yt, NY, ldk(VK_Y), oneR);
    sc_store(st, oneR);
  }
  for (uint32_t b = threadIdx.x; b < POW_LO_LG && (1u << b) < NY; b += blockDim.x) {
    const sc u = ldm(VREC_U + lg - 1 - b);
    sc_store(st + 8 * (1u << b), sc_mont(u, u));
  }
  sc_tables3({zt, NZ, false}, {yt, NY, false}, {st, NY, true});
  if constexpr (SPLIT) row_hi_table(zh, NH, zt, ldk(VK_Z), oneR);
  VS_T(1);
  auto s_of = [&](uint32_t i) {  // s_i / s_0
    sc v = sc_load(st + 8 * (i % POW_LO));
    for (uint32_t k = POW_LO_LG; k < lg; ++k)
      if ((i >> k) & 1u) {
        const sc u = ldm(VREC_U + lg - 1 - k);
        v = sc_mont(v, sc_mont(u, u));
      }
    return v;
  };
  // (weighted: w_p folded into the constants)
  const sc uyaR = ldk(VK_UYA), ubR = ldk(VK_UB), xu2R = ldk(VK_XU2), u2R = ldk(VK_U2W), fR = ldk(VK_WTF);
  // gate i = n_p - 1 - e with e ascending per lane: yr_i = y^e = yt[e mod
  // POW_LO] (y^POW_LO)^(e / POW_LO), the second factor a running product
  // (blockDim = POW_LO whenever n_p > POW_LO)
  sc yhi = oneR, ystep = oneR;
  if (n_p > POW_LO) ystep = sc_mont(sc_load(yt + 8 * (POW_LO - 1)), ldk(VK_Y));
  const size_t gb = (size_t)p * NG;
  // acc[0]: delta'' = sum yr_i zWR_i zWL_i (delta' = U^2 delta'', applied
  // once below); acc[1]: zc = <z^Q, c>
  sc acc[2] = {sc_zero(), sc_zero()};
  for (uint32_t e = threadIdx.x; e < n_p; e += blockDim.x) {
    const uint32_t i = n_p - 1 - e;
    sc yr = sc_load(yt + 8 * (e % POW_LO));
    if (e >= POW_LO) yr = sc_mont(yr, yhi);
    if (n_p > POW_LO) yhi = sc_mont(yhi, ystep);
    const sc zWL = col_sum(cp, ce, i, zp), zWR = col_sum(cp + (n_p + 1), ce, i, zp),
             zWO = col_sum(cp + 2 * (n_p + 1), ce, i, zp);
    const sc rw = sc_mont(zWR, yr);
    acc[0] = sc_add(acc[0], sc_mont(rw, zWL));
    // G_i: st[i] U Y a - (zWR yr) x U^2;  H_i: (st[e] U b - zWL x U^2 - zWO U^2) yr + F
    const sc gi = sc_sub(sc_mont(s_of(i), uyaR), sc_mont(rw, xu2R));
    const sc hi = sc_add(sc_mont(sc_sub(sc_sub(sc_mont(s_of(e), ubR), sc_mont(zWL, xu2R)), sc_mont(zWO, u2R)), yr),
                         fR);
    sc_store(gen + 8 * (gb + i), sc_from_mont(gi));
    sc_store(gen + 8 * (gb + n_p + i), sc_from_mont(hi));
  }
  VS_T(2);
  for (uint32_t q = threadIdx.x; q < Q; q += blockDim.x) {
    const sc c = q + 1 == Q ? ldk(VK_NXP) : sc_to_mont(sc_load(cR + 8 * q));
    acc[1] = sc_add(acc[1], sc_mont(row_at(zp, q), c));
  }
  if constexpr (PUB) {
    const uint32_t* wv = wu + ((2 * n_wu + 7) & ~7u);
    const uint32_t* up = pub + 8 * (size_t)p * n_pub;
    for (uint32_t e = threadIdx.x; e < n_wu; e += blockDim.x) {
      const sc au = sc_mont(sc_load(wv + 8 * (size_t)e), sc_to_mont(sc_load(up + 8 * (size_t)wu[2 * e + 1])));
      acc[1] = sc_add(acc[1], sc_mont(row_at(zp, wu[2 * e]), au));
    }
  }
  VS_T(3);
  const sc wrx2fR = ldk(VK_WRX2F);
  const size_t pb = NG + (size_t)p * npt;
  // V_j: -wt r x^2 F zWV_j (zWV from the fourth column-CSR, m columns; the
  // heavy x column summed by the whole workgroup)
  const uint32_t* cpv = cp + 3 * (n_p + 1);
  for (uint32_t j = threadIdx.x; j < m; j += blockDim.x)
    if (cpv[j + 1] - cpv[j] <= HEAVY_COL)
      sc_store(sc_out + 8 * (pb + j), sc_from_mont(sc_neg(sc_mont(col_sum(cpv, ce, j, zp), wrx2fR))));
  const uint32_t* heavy = cpv + m + 1;  // [count, columns...] (build_csr)
  for (uint32_t h = 0; h < heavy[0]; ++h) {
    const uint32_t j = heavy[1 + h];
    const sc cs = col_sum_block(cpv, ce, j, zp, red);
    if (threadIdx.x == 0) sc_store(sc_out + 8 * (pb + j), sc_from_mont(sc_neg(sc_mont(cs, wrx2fR))));
  }
  VS_T(4);
  // (A_I .. R_j: written by k_verify_consts)
  VS_T(5);
  sc_block_sum<2>(acc, red);
  VS_T(6);
  if constexpr (DECK) {
    uint32_t* prod = red + (POLY_T / 64) * 2 * 8;  // [blockDim] partial products
    const sc nxp = ldk(VK_NXP);
    sc pr = oneR;
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x)
      pr = sc_mont(pr, sc_add(sc_to_mont(sc_load(deck + 8 * (size_t)i)), nxp));
    __syncthreads();  // (red: lane 0 has read the block sums)
    sc_store(prod + 8 * threadIdx.x, pr);
    __syncthreads();
    for (uint32_t n = blockDim.x; n > 1;) {  // any blockDim: the upper half folds onto the lower
      const uint32_t h = (n + 1) / 2;
      if (threadIdx.x < n / 2)
        sc_store(prod + 8 * threadIdx.x, sc_mont(sc_load(prod + 8 * threadIdx.x), sc_load(prod + 8 * (threadIdx.x + h))));
      n = h;
      __syncthreads();
    }
    if (threadIdx.x == 0) acc[1] = sc_add(acc[1], sc_mont(row_at(zp, Q - 2), sc_load(prod)));
  }
  if (threadIdx.x == 0) {
    // B: wt (r F t_hat - r x^2 (delta' + F zc) + w F (a b - t_hat)); B_blinding: wt F (r tau_x + mu)
    const sc tB =
        sc_sub(ldk(VK_WRFT), sc_mont(ldk(VK_WRX2), sc_add(sc_mont(ldk(VK_U2), acc[0]), sc_mont(ldk(VK_F), acc[1]))));
    sc_store(gen + 8 * (gb + 2 * n_p), sc_from_mont(sc_add(tB, ldk(VK_IB))));
    sc_store(gen + 8 * (gb + 2 * n_p + 1), sc_from_mont(ldk(VK_BB)));
  }
  VS_T(7);
}

__global__ void __launch_bounds__(POLY_T) __attribute__((amdgpu_waves_per_eu(VS_WPE))) k_verify_scalars(
    uint32_t n_p, uint32_t m, uint32_t Q, uint32_t lg, const uint32_t* __restrict__ rec,
    const uint32_t* __restrict__ kc, const uint32_t* __restrict__ cp, const uint32_t* __restrict__ ce,
    const uint32_t* __restrict__ cR, uint32_t* __restrict__ gen, uint32_t* __restrict__ sc_out, uint32_t NG,
    uint32_t npt) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  verify_scalars_body<false>(lds, n_p, m, Q, lg, rec, kc, cp, ce, cR, gen, sc_out, NG, npt, nullptr, 0);
}

// dynamic LDS = k_verify_scalars' + blockDim x 32 B
__global__ void __launch_bounds__(POLY_T) __attribute__((amdgpu_waves_per_eu(VS_WPE))) k_verify_scalars_deck(
    uint32_t n_p, uint32_t m, uint32_t Q, uint32_t lg, const uint32_t* __restrict__ rec,
    const uint32_t* __restrict__ kc, const uint32_t* __restrict__ cp, const uint32_t* __restrict__ ce,
    const uint32_t* __restrict__ cR, uint32_t* __restrict__ gen, uint32_t* __restrict__ sc_out, uint32_t NG,
    uint32_t npt, const uint32_t* __restrict__ deck, uint32_t k) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  verify_scalars_body<true>(lds, n_p, m, Q, lg, rec, kc, cp, ce, cR, gen, sc_out, NG, npt, deck, k);
}

// (dynamic LDS = k_verify_scalars')
__global__ void __launch_bounds__(POLY_T) __attribute__((amdgpu_waves_per_eu(VS_WPE))) k_verify_scalars_pub(
    uint32_t n_p, uint32_t m, uint32_t Q, uint32_t lg, const uint32_t* __restrict__ rec,
    const uint32_t* __restrict__ kc, const uint32_t* __restrict__ cp, const uint32_t* __restrict__ ce,
    const uint32_t* __restrict__ cR, uint32_t* __restrict__ gen, uint32_t* __restrict__ sc_out, uint32_t NG,
    uint32_t npt, const uint32_t* __restrict__ wu, uint32_t n_wu, const uint32_t* __restrict__ pub, uint32_t n_pub) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  verify_scalars_body<false, true>(lds, n_p, m, Q, lg, rec, kc, cp, ce, cR, gen, sc_out, NG, npt, nullptr, 0, wu, n_wu,
                                   pub, n_pub);
}

#define VERIFY_SCALARS_ARGS                                                                                          \
  uint32_t n_p, uint32_t m, uint32_t Q, uint32_t lg, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ kc, \
      const uint32_t *__restrict__ cp, const uint32_t *__restrict__ ce, const uint32_t *__restrict__ cR,            \
      uint32_t *__restrict__ gen, uint32_t *__restrict__ sc_out, uint32_t NG, uint32_t npt
#define VERIFY_SCALARS_PASS lds, n_p, m, Q, lg, rec, kc, cp, ce, cR, gen, sc_out, NG, npt, nullptr, 0
// (dynamic LDS = perm::split_tables_lds(Q, n_p, 2))
__global__ void __launch_bounds__(POLY_T) __attribute__((amdgpu_waves_per_eu(VS_WPE))) k_verify_scalars_tiled(
    VERIFY_SCALARS_ARGS) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  verify_scalars_body<false, false, true>(VERIFY_SCALARS_PASS);
}
__global__ void __launch_bounds__(POLY_T) __attribute__((amdgpu_waves_per_eu(VS_WPE))) k_verify_scalars_pub_tiled(
    VERIFY_SCALARS_ARGS, const uint32_t* __restrict__ wu, uint32_t n_wu, const uint32_t* __restrict__ pub,
    uint32_t n_pub) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  verify_scalars_body<false, true, true>(VERIFY_SCALARS_PASS, wu, n_wu, pub, n_pub);
}

// sc_out[i] = sum_p gen[p][i] (one workgroup per generator column)
__global__ void __launch_bounds__(POLY_T) k_verify_merge(uint32_t count, uint32_t NG, const uint32_t* __restrict__ gen,
                                                      uint32_t* __restrict__ sc_out) {
  __shared__ __attribute__((aligned(16))) uint32_t red[(POLY_T / 64) * 8];
  const uint32_t i = blockIdx.x;
  sc acc[1] = {sc_zero()};
  for (uint32_t p = threadIdx.x; p < count; p += blockDim.x) acc[0] = sc_add(acc[0], sc_load(gen + 8 * ((size_t)p * NG + i)));
  sc_block_sum<1>(acc, red);
  if (threadIdx.x == 0) sc_store(sc_out + 8 * i, acc[0]);
}

int verify_scalars_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t count, const std::vector<uint32_t>& rec,
                       const uint8_t seed[32], uint64_t first, uint32_t* d_sc) {
  uint32_t *h = nullptr, *hs = nullptr;  // per-proof records read in place from pinned host memory (ctx_zc_in)
  BPP_TRY(ctx_zc_in(ctx, "vs_rec_h", rec.data(), rec.size() * 4, &h));
  BPP_TRY(ctx_zc_in(ctx, "vs_seed_h", seed, 32, &hs));
  return verify_scalars_dev_rec(ctx, C, count, h, hs, first, d_sc);
}

int verify_scalars_dev_rec(bpp_ctx* ctx, const perm::Circuit& C, uint32_t count, const uint32_t* d_rec,
                           const uint32_t* seed, uint64_t first, uint32_t* d_sc, const uint32_t* d_pub) {
  if (C.n_pub && !d_pub) return BPP_ERR_ARG;
  std::vector<uint32_t> cp, ce;
  build_csr(C, cp, ce, true);
  std::vector<uint32_t> cw((size_t)C.Q * 8);
  for (uint32_t q = 0; q < C.Q; ++q) memcpy(&cw[8 * (size_t)q], C.c[q].v, 32);
  const uint32_t NG = 2 * C.n_p + 2, npt = C.m + 8 + 2 * C.lg;
  void *d_cp, *d_ce, *d_c, *d_gen;
  BPP_TRY(ctx_ws(ctx, "vs_cp", cp.size() * 4, &d_cp));
  BPP_TRY(ctx_ws(ctx, "vs_ce", ce.size() * 4 + 4, &d_ce));
  BPP_TRY(ctx_ws(ctx, "vs_c", cw.size() * 4, &d_c));

  BPP_TRY(ctx_ws(ctx, "vs_gen", (size_t)count * NG * 32, &d_gen));
  BPP_TRY(ctx_h2d_const(ctx, "vs_cp", d_cp, cp.data(), cp.size() * 4));  // the circuit: same every batch
  BPP_TRY(ctx_h2d_const(ctx, "vs_ce", d_ce, ce.data(), ce.size() * 4));
  BPP_TRY(ctx_h2d_const(ctx, "vs_c", d_c, cw.data(), cw.size() * 4));
  const unsigned nt = poly_block(C);
  const bool split = C.program && circuit::verify_scalars_split(C);  // (a large circuit's row table, or TILED)
  const size_t lds = split ? perm::split_tables_lds(C.Q, C.n_p, 2) : perm::verify_scalars_lds(C.Q, C.n_p);
  if (C.lg > VC_LGMAX) return BPP_ERR_LEN;  // (k_verify_consts' LDS tables)
  void *d_kc = nullptr, *d_deck = nullptr;
  BPP_TRY(ctx_ws(ctx, "vs_kc", (size_t)count * VK_N * 32, &d_kc));
  if (C.deck) {  // the call's public deck, for c[Q-2] = prod (d_i - x_perm)
    BPP_TRY(ctx_ws(ctx, "vs_deck", (size_t)C.k * 32, &d_deck));
    BPP_TRY(ctx_h2d_const(ctx, "vs_deck", d_deck, C.cards.data(), (size_t)C.k * 32));
  }
  void* d_wu = nullptr;
  const uint32_t n_wu = (uint32_t)C.WU.size();
  if (C.n_pub) {  // W_U as the flat entry list of k_verify_scalars_pub: the circuit, same every batch
    std::vector<uint32_t> wu((((size_t)2 * n_wu + 7) & ~(size_t)7) + (size_t)8 * n_wu, 0);
    uint32_t* wv = wu.data() + (((size_t)2 * n_wu + 7) & ~(size_t)7);
    for (uint32_t e = 0; e < n_wu; ++e) {
      wu[2 * e] = C.WU[e].q;
      wu[2 * e + 1] = C.WU[e].col;
      memcpy(wv + 8 * (size_t)e, C.WU[e].valR.v, 32);
    }
    BPP_TRY(ctx_ws(ctx, "vs_wu", wu.size() * 4 + 32, &d_wu));
    BPP_TRY(ctx_h2d_const(ctx, "vs_wu", d_wu, wu.data(), wu.size() * 4));
  }
  {
    ProfScope ps(ctx, "verify_scalars");
    hipLaunchKernelGGL(k_verify_consts, dim3((count + VC_P - 1) / VC_P), dim3(64 * (VC_W + 1)), 0, ctx->stream, count,
                       C.lg, first, seed, d_rec, (uint32_t*)d_kc, NG, C.m, npt, d_sc);
    if (C.deck)
      hipLaunchKernelGGL(k_verify_scalars_deck, dim3(count), dim3(nt), lds + (size_t)nt * 32, ctx->stream, C.n_p, C.m,
                         C.Q, C.lg, d_rec, (const uint32_t*)d_kc, (const uint32_t*)d_cp, (const uint32_t*)d_ce,
                         (const uint32_t*)d_c, (uint32_t*)d_gen, d_sc, NG, npt, (const uint32_t*)d_deck, C.k);
    else if (C.n_pub)
      hipLaunchKernelGGL(split ? k_verify_scalars_pub_tiled : k_verify_scalars_pub, dim3(count), dim3(nt), lds, ctx->stream, C.n_p, C.m, C.Q, C.lg, d_rec,
                         (const uint32_t*)d_kc, (const uint32_t*)d_cp, (const uint32_t*)d_ce, (const uint32_t*)d_c,
                         (uint32_t*)d_gen, d_sc, NG, npt, (const uint32_t*)d_wu, n_wu, d_pub, C.n_pub);
    else
      hipLaunchKernelGGL(split ? k_verify_scalars_tiled : k_verify_scalars, dim3(count), dim3(nt), lds, ctx->stream, C.n_p, C.m, C.Q, C.lg, d_rec,
                         (const uint32_t*)d_kc, (const uint32_t*)d_cp, (const uint32_t*)d_ce, (const uint32_t*)d_c,
                         (uint32_t*)d_gen, d_sc, NG, npt);
    hipLaunchKernelGGL(k_verify_merge, dim3(NG), dim3(POLY_T), 0, ctx->stream, count, NG, (const uint32_t*)d_gen,
                       d_sc);
  }
  return ctx_check_launch(ctx, "k_verify_scalars/merge");
}
