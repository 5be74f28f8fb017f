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
#include "verify_dev.h"
#include "keccak_dev.cuh"
#include "sc25519.cuh"

#define POLY_SLOTS 7  // l1 r0 r1 r3 l2 l3 (Montgomery) per gate
#define POLY_T 256    // lanes per proof; lane i handles gates i, i + POLY_T, ...

// aR^e (Montgomery in, Montgomery out), e < 2^31
FE_INLINE sc sc_pow_small(const sc& aR, uint32_t e, const sc& oneR) {
  sc r = oneR;
  if (!e) return r;
  for (int b = 31 - __clz(e); b >= 0; --b) {
    r = sc_mont(r, r);
    if ((e >> b) & 1u) r = sc_mont(r, aR);
  }
  return r;
}

// Doubling tables in LDS (every lane calls; ends with a barrier).  Table t
// holds N_t >= 1 entries tab[e] = prod over the set bits b of e of f_b
// (Montgomery), from tab[0] = 1 and either tab[1] = x (powers, f_b = x^(2^b);
// pre = false) or every tab[2^b] = f_b written by the caller (pre = true);
// the step for s = 1, 2, 4, ... fills (s, 2s], or (s, 2s) when preloaded, as
// tab[e - s] tab[s] (e - s < s shares no bit with s).  A table costs log2(N)
// dependent multiplies where sc_pow_small spends up to 2 log2(N) on each
// entry, and all tables advance in the same steps.
struct ScTable {
  uint32_t* tab;
  uint32_t N;
  bool pre;
};
FE_INLINE void sc_tables3(const ScTable t0, const ScTable t1, const ScTable t2) {
  constexpr int T = 3;
  const ScTable tb[T] = {t0, t1, t2};
  uint32_t nmax = 0;
  _Pragma("unroll") for (int t = 0; t < T; ++t) nmax = max(nmax, tb[t].N);
  __syncthreads();  // the caller's preloads
  for (uint32_t s = 1; s + 1 < nmax; s <<= 1) {
    uint32_t cnt[T], tot = 0;
    _Pragma("unroll") for (int t = 0; t < T; ++t) {
      const uint32_t hi = min(2 * s - (tb[t].pre ? 1u : 0u), tb[t].N - 1);
      cnt[t] = hi > s ? hi - s : 0;
      tot += cnt[t];
    }
    for (uint32_t u = threadIdx.x; u < tot; u += blockDim.x) {
      uint32_t off = u, t = 0;
      _Pragma("unroll") for (int k = 0; k + 1 < T; ++k) if (t == (uint32_t)k && off >= cnt[k]) {
          off -= cnt[k];
          t = k + 1;
        }
      uint32_t* tab = tb[0].tab;
      _Pragma("unroll") for (int k = 1; k < T; ++k) tab = t == (uint32_t)k ? tb[k].tab : tab;
      const uint32_t e = s + 1 + off;
      sc_store(tab + 8 * e, sc_mont(sc_load(tab + 8 * (e - s)), sc_load(tab + 8 * s)));
    }
    __syncthreads();
  }
}

// Power-table preload (one lane): tab[0] = 1, tab[1] = x
FE_INLINE void sc_table_pow_init(uint32_t* tab, uint32_t N, const sc& xR, const sc& oneR) {
  sc_store(tab, oneR);
  if (N > 1) sc_store(tab + 8, xR);
}

// Gates beyond the first POW_LO: lane tid handles gate i = tid + POW_LO r
// (blockDim = POLY_T = POW_LO whenever n_p > POW_LO), so x^i = tab[tid]
// (x^POW_LO)^r with the second factor kept as a running product
#define POW_LO POLY_T
#define POW_LO_LG 8
static_assert(POW_LO == 1 << POW_LO_LG, "POW_LO");

// Sum over the workgroup of K Montgomery scalars per lane; valid in lane 0.
template <int K>
FE_INLINE void sc_block_sum(sc (&v)[K], uint32_t* lds) {
  _Pragma("unroll") for (int j = 0; j < K; ++j) v[j] = sc_wave_sum(v[j]);
  const uint32_t nw = blockDim.x >> 6, w = threadIdx.x >> 6;
  if (nw == 1) return;
  if ((threadIdx.x & 63u) == 0)
    _Pragma("unroll") for (int j = 0; j < K; ++j) sc_store(lds + (w * K + j) * 8, v[j]);
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t u = 1; u < nw; ++u)
      _Pragma("unroll") for (int j = 0; j < K; ++j) v[j] = sc_add(v[j], sc_load(lds + (u * K + j) * 8));
}

// The row powers as the kernels read them: row_at(zp, q) = z^(q+1), Montgomery.
// SPLIT = false: one LDS table z^0..z^Q (zp = its entry 1).  SPLIT = true
// (large circuits, perm::split_tables_lds): zp[i] = z^i for i < ROW_LO and
// hi[j] = z^(ROW_LO j) for j <= Q >> ROW_LO_LG, z^e = zp[e mod ROW_LO]
// hi[e / ROW_LO] -- one more multiply a read, and Q no longer sets the table's
// size (the y tables' scheme, POW_LO, with the second factor looked up instead
// of carried).  A free function over a plain struct: as a member function the
// same read changed k_verify_scalars' spills.
#define ROW_LO 256
#define ROW_LO_LG 8
static_assert(ROW_LO == 1 << ROW_LO_LG && ROW_LO == perm::kRowLo, "perm::split_tables_lds states ROW_LO");
template <bool SPLIT>
struct RowPow {
  const uint32_t* zp;
  const uint32_t* hi;
};
template <bool SPLIT>
FE_INLINE sc row_at(const RowPow<SPLIT> r, uint32_t q) {
  if constexpr (SPLIT) {
    const uint32_t e = q + 1;
    return sc_mont(sc_load(r.zp + 8 * (e & (ROW_LO - 1))), sc_load(r.hi + 8 * (e >> ROW_LO_LG)));
  } else {
    return sc_load(r.zp + 8 * q);
  }
}
// The split form's second table (every lane calls, after the sc_tables3 that
// built lo; ends with a barrier): hi = the powers of z^ROW_LO = lo[ROW_LO - 1] z
FE_INLINE void row_hi_table(uint32_t* hi, uint32_t NH, const uint32_t* lo, const sc& zR, const sc& oneR) {
  if (threadIdx.x == 0) sc_table_pow_init(hi, NH, sc_mont(sc_load(lo + 8 * (ROW_LO - 1)), zR), oneR);
  sc_tables3({hi, NH, false}, {hi, 1, false}, {hi, 1, false});
}

// sum over the column's entries of z^(q+1) * val (Montgomery)
template <class Rows>
FE_INLINE sc col_sum(const uint32_t* __restrict__ cp, const uint32_t* __restrict__ ce, uint32_t col,
                     const Rows zp) {
  sc acc = sc_zero();
  for (uint32_t e = cp[col]; e < cp[col + 1]; ++e)
    acc = sc_add(acc, sc_mont(row_at(zp, ce[9 * e]), sc_load(ce + 9 * e + 1)));
  return acc;
}

// Column sum split over the whole workgroup (every lane must call it): for
// the few columns with many entries -- W_V's x column holds one entry per
// a_L / a_R row using x (2k + 1 of them), which as one lane's serial chain
// doubled k_poly_coef (126 -> 292 us) and dominated k_verify_scalars.
// Valid in lane 0; `red` is the workgroup-sum scratch.
#define HEAVY_COL 8
template <class Rows>
FE_INLINE sc col_sum_block(const uint32_t* __restrict__ cp, const uint32_t* __restrict__ ce, uint32_t col,
                           const Rows zp, uint32_t* red) {
  sc v[1] = {sc_zero()};
  for (uint32_t e = cp[col] + threadIdx.x; e < cp[col + 1]; e += blockDim.x)
    v[0] = sc_add(v[0], sc_mont(row_at(zp, ce[9 * e]), sc_load(ce + 9 * e + 1)));
  sc_block_sum<1>(v, red);
  __syncthreads();  // red is reused by the next call
  return v[0];
}

// grid = P proofs, block = poly_block(max(n_p, m)); dynamic LDS = (Q + 1 + 2 min(n_p, POW_LO)) * 32 + (POLY_T / 64) * 7 * 32
// t_out[p] = t_1..t_6, <z^Q W_V, gamma_p> (gamma: [P][m] canonical)
#define POLY_NT 7
static_assert(POLY_T == perm::kPolyLanes && POLY_NT == 7, "perm::poly_coef_lds / verify_scalars_lds state these");
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

// ---------------------------------------------------------------------------
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

// ---------------------------------------------------------------------------
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

// The witness of a caller-defined circuit (host/circuit.h; host restatement
// circuit::eval), one proof per workgroup, every workgroup interpreting the
// same program on its own proof's data: prog = the program's device image
// (side_aux [2n], then lc_off, lc_wire, level_off, level_gate, the terms'
// flagged variable ids and their 32-byte-aligned Montgomery coefficients at the
// given word offsets).  The 3n wire values live in LDS in Montgomery form (wire
// id 3h + {0, 1, 2} = l_h, r_h, o_h).  First every gate side, one lane each:
// an aux load, or the part of its combination over {1, v_j, x, u_i} (u_i: the
// proof's public inputs, ids 2 + m_in + i, wires from 2 + m_in + n_pub; a col_sum-style
// term loop up to lc_wire) -- no side waits for another here.  Then the gates
// by dependency level: within a level one lane per gate adds the wire terms of
// both sides and forms the product, then a barrier -- a definition reads wires
// of lower levels only.  A term of coefficient 1 or -1 (the id's flag) adds or
// subtracts its value without a multiply, so a product chain's level is one
// multiply deep.  a_L, a_R, a_O go canonical into their slots of the [P][per]
// array, padding gates zero.  The asserts are evaluated by the same lanes;
// fail[p] = 1 + the first that does not hold, or 0.
//
// A level is a chain of dependent loads (gate index -> term offsets -> ids and
// coefficients -> values) in front of its multiplies; from global memory those
// round trips, not the arithmetic, were the kernel's time (0.38 ms for 384
// proofs of the two-half circuit at 52 cards, 54 levels).  STAGE: the device
// image and the proof's inputs (Montgomery form) are copied into LDS first and
// every level reads them there; taken whenever they fit beside the wires
// (circuit::witness_program_staged_lds), the plain form beyond.
// dynamic LDS = 32 B (the fail word) + 3n x 32 B [+ (m_in + n_pub) x 32 B + the image].
//
// WP_WIDE (k_witness_program_wide; large circuits, more than kLdsMax of wires):
// the 3n wires live in this proof's rows of the global array wide_wires
// ([P][3n][8] words, Montgomery form; "wp_wires", which prove_wipe zeroes),
// program and inputs are read from global memory as in WP_GLOBAL, LDS holds the
// fail word alone.  Phases and barriers are the same.  The wires are written and
// read again by lanes of ONE workgroup across __syncthreads(): its
// workgroup-scope release (the stores have left the wave before the barrier)
// and acquire order them, and a workgroup's waves share their CU's vector L1,
// so no wider scope is needed; each wave also drains its own stores (vmcnt(0))
// before it arrives at such a barrier, which the workgroup-scope release alone
// does not wait for on this target.  The array is reached through a plain pointer --
// neither const nor __restrict__, which would let the compiler keep or hoist a
// load of a wire over the barrier that publishes it.
//
// LATE (the k_witness_program*_late kernels; a circuit with late hints whose
// aux is derived, host restatement circuit::hint_eval_x): the image holds, at
// o_late, 3 words per side -- the op word of the side's late hint
// (circuit::kNoLateHint: none) and its terms [b, e) in the same term tables.
// The free-side pass skips such a side: its slot of aux is never read.  At its
// gate's level (which counts the gates the hint reads) the gate's lane forms w
// with the same term loop, in Montgomery form, applies the op -- INV is
// sc_inv_mont; BIT, NOT_BIT and IS_ZERO turn w canonical, take the bit or the
// zero test with k_hint_aux's selects and shifts, and select 0 or one-in-
// Montgomery-form -- stores the side and forms the product.  As in k_hint_aux,
// branches (a side has a late hint, its op, its term count) and addresses come
// from the program alone, never from a value.  Stores, drains and barriers
// around the wires are those of the kernel without LATE.
enum { WP_GLOBAL = 0, WP_STAGE = 1, WP_WIDE = 2 };
template <int MODE, bool LATE = false>
FE_INLINE void witness_program_body(uint32_t* lds, uint32_t m_in, uint32_t n, uint32_t n_p, uint32_t n_aux, uint32_t A,
                                    uint32_t nlev, uint32_t per, const uint32_t* __restrict__ prog,
                                    uint32_t prog_words, uint32_t o_lc, uint32_t o_wire, uint32_t o_lev, uint32_t o_gate,
                                    uint32_t o_var, uint32_t o_coef, const uint32_t* __restrict__ vals,
                                    const uint32_t* __restrict__ aux, const uint32_t* __restrict__ xs,
                                    uint32_t* __restrict__ sc_out, uint32_t* __restrict__ fail, uint32_t n_pub,
                                    const uint32_t* __restrict__ pubs, uint32_t* wide_wires = nullptr,
                                    uint32_t o_late = 0) {
  constexpr bool STAGE = MODE == WP_STAGE;
  uint32_t* bad = lds;                        // 1 + the first failing assert (8 words kept for alignment)
  uint32_t* wires = lds + 8;                  // [3n] Montgomery
  if constexpr (MODE == WP_WIDE) wires = wide_wires + 8 * 3 * (size_t)n * blockIdx.x;
  uint32_t* vm = wires + 8 * 3 * (size_t)n;   // STAGE: [m_in] inputs, Montgomery
  uint32_t* um = vm + 8 * (size_t)m_in;       // STAGE: [n_pub] public inputs, Montgomery
  uint32_t* image = um + 8 * (size_t)n_pub;   // STAGE: [prog_words] the device image
  const uint32_t p = blockIdx.x, nt = blockDim.x, t = threadIdx.x;
  const uint32_t* vp = vals + 8 * (size_t)p * m_in;
  const uint32_t* up = pubs + 8 * (size_t)p * n_pub;  // (not read when n_pub = 0)
  const uint32_t wbase = 2 + m_in + n_pub;            // the first wire id
  const uint32_t* pg = prog;
  if constexpr (STAGE) {
    for (uint32_t i = t; i < prog_words; i += nt) image[i] = prog[i];
    for (uint32_t j = t; j < m_in; j += nt) sc_store(vm + 8 * (size_t)j, sc_to_mont(sc_load(vp + 8 * (size_t)j)));
    for (uint32_t j = t; j < n_pub; j += nt) sc_store(um + 8 * (size_t)j, sc_to_mont(sc_load(up + 8 * (size_t)j)));
    pg = image;
  }
  const uint32_t *side_aux = pg, *lc_off = pg + o_lc, *lc_wire = pg + o_wire, *lev_off = pg + o_lev,
                 *lev_gate = pg + o_gate, *tvar = pg + o_var, *tcoef = pg + o_coef;
  const sc oneR = sc_one_mont(), xR = sc_to_mont(sc_load(xs + 8 * (size_t)p));
  if (t == 0) *bad = 0xFFFFFFFFu;
  __syncthreads();
  auto input = [&](uint32_t j) {  // v_j, Montgomery
    if constexpr (STAGE) return sc_load(vm + 8 * (size_t)j);
    return sc_to_mont(sc_load(vp + 8 * (size_t)j));
  };
  auto pub_in = [&](uint32_t j) {  // u_j, Montgomery
    if constexpr (STAGE) return sc_load(um + 8 * (size_t)j);
    return sc_to_mont(sc_load(up + 8 * (size_t)j));
  };
  auto terms = [&](sc acc, uint32_t b, uint32_t e_end) {  // acc + terms [b, e_end), Montgomery
    for (uint32_t e = b; e < e_end; ++e) {
      const uint32_t tv = tvar[e], var = tv & circuit::kTermVar;
      const sc val = var == 0 ? oneR
                              : var <= m_in ? input(var - 1)
                                            : var == m_in + 1 ? xR
                                            : var < wbase     ? pub_in(var - 2 - m_in)
                                                              : sc_load(wires + 8 * (size_t)(var - wbase));
      if (tv & circuit::kTermOne)
        acc = sc_add(acc, val);
      else if (tv & circuit::kTermNeg)
        acc = sc_sub(acc, val);
      else
        acc = sc_add(acc, sc_mont(val, sc_load(tcoef + 8 * (size_t)e)));
    }
    return acc;
  };
  [[maybe_unused]] const uint32_t* late = pg + o_late;  // LATE: [2n][3] op word, terms [b, e)
  [[maybe_unused]] auto late_value = [&](uint32_t opw, const sc& w) {  // op(w), Montgomery in and out
    const uint32_t op = opw & 0xFFu, arg = opw >> 8;
    if (op == circuit::kHintValue) return w;
    if (op == circuit::kHintInv) return sc_inv_mont(w);
    const sc c = sc_from_mont(w);
    uint32_t word = 0, nz = 0;
    _Pragma("unroll") for (uint32_t k = 0; k < 8; ++k) {
      word = k == (arg >> 5) ? c.v[k] : word;  // (arg: the program's, the same for a hint's every proof)
      nz |= c.v[k];
    }
    const uint32_t bit = (word >> (arg & 31u)) & 1u;
    const uint32_t b = op == circuit::kHintBit ? bit : op == circuit::kHintNotBit ? 1u - bit : (uint32_t)(nz == 0);
    sc r;
    _Pragma("unroll") for (uint32_t k = 0; k < 8; ++k) r.v[k] = oneR.v[k] & (0u - b);
    return r;
  };
  for (uint32_t u = t; u < 2 * n; u += nt) {  // side u = 2g + s
    const uint32_t a = side_aux[u];
    if constexpr (LATE)
      if (late[3 * u] != circuit::kNoLateHint) continue;  // (evaluated at its gate's level)
    const sc v = a == 0xFFFFFFFFu ? terms(sc_zero(), lc_off[u], lc_wire[u])
                                  : sc_to_mont(sc_load(aux + 8 * ((size_t)p * n_aux + a)));
    sc_store(wires + 8 * (3 * (size_t)(u >> 1) + (u & 1u)), v);
  }
  if constexpr (MODE == WP_WIDE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the wires' stores, below)
  __syncthreads();
  for (uint32_t lev = 0; lev < nlev; ++lev) {
    for (uint32_t u = lev_off[lev] + t; u < lev_off[lev + 1]; u += nt) {
      const uint32_t g = lev_gate[u];
      if constexpr (LATE) {
        // one rolled copy of the side code (the inverse's loop is in it); a side
        // is finished in its wire slot and the product reads both slots back, so
        // no side is kept in an indexed array (which the rolled loop would put
        // in scratch)
        _Pragma("nounroll") for (uint32_t s = 0; s < 2; ++s) {
          const uint32_t i = 2 * g + s, wb = lc_wire[i], we = lc_off[i + 1], opw = late[3 * i];
          uint32_t* slot = wires + 8 * (3 * (size_t)g + s);
          if (opw != circuit::kNoLateHint)  // (the program's word: the same branch for every proof)
            sc_store(slot, late_value(opw, terms(sc_zero(), late[3 * i + 1], late[3 * i + 2])));
          else if (wb < we)
            sc_store(slot, terms(sc_load(slot), wb, we));
        }
        sc_store(wires + 8 * (3 * (size_t)g + 2),
                 sc_mont(sc_load(wires + 8 * (3 * (size_t)g)), sc_load(wires + 8 * (3 * (size_t)g + 1))));
        continue;
      }
      sc side[2];
      _Pragma("unroll") for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t i = 2 * g + s, wb = lc_wire[i], we = lc_off[i + 1];
        side[s] = sc_load(wires + 8 * (3 * (size_t)g + s));
        if (wb < we) {  // (a free side's combination is empty)
          side[s] = terms(side[s], wb, we);
          sc_store(wires + 8 * (3 * (size_t)g + s), side[s]);
        }
      }
      sc_store(wires + 8 * (3 * (size_t)g + 2), sc_mont(side[0], side[1]));
    }
    if constexpr (MODE == WP_WIDE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  uint32_t* o = sc_out + 8 * (size_t)p * per;
  for (uint32_t g = t; g < n_p; g += nt) {
    sc w[3] = {sc_zero(), sc_zero(), sc_zero()};
    if (g < n)
      _Pragma("unroll") for (uint32_t s = 0; s < 3; ++s) w[s] = sc_from_mont(sc_load(wires + 8 * (3 * (size_t)g + s)));
    sc_store(o + 8 * (1 + g), w[0]);
    sc_store(o + 8 * (1 + n_p + g), w[1]);
    sc_store(o + 8 * (2 + 2 * n_p + g), w[2]);
  }
  for (uint32_t a = t; a < A; a += nt) {
    const sc r = sc_from_mont(terms(sc_zero(), lc_off[2 * n + a], lc_off[2 * n + a + 1]));
    uint32_t nz = 0;
    _Pragma("unroll") for (int i = 0; i < 8; ++i) nz |= r.v[i];
    if (nz) atomicMin(bad, a + 1);
  }
  __syncthreads();
  if (t == 0) fail[p] = *bad == 0xFFFFFFFFu ? 0u : *bad;
}

#define WITNESS_PROGRAM_ARGS                                                                                         \
  uint32_t m_in, uint32_t n, uint32_t n_p, uint32_t n_aux, uint32_t A, uint32_t nlev, uint32_t per,                  \
      const uint32_t *__restrict__ prog, uint32_t prog_words, uint32_t o_lc, uint32_t o_wire, uint32_t o_lev,       \
      uint32_t o_gate, uint32_t o_var, uint32_t o_coef, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ aux,         \
      const uint32_t *__restrict__ xs, uint32_t *__restrict__ sc_out, uint32_t *__restrict__ fail, uint32_t n_pub,   \
      const uint32_t *__restrict__ pubs
#define WITNESS_PROGRAM_PASS \
  m_in, n, n_p, n_aux, A, nlev, per, prog, prog_words, o_lc, o_wire, o_lev, o_gate, o_var, o_coef, vals, aux, xs, \
      sc_out, fail, n_pub, pubs
__global__ void __launch_bounds__(256) k_witness_program(WITNESS_PROGRAM_ARGS) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_program_body<WP_STAGE>(lds, WITNESS_PROGRAM_PASS);
}
// the plain form: program and inputs read from global memory
__global__ void __launch_bounds__(256) k_witness_program_global(WITNESS_PROGRAM_ARGS) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_program_body<WP_GLOBAL>(lds, WITNESS_PROGRAM_PASS);
}
// the wide form: the wires in global memory too (wires: [P][3n][8] words)
__global__ void __launch_bounds__(256) k_witness_program_wide(WITNESS_PROGRAM_ARGS, uint32_t* wires) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_program_body<WP_WIDE>(lds, WITNESS_PROGRAM_PASS, wires);
}

// the same three for a circuit with late hints (LATE above)
__global__ void __launch_bounds__(256) k_witness_program_late(WITNESS_PROGRAM_ARGS, uint32_t o_late) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_program_body<WP_STAGE, true>(lds, WITNESS_PROGRAM_PASS, nullptr, o_late);
}
__global__ void __launch_bounds__(256) k_witness_program_global_late(WITNESS_PROGRAM_ARGS, uint32_t o_late) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_program_body<WP_GLOBAL, true>(lds, WITNESS_PROGRAM_PASS, nullptr, o_late);
}
__global__ void __launch_bounds__(256) k_witness_program_wide_late(WITNESS_PROGRAM_ARGS, uint32_t* wires,
                                                                   uint32_t o_late) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  witness_program_body<WP_WIDE, true>(lds, WITNESS_PROGRAM_PASS, wires, o_late);
}

int witness_program_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_vals,
                        const uint32_t* d_aux, const uint32_t* d_x, uint32_t per, uint32_t* d_sc, uint32_t* fail,
                        const uint32_t* d_pub, bool derive_late) {
  if (!P) return BPP_OK;
  const circuit::Program& G = *C.program;
  if (G.n_pub && !d_pub) return BPP_ERR_ARG;
  // by size and flag: the wires in global memory (large circuits, or TILED),
  // else in LDS with the program staged beside them while that fits
  const bool wide = circuit::witness_wide(C);
  const bool late = derive_late && circuit::has_late_hints(G);  // (its own kernels: the hints evaluated at their gates)
  const bool stage = !wide && circuit::witness_program_staged_lds(G) <= perm::kLdsMax;
  const size_t lds = wide    ? circuit::witness_program_wide_lds()
                     : stage ? circuit::witness_program_staged_lds(G)
                             : circuit::witness_program_lds(G.n);
  void *d_prog = nullptr, *d_wires = nullptr;
  if (wide) BPP_TRY(ctx_ws(ctx, "wp_wires", (size_t)P * 3 * G.n * 32, &d_wires));  // (witness data: prove_wipe)
  BPP_TRY(ctx_ws(ctx, "wp_prog", G.dev.size() * 4, &d_prog));
  BPP_TRY(ctx_h2d_const(ctx, "wp_prog", d_prog, G.dev.data(), G.dev.size() * 4));  // the circuit: same every batch
  // whole waves, no more lanes than the padded gates (narrow levels leave the
  // rest waiting at the barriers)
  const unsigned nt = std::min<unsigned>(256, std::max<unsigned>(64, (C.n_p + 63) & ~63u));
  {
    ProfScope ps(ctx, "witness_program");
#define WITNESS_PROGRAM_LAUNCH                                                                                      \
  G.m_in, G.n, C.n_p, G.n_aux, G.A, (uint32_t)G.level_off.size() - 1, per, (const uint32_t*)d_prog,                \
      (uint32_t)G.dev.size(), G.dev_lc_off, G.dev_lc_wire, G.dev_level_off, G.dev_level_gate, G.dev_vars, G.dev_coefs, \
      d_vals, d_aux, d_x, d_sc, fail, G.n_pub, d_pub
    if (late && wide)
      hipLaunchKernelGGL(k_witness_program_wide_late, dim3(P), dim3(nt), lds, ctx->stream, WITNESS_PROGRAM_LAUNCH,
                         (uint32_t*)d_wires, G.dev_late);
    else if (late)
      hipLaunchKernelGGL(stage ? k_witness_program_late : k_witness_program_global_late, dim3(P), dim3(nt), lds,
                         ctx->stream, WITNESS_PROGRAM_LAUNCH, G.dev_late);
    else if (wide)
      hipLaunchKernelGGL(k_witness_program_wide, dim3(P), dim3(nt), lds, ctx->stream, WITNESS_PROGRAM_LAUNCH,
                         (uint32_t*)d_wires);
    else
      hipLaunchKernelGGL(stage ? k_witness_program : k_witness_program_global, dim3(P), dim3(nt), lds, ctx->stream,
                         WITNESS_PROGRAM_LAUNCH);
  }
  const char* const plain = wide ? "k_witness_program_wide" : stage ? "k_witness_program" : "k_witness_program_global";
  const char* const lated = wide    ? "k_witness_program_wide_late"
                            : stage ? "k_witness_program_late"
                                    : "k_witness_program_global_late";
  return ctx_check_launch(ctx, late ? lated : plain);
}

// k_hint_aux: the auxiliary values of a circuit with hints, in front of
// k_witness_program.  One lane per (proof, hint): blockIdx.y = the proof, lane
// i of the row takes record i of the hints' device image (circuit::Hints::dev:
// the hint's index t, its op word, its terms [b, e)), whose order groups the
// hints by op, so the lanes of a wave run one op wherever the counts allow.
// w = the combination over {1, v_j, u_i}, accumulated CANONICAL: a term of
// coefficient 1 or -1 (the id's flag) adds or subtracts the canonical value, and
// a general term is sc_mont(value, coefficient R) = value x coefficient, so a
// BIT lane over v_j runs no product at all.  aux_t = op(w), canonical, to
// aux[p][t].  Branches (the op, the term flags, the term count, the exponent of
// sc_inv_mont) and addresses (t, the variable ids) come from the hint program
// alone; the value is tested and its bit taken with selects and shifts.  No LDS.
__global__ void __launch_bounds__(256) k_hint_aux(uint32_t n_aux, uint32_t m_in, uint32_t n_pub,
                                                  const uint32_t* __restrict__ prog, uint32_t o_var, uint32_t o_coef,
                                                  const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pubs,
                                                  uint32_t* __restrict__ aux) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
  if (i >= n_aux) return;
  const uint4 rec = reinterpret_cast<const uint4*>(prog)[i];  // t, op | arg << 8, b, e
  const uint32_t* vp = vals + 8 * (size_t)p * m_in;
  const uint32_t* up = pubs + 8 * (size_t)p * n_pub;  // (not read when n_pub = 0)
  sc one = sc_zero();
  one.v[0] = 1;
  sc w = sc_zero();
  for (uint32_t e = rec.z; e < rec.w; ++e) {
    const uint32_t tv = prog[o_var + e], var = tv & circuit::kTermVar;
    const sc val = var == 0 ? one : sc_load(var <= m_in ? vp + 8 * (size_t)(var - 1) : up + 8 * (size_t)(var - 2 - m_in));
    if (tv & circuit::kTermOne)
      w = sc_add(w, val);
    else if (tv & circuit::kTermNeg)
      w = sc_sub(w, val);
    else
      w = sc_add(w, sc_mont(val, sc_load(prog + o_coef + 8 * (size_t)e)));
  }
  const uint32_t op = rec.y & 0xFFu, arg = rec.y >> 8;
  sc r = w;  // (circuit::kHintValue)
  if (op == circuit::kHintInv) {
    r = sc_from_mont(sc_inv_mont(sc_to_mont(w)));
  } else if (op != circuit::kHintValue) {
    uint32_t word = 0, nz = 0;
    _Pragma("unroll") for (uint32_t k = 0; k < 8; ++k) {
      word = k == (arg >> 5) ? w.v[k] : word;  // (arg: the program's, the same for a hint's every proof)
      nz |= w.v[k];
    }
    const uint32_t bit = (word >> (arg & 31u)) & 1u;
    r = sc_zero();
    r.v[0] = op == circuit::kHintBit ? bit : op == circuit::kHintNotBit ? 1u - bit : (uint32_t)(nz == 0);
  }
  sc_store(aux + 8 * ((size_t)p * n_aux + rec.x), r);
}

int hint_aux_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_vals, const uint32_t* d_pub,
                 uint32_t* d_aux) {
  const circuit::Program& G = *C.program;
  if (!G.hints || (G.n_pub && !d_pub)) return BPP_ERR_ARG;
  if (!P || !G.n_aux) return BPP_OK;
  const circuit::Hints& H = *G.hints;
  void* d_prog = nullptr;
  BPP_TRY(ctx_ws(ctx, "ha_prog", H.dev.size() * 4, &d_prog));
  BPP_TRY(ctx_h2d_const(ctx, "ha_prog", d_prog, H.dev.data(), H.dev.size() * 4));  // the circuit: same every batch
  {
    ProfScope ps(ctx, "hint_aux");
    constexpr uint32_t kRows = 65535;  // (gridDim.y's bound)
    for (uint32_t p0 = 0; p0 < P; p0 += kRows)
      hipLaunchKernelGGL(k_hint_aux, dim3((G.n_aux + 255) / 256, std::min(kRows, P - p0)), dim3(256), 0, ctx->stream,
                         G.n_aux, G.m_in, G.n_pub, (const uint32_t*)d_prog, H.dev_vars, H.dev_coefs,
                         d_vals + 8 * (size_t)p0 * G.m_in, d_pub ? d_pub + 8 * (size_t)p0 * G.n_pub : nullptr,
                         d_aux + 8 * (size_t)p0 * G.n_aux);
  }
  return ctx_check_launch(ctx, "k_hint_aux");
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


namespace {

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

}  // namespace

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
