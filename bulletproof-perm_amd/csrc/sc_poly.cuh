// Device helpers shared by the prover's polynomial kernels (poly.hip) and the
// verifier's scalar kernels (verify_scalars.hip): the lane layout of a proof's
// workgroup, the LDS power tables, the row powers z^(q+1) and the column sums
// of the circuit matrices' column-CSR (build_csr, poly.h).
#pragma once
#include "host/perm.h"
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

// t_1..t_6 and <z^Q W_V, gamma>: the sums a proof's k_poly_coef workgroup reduces
#define POLY_NT 7
static_assert(POLY_T == perm::kPolyLanes && POLY_NT == 7, "perm::poly_coef_lds / verify_scalars_lds state these");
