// k_poly_coef's definition, included by poly.hip once per kernel with
//   POLY_COEF_KERNEL  the kernel's name
//   POLY_COEF_SPLIT   false: the row table z^0..z^Q in LDS (k_poly_coef);
//                     true: the table in two (RowPow; k_poly_coef_tiled, large
//                     circuits), dynamic LDS = perm::split_tables_lds(Q, n_p, 7)
// The text is included, not called: a kernel whose body is an inlined function
// loses the __restrict__ of its own arguments to scoped metadata, and
// k_poly_coef with the flag off must stay the kernel it was (same registers and
// spills).
__global__ void __launch_bounds__(POLY_T) POLY_COEF_KERNEL(uint32_t n_p, uint32_t m, uint32_t Q, uint32_t per,
                                                         const uint32_t* __restrict__ sc_in,
                                                         const uint32_t* __restrict__ ch,
                                                         const uint32_t* __restrict__ cp,
                                                         const uint32_t* __restrict__ ce,
                                                         const uint32_t* __restrict__ gamma,
                                                         uint32_t* __restrict__ vec, uint32_t* __restrict__ hf,
                                                         uint32_t* __restrict__ t_out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr bool SPLIT = POLY_COEF_SPLIT;
  const uint32_t NY = min(n_p, (uint32_t)POW_LO);
  const uint32_t NZ = SPLIT ? (uint32_t)ROW_LO : Q + 1, NH = SPLIT ? (Q >> ROW_LO_LG) + 1 : 0u;
  uint32_t* zt = lds;               // [Q + 1] z^e; SPLIT: [ROW_LO] z^i
  uint32_t* zh = zt + 8 * NZ;       // SPLIT: [NH] z^(ROW_LO j)
  uint32_t* yt = zh + 8 * NH;       // [NY] y^i
  uint32_t* yit = yt + 8 * NY;      // [NY] y^-i
  uint32_t* red = yit + 8 * NY;     // reduction scratch
  const RowPow<SPLIT> zp = {SPLIT ? zt : zt + 8, zh};  // z^(q+1)
  const uint32_t p = blockIdx.x;
  const sc oneR = sc_one_mont();
  const sc yR = sc_to_mont(sc_load(ch + 24 * p)), yiR = sc_to_mont(sc_load(ch + 24 * p + 8)),
           zR = sc_to_mont(sc_load(ch + 24 * p + 16));
  if (threadIdx.x == 0) {
    sc_table_pow_init(zt, NZ, zR, oneR);
    sc_table_pow_init(yt, NY, yR, oneR);
    sc_table_pow_init(yit, NY, yiR, oneR);
  }
  sc_tables3({zt, NZ, false}, {yt, NY, false}, {yit, NY, false});
  if constexpr (SPLIT) row_hi_table(zh, NH, zt, zR, oneR);
  sc yhi = oneR, yihi = oneR, ystep = oneR, yistep = oneR;  // (y^POW_LO)^r
  if (n_p > POW_LO) {
    ystep = sc_mont(sc_load(yt + 8 * (POW_LO - 1)), yR);
    yistep = sc_mont(sc_load(yit + 8 * (POW_LO - 1)), yiR);
  }
  sc t[POLY_NT];
  _Pragma("unroll") for (int j = 0; j < POLY_NT; ++j) t[j] = sc_zero();
  for (uint32_t i = threadIdx.x; i < n_p; i += blockDim.x) {
    const uint32_t* s = sc_in + (size_t)p * per * 8;
    const sc aL = sc_to_mont(sc_load(s + 8 * (1 + i)));
    const sc aR = sc_to_mont(sc_load(s + 8 * (1 + n_p + i)));
    const sc l2 = sc_to_mont(sc_load(s + 8 * (2 + 2 * n_p + i)));  // a_O
    const sc l3 = sc_to_mont(sc_load(s + 8 * (3 + 3 * n_p + i)));  // s_L
    const sc sR = sc_to_mont(sc_load(s + 8 * (3 + 4 * n_p + i)));
    sc yp = sc_load(yt + 8 * (i % POW_LO)), yip = sc_load(yit + 8 * (i % POW_LO));
    if (i >= POW_LO) {
      yp = sc_mont(yp, yhi);
      yip = sc_mont(yip, yihi);
    }
    if (n_p > POW_LO) {
      yhi = sc_mont(yhi, ystep);
      yihi = sc_mont(yihi, yistep);
    }
    const sc zWL = col_sum(cp, ce, i, zp), zWR = col_sum(cp + (n_p + 1), ce, i, zp),
             zWO = col_sum(cp + 2 * (n_p + 1), ce, i, zp);
    const sc l1 = sc_add(aL, sc_mont(zWR, yip));
    const sc r0 = sc_sub(zWO, yp);
    const sc r1 = sc_add(sc_mont(aR, yp), zWL);
    const sc r3 = sc_mont(sR, yp);
    t[0] = sc_add(t[0], sc_mont(l1, r0));
    t[1] = sc_add(t[1], sc_add(sc_mont(l1, r1), sc_mont(l2, r0)));
    t[2] = sc_add(t[2], sc_add(sc_mont(l2, r1), sc_mont(l3, r0)));
    t[3] = sc_add(t[3], sc_add(sc_mont(l1, r3), sc_mont(l3, r1)));
    t[4] = sc_add(t[4], sc_mont(l2, r3));
    t[5] = sc_add(t[5], sc_mont(l3, r3));
    uint32_t* v = vec + ((size_t)p * n_p + i) * POLY_SLOTS * 8;
    sc_store(v + 0, l1);
    sc_store(v + 8, r0);
    sc_store(v + 16, r1);
    sc_store(v + 24, r3);
    sc_store(v + 32, l2);
    sc_store(v + 40, l3);
    sc_store(hf + ((size_t)p * n_p + i) * 8, sc_from_mont(yip));  // H factors y^-i
  }
  // tau_x's <z^Q W_V, gamma>: V column j of the fourth CSR block (Montgomery)
  // times gamma_j (canonical) is canonical z^Q W_V[j] gamma_j; to_mont keeps
  // the sum in the Montgomery domain of the other six
  const uint32_t* cpv = cp + 3 * (n_p + 1);
  const uint32_t* gam = gamma + 8 * (size_t)p * m;
  for (uint32_t j = threadIdx.x; j < m; j += blockDim.x)
    if (cpv[j + 1] - cpv[j] <= HEAVY_COL) t[6] = sc_add(t[6], sc_mont(col_sum(cpv, ce, j, zp), sc_to_mont(sc_load(gam + 8 * j))));
  const uint32_t* heavy = cpv + m + 1;  // [count, columns...] (build_csr)
  for (uint32_t h = 0; h < heavy[0]; ++h) {
    const uint32_t j = heavy[1 + h];
    const sc cs = col_sum_block(cpv, ce, j, zp, red);
    if (threadIdx.x == 0) t[6] = sc_add(t[6], sc_mont(cs, sc_to_mont(sc_load(gam + 8 * j))));
  }
  sc_block_sum<POLY_NT>(t, red);
  if (threadIdx.x == 0)
    _Pragma("unroll") for (int j = 0; j < POLY_NT; ++j) sc_store(t_out + (POLY_NT * p + j) * 8, sc_from_mont(t[j]));
}
#undef POLY_COEF_KERNEL
#undef POLY_COEF_SPLIT
