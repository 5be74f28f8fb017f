// Device helpers the re-shuffle kernels share (reshuffle.hip: k_rs_*, the blind
// re-shuffle's, and k_mrs_*, the masked one's): small scalar steps, the masked
// select, and the constant-time scalar-times-point walk.
#pragma once
#include "ge_io.cuh"
#include "sc25519.cuh"

FE_INLINE sc sc_from_u32(uint32_t v) {
  sc r = sc_zero();
  r.v[0] = v;
  return r;
}
// a b for canonical a, b
FE_INLINE sc sc_mul(const sc& a, const sc& b) { return sc_mont(sc_to_mont(a), b); }
// x^e in Montgomery form from x in Montgomery form, e >= 1 (e is public: a
// card's index)
FE_INLINE sc sc_pow_mont(const sc& xR, uint32_t e) {
  sc r = xR;
  for (int i = 30 - __builtin_clz(e); i >= 0; --i) {
    r = sc_mont(r, r);
    if ((e >> i) & 1u) r = sc_mont(r, xR);
  }
  return r;
}

// take_b ? b : a, limb by limb under a mask: no branch on the (secret) bit
FE_INLINE fe fe_select(const fe& a, const fe& b, uint32_t mask) {
  fe r;
  _Pragma("unroll") for (int i = 0; i < FE_LIMBS; ++i) r.v[i] = a.v[i] ^ ((a.v[i] ^ b.v[i]) & mask);
  return r;
}
FE_INLINE ge_p3 ge_select(const ge_p3& a, const ge_p3& b, uint32_t take_b) {
  const uint32_t mask = 0u - take_b;
  ge_p3 r;
  r.X = fe_select(a.X, b.X, mask);
  r.Y = fe_select(a.Y, b.Y, mask);
  r.Z = fe_select(a.Z, b.Z, mask);
  r.T = fe_select(a.T, b.T, mask);
  return r;
}

// One bit of the constant-time scalar-times-point walk, double-and-add-always:
// a doubling, an addition and a select, the same instructions and the same
// addresses whatever the (secret) bit is.
FE_INLINE ge_p3 ge_ct_step(const ge_p3& acc, const ge_niels& A, uint32_t bit) {
  const ge_p3 d = ge_dbl(acc);
  return ge_select(d, ge_madd(d, A), bit);
}

// s A for a secret canonical scalar s (8 words in memory): 253 such steps (as
// pedersen_dev's walk is for its scalars).  s is read a word per 32 bits: no
// register array indexed by the bit.
FE_INLINE ge_p3 ge_ct_mul(const uint32_t* s, const ge_niels& A) {
  ge_p3 acc = ge_identity();
  _Pragma("nounroll") for (int bit = 252; bit >= 0; --bit) acc = ge_ct_step(acc, A, (s[bit >> 5] >> (bit & 31)) & 1u);
  return acc;
}
