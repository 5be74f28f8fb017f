// Device arithmetic probe: calls the product's own field, scalar, point and
// digit-recoding functions (the csrc/ headers, nothing re-implemented) one
// lane per case, on raw limbs, so that tests can drive them at the bounds
// their contracts state (tests/test_gpu_arith_*.py).
//
// Built into bpperm/libbpperm_probe.so by build.py build_probe(); it is not
// part of libbpperm.so or its ABI and nothing in the product loads it.
//
// Every entry point takes HOST pointers, allocates its device buffers on
// device 0, copies in, launches, copies out and frees; it returns the HIP
// error code (0 = success, and 0 at once for n == 0).  Layouts: 10 words per
// field element, 8 per scalar, the 40-word P3 and 32-word Niels rows of
// ge_io.cuh.  Blocks are 64 lanes and every launched wave is fully active:
// lanes past the last case recompute case 0 and store nothing (sc_wave_sum,
// sc_shfl and ge_add_quad exchange data between lanes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc/dt_walk.cuh"
#include "../csrc/ge25519.cuh"
#include "../csrc/ge_io.cuh"
#include "../csrc/msm_kernels.cuh"
#include "../csrc/sc25519.cuh"

#define PROBE_T 64

// ------------------------------------------------------------------ field
enum {
  FE_OP_CARRY = 0, FE_OP_ADD, FE_OP_SUB, FE_OP_NEG, FE_OP_ADD_NC, FE_OP_SUB_NC, FE_OP_MUL, FE_OP_SQ, FE_OP_MUL_SMALL,
  FE_OP_CANON, FE_OP_PRED, FE_OP_ABS, FE_OP_INVERT, FE_OP_POW22523, FE_OP_LOAD_WORDS, FE_OP_STORE_WORDS,
  FE_OP_WORDS_CANONICAL, FE_OP_SQRT_RATIO_M1, FE_OP_COUNT
};
#define FE_OUT_WORDS 12

FE_INLINE fe probe_load_fe(const uint32_t* p) {
  fe r;
  _Pragma("unroll") for (int i = 0; i < FE_LIMBS; ++i) r.v[i] = p[i];
  return r;
}
FE_INLINE void probe_store_fe(uint32_t* p, const fe& a) {
  _Pragma("unroll") for (int i = 0; i < FE_LIMBS; ++i) p[i] = a.v[i];
}

// a, b: n x 10 words (word-input ops read the first 8 of a; fe_mul_small's k
// is b[0]); out: n x FE_OUT_WORDS, zero-filled by the host first.
__global__ void __launch_bounds__(PROBE_T) k_probe_fe(uint32_t op, const uint32_t* __restrict__ a,
                                                      const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                                                      uint32_t n) {
  const uint32_t t = blockIdx.x * PROBE_T + threadIdx.x;
  const uint32_t i = t < n ? t : 0;
  const fe x = probe_load_fe(a + 10 * (size_t)i), y = probe_load_fe(b + 10 * (size_t)i);
  uint32_t w[8];
  _Pragma("unroll") for (int k = 0; k < 8; ++k) w[k] = a[10 * (size_t)i + k];
  uint32_t o[FE_OUT_WORDS];
  _Pragma("unroll") for (int k = 0; k < FE_OUT_WORDS; ++k) o[k] = 0;
  fe r = fe_zero();
  bool has_r = true;
  switch (op) {
    case FE_OP_CARRY: r = fe_carry(x); break;
    case FE_OP_ADD: r = fe_add(x, y); break;
    case FE_OP_SUB: r = fe_sub(x, y); break;
    case FE_OP_NEG: r = fe_neg(x); break;
    case FE_OP_ADD_NC: r = fe_add_nc(x, y); break;
    case FE_OP_SUB_NC: r = fe_sub_nc(x, y); break;
    case FE_OP_MUL: r = fe_mul(x, y); break;
    case FE_OP_SQ: r = fe_sq(x); break;
    case FE_OP_MUL_SMALL: r = fe_mul_small(x, y.v[0]); break;
    case FE_OP_CANON: r = fe_canon(x); break;
    case FE_OP_PRED:
      has_r = false;
      o[0] = fe_iszero(x);
      o[1] = fe_isneg(x);
      o[2] = fe_eq(x, y);
      break;
    case FE_OP_ABS: r = fe_abs(x); break;
    case FE_OP_INVERT: r = fe_invert(x); break;
    case FE_OP_POW22523: r = fe_pow22523(x); break;
    case FE_OP_LOAD_WORDS: r = fe_load_words(w); break;
    case FE_OP_STORE_WORDS:
      has_r = false;
      fe_store_words(o, x);
      break;
    case FE_OP_WORDS_CANONICAL:
      has_r = false;
      o[0] = fe_words_canonical(w);
      break;
    case FE_OP_SQRT_RATIO_M1:
      has_r = false;
      o[0] = fe_sqrt_ratio_m1(x, y, r);
      probe_store_fe(o + 1, r);
      break;
    default: break;
  }
  if (has_r) probe_store_fe(o, r);
  if (t < n) {
    _Pragma("unroll") for (int k = 0; k < FE_OUT_WORDS; ++k) out[FE_OUT_WORDS * (size_t)t + k] = o[k];
  }
}

// ----------------------------------------------------------------- scalar
enum {
  SC_OP_ADD = 0, SC_OP_SUB, SC_OP_NEG, SC_OP_MONT, SC_OP_MONT_CIOS, SC_OP_TO_MONT, SC_OP_FROM_MONT, SC_OP_HALF,
  SC_OP_REDUCE256, SC_OP_FROM_WIDE, SC_OP_WAVE_SUM, SC_OP_SHFL, SC_OP_COUNT
};

// a, b, out: n x 8 words.  SC_OP_FROM_WIDE reads a (low 256 bits) and b (high);
// SC_OP_WAVE_SUM leaves the sum of a wave's 64 cases in its lane 0 (the other
// lanes' outputs are sc_wave_sum's unspecified partial sums); SC_OP_SHFL
// gives every lane the a of lane b[0] & 63 of its wave.
__global__ void __launch_bounds__(PROBE_T) k_probe_sc(uint32_t op, const uint32_t* __restrict__ a,
                                                      const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                                                      uint32_t n) {
  const uint32_t t = blockIdx.x * PROBE_T + threadIdx.x;
  const uint32_t i = t < n ? t : 0;
  const sc x = sc_load(a + 8 * (size_t)i), y = sc_load(b + 8 * (size_t)i);
  sc r = sc_zero();
  switch (op) {
    case SC_OP_ADD: r = sc_add(x, y); break;
    case SC_OP_SUB: r = sc_sub(x, y); break;
    case SC_OP_NEG: r = sc_neg(x); break;
    case SC_OP_MONT: r = sc_mont(x, y); break;
    case SC_OP_MONT_CIOS: r = sc_mont_cios(x, y); break;
    case SC_OP_TO_MONT: r = sc_to_mont(x); break;
    case SC_OP_FROM_MONT: r = sc_from_mont(x); break;
    case SC_OP_HALF: r = sc_half(x); break;
    case SC_OP_REDUCE256: r = sc_reduce256(x.v); break;
    case SC_OP_FROM_WIDE: {
      uint32_t w[16];
      _Pragma("unroll") for (int k = 0; k < 8; ++k) {
        w[k] = x.v[k];
        w[8 + k] = y.v[k];
      }
      r = sc_from_wide_w(w);
      break;
    }
    case SC_OP_WAVE_SUM: r = sc_wave_sum(x); break;  // op is uniform: the whole wave is here
    case SC_OP_SHFL: r = sc_shfl(x, (int)(y.v[0] & 63u)); break;
    default: break;
  }
  if (t < n) sc_store(out + 8 * (size_t)t, r);
}

// ------------------------------------------------------------------ point
enum {
  GE_OP_MADD = 0, GE_OP_MSUB, GE_OP_MADD_SIGNED, GE_OP_MADD_FG, GE_OP_MADD_H1H2, GE_OP_ADD, GE_OP_ADD_QUAD, GE_OP_DBL,
  GE_OP_NEG, GE_OP_NIELS_FROM_AFFINE, GE_OP_TO_NIELS, GE_OP_FROM_NIELS, GE_OP_ENCODE, GE_OP_DECODE, GE_OP_EQ,
  GE_OP_ELLIGATOR, GE_OP_COUNT
};
#define GE_AUX_WORDS 32

// p, q: n x 40 (P3 rows); nl: n x 32 (Niels rows; GE_OP_DECODE reads words
// 0..7 of a row as the encoding); flag: n words (the sign of the signed
// additions); out: n x 40; aux: n x 32 (Niels results, encodings, booleans).
// GE_OP_MADD_FG fetches its operand with the product's fetch_entry_sw (entry
// = row | sign << 31), swap included.  GE_OP_ADD_QUAD runs four lanes per
// case (lanes = 4 n, rounded up to whole waves): lane c writes coordinate c.
__global__ void __launch_bounds__(PROBE_T) k_probe_ge(uint32_t op, const uint32_t* __restrict__ p,
                                                      const uint32_t* __restrict__ q,
                                                      const uint32_t* __restrict__ nl,
                                                      const uint32_t* __restrict__ flag, uint32_t* __restrict__ out,
                                                      uint32_t* __restrict__ aux, uint32_t n) {
  const uint32_t t = blockIdx.x * PROBE_T + threadIdx.x;
  const bool quad = op == GE_OP_ADD_QUAD;
  const uint32_t cs = quad ? t >> 2 : t;  // case of this lane
  const bool live = cs < n;
  const uint32_t i = live ? cs : 0;
  const ge_p3 P = load_p3(p, i), Q = load_p3(q, i);
  const ge_niels N = load_niels(nl, i);
  const bool neg = flag[i] != 0;
  ge_p3 r = ge_identity();
  ge_niels rn = ge_niels_identity();
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int kind = 0;  // 0: r -> out, 1: rn -> aux, 2: w -> aux, 3: quad coordinate
  fe coord = fe_zero();
  switch (op) {
    case GE_OP_MADD: r = ge_madd(P, N); break;
    case GE_OP_MSUB: r = ge_msub(P, N); break;
    case GE_OP_MADD_SIGNED: r = ge_madd_signed(P, N, neg); break;
    case GE_OP_MADD_FG: {
      const uint32_t e = i | (neg ? 0x80000000u : 0u);
      r = ge_madd_fg(P, fetch_entry_sw(nl, nullptr, 0xffffffffu, e), (e >> 31) != 0);
      break;
    }
    case GE_OP_MADD_H1H2: r = ge_madd_h2(ge_madd_signed_h1(P, N, neg)); break;
    case GE_OP_ADD: r = ge_add(P, Q); break;
    case GE_OP_ADD_QUAD:
      kind = 3;
      coord = ge_add_quad(P, Q, t & 3u);  // op is uniform: whole waves run the DPP exchange
      break;
    case GE_OP_DBL: r = ge_dbl(P); break;
    case GE_OP_NEG: r = ge_neg(P); break;
    case GE_OP_NIELS_FROM_AFFINE:
      kind = 1;
      rn = ge_niels_from_affine(P.X, P.Y);
      break;
    case GE_OP_TO_NIELS:
      kind = 1;
      rn = ge_to_niels(P);
      break;
    case GE_OP_FROM_NIELS: r = ge_from_niels(N); break;
    case GE_OP_ENCODE:
      kind = 2;
      ge_ristretto_encode(P, w);
      break;
    case GE_OP_DECODE: {
      uint32_t enc[8];
      _Pragma("unroll") for (int k = 0; k < 8; ++k) enc[k] = N.ypx.v[k];
      w[0] = ge_ristretto_decode(enc, r);
      if (live) aux[GE_AUX_WORDS * (size_t)i] = w[0];
      break;
    }
    case GE_OP_EQ:
      kind = 2;
      w[0] = ge_ristretto_eq(P, Q);
      break;
    case GE_OP_ELLIGATOR: r = ge_elligator(P.X); break;
    default: break;
  }
  if (!live) return;  // (after every cross-lane exchange)
  if (kind == 0) {
    store_p3(out, i, r);
  } else if (kind == 1) {
    store_niels(aux, i, rn);
  } else if (kind == 2) {
    _Pragma("unroll") for (int k = 0; k < 8; ++k) aux[GE_AUX_WORDS * (size_t)i + k] = w[k];
  } else {
    const uint32_t c = t & 3u;
    _Pragma("unroll") for (int k = 0; k < FE_LIMBS; ++k) out[P3_WORDS * (size_t)i + 10 * c + k] = coord.v[k];
  }
}

// ----------------------------------------------------------------- digits
// out[t * Wn + w] = digit of window wb + w (zero-filled by the host: the
// callback is only called for non-zero digits)
__global__ void __launch_bounds__(PROBE_T) k_probe_for_each_digit(const uint32_t* __restrict__ scalars, MsmGeom g,
                                                                  int32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * PROBE_T + threadIdx.x;
  const uint32_t i = t < g.T ? t : 0;
  uint32_t s[8];
  load_scalar(scalars, i, s);
  const bool live = t < g.T;
  for_each_digit(s, g, [&](uint32_t w, int d) {
    if (live) out[(size_t)i * g.Wn + w] = d;
  });
}

// out[(t * W + w) * 3 ..] = row, neg, zero of DtLane::row_of for generator gen
__global__ void __launch_bounds__(PROBE_T) k_probe_dt_rows(const uint32_t* __restrict__ scalars, DtGeom g, uint32_t gen,
                                                           uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * PROBE_T + threadIdx.x;
  const uint32_t cs = t / g.W, w = t % g.W;
  const uint32_t i = cs < n ? cs : 0;
  uint32_t s[8];
  load_scalar(scalars, i, s);
  const DtLane ln = DtLane::make(g, w);
  uint32_t row;
  bool neg, zero;
  ln.row_of(g, s, gen, row, neg, zero);
  if (cs < n) {
    uint32_t* o = out + ((size_t)i * g.W + w) * 3;
    o[0] = row;
    o[1] = neg;
    o[2] = zero;
  }
}

// bins[k] = rs_bin of the 16-bit digit code dig[ww * T + t] in window ww of
// the launch (0xffffffff for a zero digit)
__global__ void __launch_bounds__(PROBE_T) k_probe_rs_bins(const dig_t* __restrict__ dig, MsmGeom g, uint32_t NC,
                                                           uint32_t* __restrict__ bins) {
  const uint32_t k = blockIdx.x * PROBE_T + threadIdx.x;
  const uint32_t tot = g.Wn * g.T;
  const uint32_t i = k < tot ? k : 0;
  const uint32_t code = dig_expand(dig[i]);
  const uint32_t ww = i / g.T;
  const uint32_t bin = code == DIG_ZERO ? 0xffffffffu : rs_bin(code & ~DIG_SIGN, rs_fbits(g, ww), NC);
  if (k < tot) bins[i] = bin;
}

// ------------------------------------------------------------------- host
namespace {
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
  hipError_t upload(const void* h, size_t bytes) {
    hipError_t e = alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, h, bytes, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t zeroed(size_t bytes) {
    hipError_t e = alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemset(p, 0, bytes);
    return e;
  }
  hipError_t download(void* h, size_t bytes) const {
    return bytes ? hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  }
  template <class T>
  T* as() const { return (T*)p; }
};
unsigned blocks_for(size_t lanes) { return (unsigned)((lanes + PROBE_T - 1) / PROBE_T); }
hipError_t finish_launch() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}
}  // namespace

#define PR(x)                          \
  do {                                 \
    const hipError_t e_ = (x);         \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

extern "C" {

int bpp_probe_fe(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  if (!n) return 0;
  if (op >= FE_OP_COUNT || n > (1u << 24)) return (int)hipErrorInvalidValue;
  PR(hipSetDevice(0));
  DevBuf da, db, dout;
  PR(da.upload(a, n * 40));
  PR(db.upload(b, n * 40));
  PR(dout.zeroed(n * FE_OUT_WORDS * 4));
  hipLaunchKernelGGL(k_probe_fe, dim3(blocks_for(n)), dim3(PROBE_T), 0, 0, op, da.as<uint32_t>(), db.as<uint32_t>(),
                     dout.as<uint32_t>(), (uint32_t)n);
  PR(finish_launch());
  return (int)dout.download(out, n * FE_OUT_WORDS * 4);
}

int bpp_probe_sc(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  if (!n) return 0;
  if (op >= SC_OP_COUNT || n > (1u << 24)) return (int)hipErrorInvalidValue;
  PR(hipSetDevice(0));
  DevBuf da, db, dout;
  PR(da.upload(a, n * 32));
  PR(db.upload(b, n * 32));
  PR(dout.zeroed(n * 32));
  hipLaunchKernelGGL(k_probe_sc, dim3(blocks_for(n)), dim3(PROBE_T), 0, 0, op, da.as<uint32_t>(), db.as<uint32_t>(),
                     dout.as<uint32_t>(), (uint32_t)n);
  PR(finish_launch());
  return (int)dout.download(out, n * 32);
}

int bpp_probe_ge(uint32_t op, const uint32_t* p, const uint32_t* q, const uint32_t* nl, const uint32_t* flag,
                 uint32_t* out, uint32_t* aux, size_t n) {
  if (!n) return 0;
  if (op >= GE_OP_COUNT || n > (1u << 20)) return (int)hipErrorInvalidValue;
  PR(hipSetDevice(0));
  DevBuf dp, dq, dn, df, dout, daux;
  PR(dp.upload(p, n * P3_BYTES));
  PR(dq.upload(q, n * P3_BYTES));
  PR(dn.upload(nl, n * MSM_NIELS_WORDS * 4));
  PR(df.upload(flag, n * 4));
  PR(dout.zeroed(n * P3_BYTES));
  PR(daux.zeroed(n * GE_AUX_WORDS * 4));
  const size_t lanes = op == GE_OP_ADD_QUAD ? 4 * n : n;
  hipLaunchKernelGGL(k_probe_ge, dim3(blocks_for(lanes)), dim3(PROBE_T), 0, 0, op, dp.as<uint32_t>(),
                     dq.as<uint32_t>(), dn.as<uint32_t>(), df.as<uint32_t>(), dout.as<uint32_t>(), daux.as<uint32_t>(),
                     (uint32_t)n);
  PR(finish_launch());
  PR(dout.download(out, n * P3_BYTES));
  return (int)daux.download(aux, n * GE_AUX_WORDS * 4);
}

// geom[0..11] = W, B, tfb, K[0..7], NC (the radix sort's coarse bins, B >> RS_FINE_BITS)
// of msm_geom(1, 1, c, 0, W); geom[12..21] = W, H, K[0..7] of dt_geom(c)
int bpp_probe_geom(uint32_t c, uint32_t* geom) {
  if (c < 2 || c > 16) return (int)hipErrorInvalidValue;
  const uint32_t W = (254 + c - 1) / c;
  const MsmGeom g = msm_geom(1, 1, c, 0, W);
  geom[0] = g.W;
  geom[1] = g.B;
  geom[2] = g.tfb;
  for (int i = 0; i < 8; ++i) geom[3 + i] = g.K[i];
  geom[11] = g.B >> RS_FINE_BITS;
  const DtGeom d = dt_geom(c);
  geom[12] = d.W;
  geom[13] = d.H;
  for (int i = 0; i < 8; ++i) geom[14 + i] = d.K[i];
  return 0;
}

static bool window_range_ok(uint32_t c, uint32_t wb, uint32_t Wn) {
  if (c < 2 || c > 16) return false;
  const uint32_t W = (254 + c - 1) / c;
  return Wn >= 1 && wb < W && Wn <= W - wb;
}

// for_each_digit over windows [wb, wb + Wn): out = n x Wn signed digits
int bpp_probe_for_each_digit(uint32_t c, uint32_t wb, uint32_t Wn, const uint32_t* scalars, size_t n, int32_t* out) {
  if (!n) return 0;
  if (!window_range_ok(c, wb, Wn) || n > (1u << 20)) return (int)hipErrorInvalidValue;
  PR(hipSetDevice(0));
  const MsmGeom g = msm_geom(1, (uint32_t)n, c, wb, Wn);
  DevBuf ds, dout;
  PR(ds.upload(scalars, n * 32));
  PR(dout.zeroed(n * Wn * 4));
  hipLaunchKernelGGL(k_probe_for_each_digit, dim3(blocks_for(n)), dim3(PROBE_T), 0, 0, ds.as<uint32_t>(), g,
                     dout.as<int32_t>());
  PR(finish_launch());
  return (int)dout.download(out, n * Wn * 4);
}

// the product's k_msm_digits: dig = Wn x n 16-bit codes, window-major
int bpp_probe_msm_digits(uint32_t c, uint32_t wb, uint32_t Wn, const uint32_t* scalars, size_t n, uint16_t* dig) {
  if (!n) return 0;
  if (!window_range_ok(c, wb, Wn) || n > (1u << 20)) return (int)hipErrorInvalidValue;
  PR(hipSetDevice(0));
  const MsmGeom g = msm_geom(1, (uint32_t)n, c, wb, Wn);
  DevBuf ds, dd;
  PR(ds.upload(scalars, n * 32));
  PR(dd.zeroed(n * Wn * sizeof(dig_t)));
  hipLaunchKernelGGL(k_msm_digits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ds.as<uint32_t>(), g,
                     dd.as<dig_t>());
  PR(finish_launch());
  return (int)dd.download(dig, n * Wn * sizeof(dig_t));
}

// the product's k_rsort_digits_count on one chunk (n <= RS_CHUNK, c in
// 12..16): dig = Wn x n codes, cntA = Wn x NC coarse counts (NC = 2^(c-1) >>
// RS_FINE_BITS), bins = Wn x n rs_bin of every code (0xffffffff: zero digit)
int bpp_probe_rsort_digits_count(uint32_t c, uint32_t wb, uint32_t Wn, const uint32_t* scalars, size_t n,
                                 uint16_t* dig, uint32_t* cntA, uint32_t* bins) {
  if (!n) return 0;
  if (!window_range_ok(c, wb, Wn) || c < 12 || n > RS_CHUNK) return (int)hipErrorInvalidValue;
  const MsmGeom g = msm_geom(1, (uint32_t)n, c, wb, Wn);
  const uint32_t NC = g.B >> RS_FINE_BITS;
  if ((size_t)Wn * NC > RS_DC_HMAX) return (int)hipErrorInvalidValue;
  PR(hipSetDevice(0));
  DevBuf ds, dd, dc, dz, db;
  PR(ds.upload(scalars, n * 32));
  PR(dd.zeroed(n * Wn * sizeof(dig_t)));
  PR(dc.zeroed((size_t)Wn * NC * 4));
  PR(dz.zeroed(8));
  PR(db.zeroed(n * Wn * 4));
  hipLaunchKernelGGL(k_rsort_digits_count, dim3(1), dim3(RS_DC_T), 0, 0, ds.as<uint32_t>(), g, 1u, NC, dd.as<dig_t>(),
                     dc.as<uint32_t>(), dz.as<uint32_t>(), dz.as<uint32_t>() + 1);
  hipLaunchKernelGGL(k_probe_rs_bins, dim3(blocks_for(n * Wn)), dim3(PROBE_T), 0, 0, dd.as<dig_t>(), g, NC,
                     db.as<uint32_t>());
  PR(finish_launch());
  PR(dd.download(dig, n * Wn * sizeof(dig_t)));
  PR(dc.download(cntA, (size_t)Wn * NC * 4));
  return (int)db.download(bins, n * Wn * 4);
}

// DtLane::row_of for every (scalar, window): out = n x W x (row, neg, zero)
int bpp_probe_dt_rows(uint32_t c, uint32_t gen, const uint32_t* scalars, size_t n, uint32_t* out) {
  if (!n) return 0;
  if (c < 2 || c > 16 || n > (1u << 20)) return (int)hipErrorInvalidValue;
  PR(hipSetDevice(0));
  const DtGeom g = dt_geom(c);
  if (((uint64_t)gen * g.W + g.W) * g.H >= 0x100000000ull) return (int)hipErrorInvalidValue;  // row is 32-bit
  DevBuf ds, dout;
  PR(ds.upload(scalars, n * 32));
  PR(dout.zeroed(n * g.W * 12));
  hipLaunchKernelGGL(k_probe_dt_rows, dim3(blocks_for(n * g.W)), dim3(PROBE_T), 0, 0, ds.as<uint32_t>(), g, gen,
                     (uint32_t)n, dout.as<uint32_t>());
  PR(finish_launch());
  return (int)dout.download(out, n * g.W * 12);
}

}  // extern "C"
