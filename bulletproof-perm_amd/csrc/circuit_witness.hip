// The circuit interpreter on the GPU: the witness of a caller-defined circuit
// (k_witness_program and its variants) and the auxiliary values its hints
// derive (k_hint_aux).  Declared in circuit_witness.h; the program and its
// device images are host/circuit.h.
#include <algorithm>

#include "ctx.h"
#include "circuit_witness.h"
#include "host/circuit.h"
#include "sc25519.cuh"

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
