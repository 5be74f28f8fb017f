// Caller-defined circuits (bpp_circuit_*): a gate program in the style of an
// R1CS constraint system, compiled to the sparse matrices of perm::Circuit
// (the convention of perm::build: W_L a_L + W_R a_R + W_O a_O = W_V v + c).
// Host code only; the C ABI is circuit_api.hip.
//
// Variables: committed inputs v_0..v_{m_in-1}; the challenge x (x_perm,
// squeezed after V_0..V_{m_in-1} and committed as V_{m_in}); the public inputs
// u_0..u_{n_pub-1} (per proof, never committed: both sides are given them and
// the transcript absorbs them before V_0); the wires l_h, r_h, o_h = l_h r_h of
// n multiplication gates.  A gate side is DEFINED -- a sparse linear
// combination over {1, v_j, x, u_i, wires of gates h < g} -- or FREE, fed from
// a per-proof auxiliary value aux_t supplied before x exists.  A assert rows
// each force a linear combination over any variable to 0.
//
// Rows: defined left sides by gate, defined right sides by gate, the asserts,
// then v_{m_in} = x (c[Q-1] = -x per proof).  Defined side of gate g at row q:
// W(q, g) = 1 in its own matrix, a wire term a -> -a in the wire's matrix, a
// v_j / x term -> W_V = a, a u_i term -> W_U = a, the constant -> c[q] = a.
// Assert row: wire terms +a, v / x terms -a, u_i terms -a, constant -a.  A
// proof's constant vector is c + W_U u (W_U: Q x n_pub); nothing else of the
// statement depends on u.  Q = defined sides + A + 1, m = m_in + 1, nv = m_in,
// n_p = max(4, next_pow2(n)).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "perm.h"

namespace circuit {

constexpr uint32_t SIDE_LC = 0xFFFFFFFFu;  // BPP_SIDE_LC: a defined side
constexpr uint32_t kTermOne = 0x80000000u, kTermNeg = 0x40000000u, kTermVar = 0x3FFFFFFFu;  // (ids stay below 2^30)
enum { OK = 0, ERR_ARG = 1, ERR_LEN = 2, ERR_NONCANONICAL = 4 };  // (the BPP_ codes)

// The caller's description (bpp_circuit_desc).
struct Desc {
  uint32_t m_in, n_gates, n_aux, n_asserts;
  const uint32_t* side_aux;  // [2n]
  const uint32_t* lc_off;    // [2n + A + 1]
  const uint32_t* lc_var;    // [T]
  const uint8_t* lc_coef;    // [T][32]
  uint32_t n_pub = 0;        // (bpp_circuit_create_pub's; not a field of bpp_circuit_desc)
  uint32_t flags = 0;        // (bpp_circuit_create_ex's kLarge | kTiled; never part of the digest)
};
constexpr uint32_t kLarge = 1u, kTiled = 2u;  // BPP_CIRCUIT_LARGE, BPP_CIRCUIT_TILED (TILED implies LARGE)

// variable ids of lc_var
inline uint32_t var_one() { return 0; }
inline uint32_t var_v(uint32_t j) { return 1 + j; }
inline uint32_t var_x(uint32_t m_in) { return 1 + m_in; }
inline uint32_t var_pub(uint32_t m_in, uint32_t i) { return 2 + m_in + i; }
inline uint32_t var_wire(uint32_t m_in, uint32_t h, uint32_t lro, uint32_t n_pub = 0) {
  return 2 + m_in + n_pub + 3 * h + lro;
}

// A hint program (bpp_circuit_hints): how the prover derives aux_t from {1, v_j,
// u_i}.  aux_t = op(w), w = the hint's combination mod l (empty: 0):
//   kHintValue  w                 kHintBit     bit `arg` of w in [0, l)
//   kHintInv    w^-1, 0 for w = 0  kHintNotBit  1 - that bit
//   kHintIsZero 1 when w = 0, else 0
// op word = op | arg << 8 (arg <= 252, BIT / NOT_BIT only).  A hint reads
// neither x (aux exists before x does) nor wires.  Attached at creation; no
// part of the statement: digest, matrices, transcript and proof bytes do not
// see it.
//
// Wire hints (bpp_circuit_create_wire_hinted): the combination ranges over the
// variable space of a defined side, {1, v_j, x, u_i, wires}.  A hint that reads
// x or a wire is LATE: it has no value before x exists, so it is evaluated
// where the witness is, when the gate it feeds is reached -- once for each side
// it feeds, from the wires of earlier gates (a late hint reading a wire of gate
// h feeds sides of gates g > h only); one that feeds no side is never evaluated.
// Every other hint is EARLY and is the hint above.
enum : uint32_t { kHintValue = 0, kHintBit = 1, kHintNotBit = 2, kHintInv = 3, kHintIsZero = 4, kHintOps = 5 };
constexpr uint32_t kHintMaxBit = 252;
constexpr uint32_t kNoLateHint = 0xFFFFFFFFu;  // the op word of a side without a late hint (Program::dev)
struct HintDesc {
  const uint32_t* op;       // [n_aux]
  const uint32_t* lc_off;   // [n_aux + 1]
  const uint32_t* lc_var;   // [T]: 0 = one, 1 + j = v_j, 2 + m_in + i = u_i (wire hints: every id of Desc::lc_var)
  const uint8_t* lc_coef;   // [T][32]
};
struct Hints {
  std::vector<uint32_t> op, lc_off, lc_var;
  std::vector<hsc::Sc> lc_coef;
  // what k_hint_aux reads, one upload: a record of 4 words per LANE -- the
  // hint's index t, its op word, its terms [begin, end) -- in an order grouped
  // by op (INV first: its lanes run a few hundred products, a BIT lane none),
  // so that the lanes of one wave run one op wherever the counts allow; then
  // the T terms' variable ids (| kTermOne / kTermNeg as in Program::dev), then
  // (from a multiple of 8 words) their Montgomery coefficients [T][8]
  // A late hint has a record too, {t, VALUE, 0, 0}: its lane writes a 0 that
  // nothing reads, and k_hint_aux stays the kernel it was.
  std::vector<uint32_t> dev;
  uint32_t dev_vars = 0, dev_coefs = 0;
  std::vector<uint8_t> late;  // [n_aux]: the hint reads x or a wire (empty: no late hint)
  uint32_t n_late = 0;
};

struct Program {
  uint32_t m_in = 0, n = 0, n_aux = 0, A = 0, n_pub = 0;
  std::shared_ptr<const Hints> hints;  // (compile with a HintDesc; null: aux is the caller's)
  std::vector<uint32_t> side_aux, lc_off, lc_var;
  std::vector<hsc::Sc> lc_coef;
  // gates by dependency level: level = 1 + the highest level among the gates
  // whose wires its definitions and its sides' late hints read (0: none); level
  // l = level_gate[level_off[l] .. level_off[l + 1]).  Scheduling, not statement.
  std::vector<uint32_t> level_off, level_gate;
  // what k_witness_program reads, one upload: side_aux [2n], lc_off [2n + A + 1],
  // lc_wire [2n + A] (the first term of each combination that reads a wire: ids
  // ascend, so the terms over {1, v_j, x, u_i} come before it), level_off [levels +
  // 1], level_gate [n], the T terms' variable ids (| kTermOne: coefficient 1, |
  // kTermNeg: coefficient -1, no multiply), then (from a multiple of 8 words:
  // 32-byte aligned) their Montgomery coefficients [T][8]; word offsets of the
  // six tables after side_aux.  With late hints (hints->n_late > 0) the image
  // gains, behind level_gate at dev_late, a record of 3 words per side -- the
  // op word of the side's late hint (kNoLateHint: none) and its terms [begin,
  // end) -- and the late hints' terms behind the T terms of the description, in
  // the same two tables (ids flagged, coefficients Montgomery), so one term loop
  // serves both; without late hints the image is what it was.
  std::vector<uint32_t> dev;
  uint32_t dev_lc_off = 0, dev_lc_wire = 0, dev_level_off = 0, dev_level_gate = 0, dev_vars = 0, dev_coefs = 0;
  uint32_t dev_late = 0;  // (0: no late hint)
  uint8_t digest[32] = {0};
};

// SHAKE256("bpperm-circuit" || le32 m_in || le32 n || le32 n_aux || le32 A ||
// side_aux || lc_off || lc_var || lc_coef)[0..32] over the arrays as given;
// with n_pub > 0, "bpperm-pubcircuit" || le32 m_in || le32 n_pub || le32 n || ..
void digest(const Desc& d, uint8_t out[32]);

// Validates and compiles: ERR_ARG for m_in = 0 or n = 0, ids or aux indices
// out of range, a definition reading a wire of gate h >= g, a nonempty
// combination on a free side, unsorted or duplicate ids, a zero coefficient, a
// non-monotone lc_off, unknown flag bits; ERR_NONCANONICAL for a coefficient
// >= l; ERR_LEN beyond kMaxPub, the kMax* below or, without kLarge, lds_fits.
// C.program is the compiled program; C.tiled = the kTiled flag.
// hints: nullptr, or the hint program (one hint per aux value), validated the
// same way: ERR_ARG for an unknown op, arg > 252, an arg on an op that takes
// none, an id out of range or naming x or a wire, unsorted ids, a zero
// coefficient, a non-monotone lc_off; ERR_NONCANONICAL for a coefficient >= l.
// wire_hints (bpp_circuit_create_wire_hinted): a hint's ids range over x and
// the wires too; ERR_ARG for an id beyond the last wire and for a late hint that
// reads a wire of gate h and feeds a side of a gate g <= h (checked for every
// side the aux index feeds).
int compile(const Desc& d, perm::Circuit& C, std::string& err, const HintDesc* hints = nullptr,
            bool wire_hints = false);
inline bool has_late_hints(const Program& P) { return P.hints && P.hints->n_late; }
// A prover given no aux rows (aux == nullptr) on a circuit with hints derives
// them: k_hint_aux, late hints inside the witness kernel.
inline bool aux_derived(const Program& P, const void* aux) { return !aux && P.n_aux && P.hints; }

// The hints' host reference: aux [n_aux] from v [m_in] and pub [n_pub]
// (canonical).  What BPP_CIRCUIT_HOST_WITNESS=1 runs in the prover, and what
// k_hint_aux must equal.  Not for a circuit with late hints (it has no x).
void hint_eval(const Program& P, const hsc::Sc* v, const hsc::Sc* pub, hsc::Sc* aux);
// The same with x: the early hints as hint_eval gives them, then the gates in
// order, each late hint from the wires so far, at every side it feeds (a late
// hint that feeds no side stays 0).  eval over this aux is the witness; what
// the late witness kernels must equal.
void hint_eval_x(const Program& P, const hsc::Sc* v, const hsc::Sc* pub, const hsc::Sc& x, hsc::Sc* aux);

// The host witness: a_L, a_R, a_O (n_p each, padding gates zero) from v
// [m_in], aux [n_aux] and x; *bad_assert = 1 + the first assert that does not
// hold, or 0.  pub: the n_pub public inputs (not read when n_pub = 0).
void eval(const Program& P, uint32_t n_p, const hsc::Sc* v, const hsc::Sc* aux, const hsc::Sc& x,
          std::vector<hsc::Sc>& aL, std::vector<hsc::Sc>& aR, std::vector<hsc::Sc>& aO, uint32_t* bad_assert,
          const hsc::Sc* pub = nullptr);

// k_witness_program's dynamic LDS: its fail word (32 B) and the 3n wire values;
// staged, also the proof's m_in inputs and n_pub public inputs in Montgomery form and a copy of the
// program's device image, which turns every level's dependent index and term
// loads from global-memory round trips into LDS reads.  Staged whenever that
// fits one workgroup's LDS, the plain form (program and inputs read from
// global memory) beyond.
inline size_t witness_program_lds(uint32_t n) { return (size_t)3 * n * 32 + 32; }
inline size_t witness_program_staged_lds(const Program& P) {
  return witness_program_lds(P.n) + ((size_t)P.m_in + P.n_pub) * 32 + P.dev.size() * 4;
}
// k_witness_program_wide keeps the 3n wires in global memory ([P][3n][8] words,
// "wp_wires", inside what prove_wipe zeroes) and only the fail word in LDS.
constexpr size_t witness_program_wide_lds() { return 32; }
// Which kernels a circuit's batches launch: each by its own bound, or all of
// the large-circuit ones under kTiled.
inline bool witness_wide(const perm::Circuit& C) { return C.tiled || witness_program_lds(C.n) > perm::kLdsMax; }
inline bool poly_coef_split(const perm::Circuit& C) {
  return C.tiled || perm::poly_coef_lds(C.Q, C.n_p) > perm::kLdsMax;
}
inline bool verify_scalars_split(const perm::Circuit& C) {
  return C.tiled || perm::verify_scalars_lds(C.Q, C.n_p) > perm::kLdsMax;
}
// "every per-proof kernel's workgroup fits its LDS" (what a circuit created
// without kLarge must satisfy): k_poly_coef and
// k_verify_scalars (perm.h, the formulas their launches use) and
// k_witness_program -- Q <= 1507 at n_p >= 256, n <= 682
inline bool lds_fits(uint32_t Q, uint32_t n_p, uint32_t n) {
  return perm::poly_coef_lds(Q, n_p) <= perm::kLdsMax && perm::verify_scalars_lds(Q, n_p) <= perm::kLdsMax &&
         witness_program_lds(n) <= perm::kLdsMax;
}
constexpr uint32_t kMaxInputs = 1u << 20, kMaxGates = 1u << 16, kMaxAsserts = 1u << 16, kMaxAux = 1u << 20,
                   kMaxPub = 1u << 16;

}  // namespace circuit
