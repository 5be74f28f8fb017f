// Permutation circuit + arithmetic-circuit proof (sound mode) — host side.
//
// Restates the reference's ACProof::ArithmeticCircuitProof
// (bp-perm/src/circuit_lib.rs:139-585) and the permutation circuit of
// weights.rs:26-204 in their sound form (SURVEY.md §2.2 defects Q1-Q10
// fixed; DESIGN.md "Protocol"), with every group operation dropped through
// the GPU (MSM engine, fixed-base Pedersen, IPA).  Matrices are sparse
// (the reference's dense Q x n matrices are 99.4 % zeros).
#pragma once
#include <stdint.h>

#include <array>
#include <memory>
#include <vector>

#include "merlin.h"
#include "scalar.h"

namespace circuit {
struct Program;  // circuit.h
}

namespace perm {

struct Entry {
  uint32_t q, col;
  hsc::Sc val;
  hsc::Sc valR;  // Montgomery form of val (zW products in one step)
};

struct Circuit {
  uint32_t k = 0, n = 0, n_p = 0, lg = 0, Q = 0, m = 0;
  uint32_t nv = 0;  // commitments absorbed before the x_perm challenge: 2k (two halves) or k (deck circuit)
  std::vector<Entry> WL, WR, WO, WV;
  std::vector<hsc::Sc> c;  // c[Q-1] = -x set per proof (deck circuit: c[Q-2] = deck_product(x) too)
  // deck circuit (build_deck) only: the public deck and its transcript digest
  bool deck = false;
  std::vector<hsc::Sc> cards;
  uint8_t deck_digest[32] = {0};
  // caller-defined circuit (circuit.h compile) only: the gate program the
  // witness is evaluated from, and its description's transcript digest
  std::shared_ptr<const circuit::Program> program;
  uint8_t program_digest[32] = {0};
  // ... with public inputs (bpp_circuit_create_pub): a proof's constant vector
  // is c + W_U u over its own n_pub public scalars u, which its transcript
  // absorbs ("pub", 32 bytes each) right after the prefix below
  uint32_t n_pub = 0;
  std::vector<Entry> WU;  // (col = the public input's index)
  // BPP_CIRCUIT_TILED: the large-circuit kernels (split row tables, wires in
  // global memory) even where the narrow ones fit.  How the statement is
  // computed, never part of it: no digest, transcript or proof byte reads it.
  bool tiled = false;
};

Circuit build(uint32_t k);

// The deck circuit (bpp_deck_*): V_0..V_{k-1} commit to a permutation of the
// PUBLIC deck d_0..d_{k-1}, V_k to x.  One product chain prod (v_i - x) of
// n = k - 1 gates inside the proof; the deck's own product D = prod (d_i - x)
// is a per-proof constant both sides compute.  v = [d_pi(0)..d_pi(k-1), x],
// m = k + 1, Q = 2k:
//   rows q = g (g < n):  a_L[g] = v_0 - x (g = 0) or a_O[g-1]
//   rows q = n + g:      a_R[g] = v_{g+1} - x
//   row 2k - 2:          a_O[k-2] = D
//   row 2k - 1:          v_k = x  (c = -x: the last row, as in build)
// n_p = max(4, next_pow2(k - 1)): no batched kernel has run below n_p = 4
// (build's k = 2).  deck: k canonical scalars (32 bytes each; the caller has
// checked them), or nullptr for 1..k.  deck_digest =
// SHAKE256("bpperm-deck" || le32 k || d_0 || .. || d_{k-1})[0..32], absorbed
// by transcript_prefix.
Circuit build_deck(uint32_t k, const uint8_t* deck);
// D = prod_i (d_i - x) of a deck circuit
hsc::Sc deck_product(const Circuit& C, const hsc::Sc& x);
// v = [cards[pi], x]; gate values of the one chain
void witness_deck(const Circuit& C, const std::vector<uint32_t>& pi, const hsc::Sc& x, std::vector<hsc::Sc>& v,
                  std::vector<hsc::Sc>& aL, std::vector<hsc::Sc>& aR, std::vector<hsc::Sc>& aO);
// What every proof's transcript absorbs after Transcript(label) and before
// V_0: dom-sep("acp v1", n_p), then the statement's label and digest -- "deck"
// and the deck's digest, "circuit" and the program's, nothing for the two-half
// circuit -- which is what keeps proofs of one shape (same m, n_p and byte
// length: a two-half proof of k' cards, a deck proof of 2k' cards, a program
// that restates either) from verifying as each other.
inline const char* statement_label(const Circuit& C) { return C.deck ? "deck" : C.program ? "circuit" : nullptr; }
inline void transcript_prefix(const Circuit& C, merlin::Transcript& tr) {
  tr.arithmetic_domain_sep(C.n_p);
  if (const char* s = statement_label(C)) tr.append(s, C.deck ? C.deck_digest : C.program_digest, 32);
}
// ... then one proof's own public inputs (pub: C.n_pub canonical scalars),
// before V_0 and so before every challenge
inline void transcript_pub(const Circuit& C, merlin::Transcript& tr, const uint8_t* pub) {
  for (uint32_t i = 0; i < C.n_pub; ++i) tr.append("pub", pub + 32 * (size_t)i, 32);
}

// Dynamic LDS of the one-workgroup-per-proof kernels k_poly_coef and
// k_verify_scalars (poly.hip and verify_scalars.hip launch them with exactly these; kPolyLanes =
// POLY_T = POW_LO): z^0..z^Q, two tables of min(n_p, kPolyLanes) powers, and
// the workgroup-sum scratch of 7 (2) scalars per wave.  kLdsMax: what one
// workgroup may take.
constexpr uint32_t kPolyLanes = 256;
constexpr size_t kLdsMax = 64 * 1024;
inline size_t poly_coef_lds(uint32_t Q, uint32_t n_p) {
  return ((size_t)Q + 1 + 2 * (n_p < kPolyLanes ? n_p : kPolyLanes)) * 32 + (kPolyLanes / 64) * 7 * 32;
}
inline size_t verify_scalars_lds(uint32_t Q, uint32_t n_p) {
  return ((size_t)Q + 1 + 2 * (n_p < kPolyLanes ? n_p : kPolyLanes)) * 32 + (kPolyLanes / 64) * 2 * 32;
}
// The same two kernels with the row table split in two (k_poly_coef_tiled,
// k_verify_scalars[_pub]_tiled; large circuits, circuit.h): lo[i] = z^i for i <
// kRowLo and hi[j] = z^(kRowLo j) for j <= Q / kRowLo in place of z^0..z^Q, the
// rest as above; nred = 7 (2) scalars of workgroup-sum scratch per wave.  Below
// kLdsMax for every Q a circuit may have (static_assert).
constexpr uint32_t kRowLo = 256;
constexpr size_t split_tables_lds(uint32_t Q, uint32_t n_p, uint32_t nred) {
  return ((size_t)kRowLo + (Q / kRowLo) + 1 + 2 * (n_p < kPolyLanes ? n_p : kPolyLanes)) * 32 +
         (kPolyLanes / 64) * nred * 32;
}
static_assert(split_tables_lds((3u << 16) + 1, 1u << 16, 7) <= kLdsMax, "Q <= 2 kMaxGates + kMaxAsserts + 1 fits");
// The chain witness kernels (witness.hip chain_prefix_products; k_witness and
// k_witness_cards: 2 chains of k, k_witness_deck: 1): the prefix products
// [chains][k] and two scan buffers [chains][lanes] of 32-byte scalars.  256
// lanes while that fits; the two-chain kernels then go on at 128, and the
// device witness ends (the host's begins) past chain_witness_dev_max.
constexpr uint32_t chain_witness_min_lanes(uint32_t chains) { return chains == 2 ? 128 : 256; }
constexpr size_t chain_witness_lds(uint32_t chains, uint32_t k, uint32_t lanes) {
  return ((size_t)chains * k + 2 * (size_t)chains * lanes) * 32;
}
constexpr uint32_t chain_witness_lanes(uint32_t chains, uint32_t k) {
  return chain_witness_lds(chains, k, 256) <= kLdsMax ? 256 : chain_witness_min_lanes(chains);
}
constexpr size_t chain_witness_lds(uint32_t chains, uint32_t k) {
  return chain_witness_lds(chains, k, chain_witness_lanes(chains, k));
}
constexpr uint32_t chain_witness_dev_max(uint32_t chains) {
  return (uint32_t)(kLdsMax / 32 - 2 * chains * chain_witness_min_lanes(chains)) / chains;
}
static_assert(chain_witness_dev_max(2) == 768 && chain_witness_lanes(2, 512) == 256 && chain_witness_lanes(2, 513) == 128 &&
                  chain_witness_dev_max(1) == 1536 && chain_witness_lds(1, 1536) == kLdsMax &&
                  chain_witness_lds(2, 768) == kLdsMax,
              "the witness paths' sizes");

// v = [1..k, pi(1..k), x]; gate values (sound create_a)
void witness(const Circuit& C, const std::vector<uint32_t>& pi, const hsc::Sc& x, std::vector<hsc::Sc>& v,
             std::vector<hsc::Sc>& aL, std::vector<hsc::Sc>& aR, std::vector<hsc::Sc>& aO);
// The same over a caller's deck (bpp_perm_prove_shuffle_batch): v = [cards,
// cards[pi], x], cards = k canonical scalars (the explicit v of the
// reference's create_a, weights.rs:63-113)
void witness(const Circuit& C, const hsc::Sc* cards, const std::vector<uint32_t>& pi, const hsc::Sc& x,
             std::vector<hsc::Sc>& v, std::vector<hsc::Sc>& aL, std::vector<hsc::Sc>& aR, std::vector<hsc::Sc>& aO);

// (z^Q)^T W as a dense vector of length ncols
std::vector<hsc::Sc> zW(const std::vector<Entry>& W, const std::vector<hsc::Sc>& zq, uint32_t ncols);

// Prover seed: the 8-byte little-endian u64 of the deterministic test
// entry points (bpp_perm_prove / _batch) or 32 bytes of caller / OS entropy
// (bpp_perm_prove_batch_entropy), absorbed after the domain string.
struct Seed {
  uint8_t b[32] = {0};
  uint32_t len = 8;
  static Seed u64(uint64_t x) {
    Seed s;
    memcpy(s.b, &x, 8);
    s.len = 8;
    return s;
  }
  static Seed bytes32(const uint8_t* p) {
    Seed s;
    memcpy(s.b, p, 32);
    s.len = 32;
    return s;
  }
};

// SHAKE256(domain || seed bytes) byte stream (oracle/merlin.py Rng)
struct Rng {
  merlin::Shake256 sh;
  Rng(const char* domain, const Seed& seed) {
    sh.update((const uint8_t*)domain, strlen(domain));
    sh.update(seed.b, seed.len);
  }
  Rng(const char* domain, uint64_t seed) : Rng(domain, Seed::u64(seed)) {}
  void bytes(uint8_t* out, size_t n) { sh.read(out, n); }
  uint64_t u64() {
    uint8_t b[8];
    bytes(b, 8);
    uint64_t x;
    memcpy(&x, b, 8);
    return x;
  }
  hsc::Sc scalar() {
    uint8_t b[64];
    bytes(b, 64);
    return hsc::from_wide(b);
  }
};

std::vector<uint32_t> fisher_yates(uint32_t k, Rng& rng);

// The prover's random draws (the stand-in for thread_rng,
// circuit_lib.rs:175): pi by Fisher-Yates from the stream
// SHAKE256("bpperm-prove" || seed), one u64 per step; the blinding scalars
// by index j in the order gamma[m], alpha, beta, rho, s_L[n_p], s_R[n_p],
// tau[5], scalar j = from_wide(SHAKE256("bpperm-prove-sc" || seed ||
// le32 j)[0..64]) (draw_scalar; oracle/merlin.py indexed_scalar) -- one
// sponge block per draw, so the GPU makes every draw in its own thread
// (witness.h draws_dev).
void draw_prover_randomness(const Circuit& C, const Seed& seed, std::vector<uint32_t>& pi, std::vector<hsc::Sc>& gamma,
                            hsc::Sc& alpha, hsc::Sc& beta, hsc::Sc& rho, std::vector<hsc::Sc>& sL,
                            std::vector<hsc::Sc>& sR, std::vector<hsc::Sc>& taus);
#define BPP_DRAW_DOMAIN "bpperm-prove-sc"
#define BPP_DRAW_DOMAIN_LEN 15
hsc::Sc draw_scalar(const Seed& seed, uint32_t j);
inline uint32_t draw_alpha_index(const Circuit& C) { return C.m; }            // then beta, rho
inline uint32_t draw_tau_index(const Circuit& C) { return C.m + 3 + 2 * C.n_p; }  // tau[5]
inline uint32_t draw_count(const Circuit& C) { return C.m + 3 + 2 * C.n_p + 5; }

struct RandomDraws {
  std::vector<uint32_t> pi;
  std::vector<hsc::Sc> gamma, sL, sR, taus;
  hsc::Sc alpha, beta, rho;
};
// The draws of eight proofs at once: the eight pi streams and each index's
// eight scalar sponges run through an AVX-512 8-way Keccak
// (host/keccak_x8.cpp; scalar fallback without AVX-512), identical to
// draw_prover_randomness.  (the eight seeds must have the same length)
void draw_prover_randomness_x8(const Circuit& C, const Seed seeds[8], RandomDraws* const out[8]);
// As above, but only the host's share -- pi, alpha, beta, rho and tau: the
// GPU draws gamma, s_L and s_R (and alpha, beta, rho again, into its scalar
// arrays; witness.h draws_dev), and out[j]'s vectors for them are left empty.
// with_pi = false (a caller-supplied shuffle): no pi stream is read and
// out[j]->pi is left as it is.
void draw_prover_host_x8(const Circuit& C, const Seed seeds[8], RandomDraws* const out[8], bool with_pi = true);

size_t proof_len(uint32_t k);        // two-half circuit of k cards
size_t proof_len(const Circuit& C);  // either circuit: 32 (13 + 2 lg)

// Batch-verification weight of proof p (its index in the batch) with weight
// challenge r_p (its own transcript's "t-check-weight"):
//   w_p = from_bytes_mod_order_wide(SHAKE256("bp-perm-batch-wt" || seed ||
//         le64 p || r_p)[0..64])
// seed = 32 bytes of the VERIFIER's randomness (getrandom; every rank of a
// split batch uses the same seed), mixed with the proof's own transcript
// challenge as bulletproofs' r1cs batch verifier mixes its external rng into
// each proof's TranscriptRng.  The weights need nothing from the other
// proofs, so they are made in each proof's own GPU lane right after its
// replay (DESIGN.md §5 "Batch weights").  A seed the provers can predict
// voids the batch's soundness.
hsc::Sc batch_weight(const uint8_t seed[32], uint64_t p, const hsc::Sc& r);
// len bytes from the OS CSPRNG (getrandom, restarted when a signal
// interrupts it); false if it fails.  The verifier's batch seed and the
// provers' entropy both come from here.
__attribute__((visibility("hidden"))) bool os_entropy(uint8_t* out, size_t len);  // (not exported)
bool verify_seed(uint8_t seed[32]);  // os_entropy(seed, 32)

}  // namespace perm
