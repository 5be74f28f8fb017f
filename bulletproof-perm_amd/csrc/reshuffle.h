// Blind re-shuffle proof: the device steps (reshuffle.hip) that the prover and
// the verifiers of reshuffle_api.hip queue on a context's stream.  All arrays
// are device memory unless named otherwise; a scalar is 8 canonical words.
#pragma once
#include <stdint.h>

#include "ctx.h"

// Points per proof in the verifier's table, in this order: C[k] C'[k] A[k]
// E[k] Ti[k] T_S
inline uint32_t rs_points(uint32_t k) { return 5 * k + 1; }
// Draws per proof; draw j is r, alpha, beta, t, w (k each), then t_R
inline uint32_t rs_draws(uint32_t k) { return 5 * k + 1; }

// What the masked re-shuffle (masked_reshuffle_api.hip) takes from
// reshuffle_api.hip as it is: the inner circuit shuffle_of_public(k), compiled
// once per k and kept (null: it did not compile), its proof's length, "k is a
// size this argument takes" (BPP_ERR_ARG below 2, BPP_ERR_LEN past 342), and
// k_decompress over n encodings with its verdict word reset (bad: 8 bytes, ~0
// or the first index that does not decode)
namespace perm {
struct Circuit;
}
const perm::Circuit* rs_circuit(uint32_t k);
size_t rs_inner_len(uint32_t k);
int rs_k_check(bpp_ctx* ctx, uint32_t k);
int rs_decompress_dev(bpp_ctx* ctx, const uint32_t* d_enc, size_t n, uint32_t* d_tbl, void* d_bad);

// One transcript phase: up to three runs of 32-byte messages, run s = n[s]
// messages under label lab[s] from seg[s] + p * stride[s] words, then one
// challenge scalar.  A label is its bytes packed little-endian, ln its length.
struct RsPhase {
  const uint32_t* seg[3];
  uint32_t n[3], stride[3], lab[3], ln[3];
  uint32_t ch, chn;
};

// draws (r, alpha, beta, t, w as [P][k] each, then t_R [P]) from seeds [P][8] (blinds: null, or [P][k] over draws 0..k-1),
// and per output slot pi(i) as a scalar (piv [P][k]) and 0 (zero [P][k])
int rs_draws_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* seeds, const uint32_t* blinds,
                 const uint32_t* perms, uint32_t* draws, uint32_t* piv, uint32_t* zero);
// C'_i = C_perm[i] + R_i (tbl_in: Niels [P][k]; rB: extended [P][k]) -> its
// encoding and its table point
int rs_outputs_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* tbl_in, const uint32_t* perms,
                   const uint32_t* rB, uint32_t* out_enc, uint32_t* out_tbl);
// init: the 52 shared state words (first phase), or null: continue from states
int rs_transcript_dev(bpp_ctx* ctx, uint32_t P, const uint32_t* init, uint8_t* states, const RsPhase& ph,
                      uint32_t* ch_out);
// b_i = x^(perm[i] + 1)
int rs_exponents_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* x, const uint32_t* perms, uint32_t* b);
// T_S = sum_i t_i C'_i - t_R Bb per proof -> res [P] extended, in constant time
// over the secret t_i: prod [P][k] extended (secret) holds t_i C'_i, tRB [P] is
// t_R Bb (pedersen_dev's walk); tbl_out: the Niels table of C'
int rs_tsum_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* tbl_out, uint32_t* prod,
                const uint32_t* tRB, uint32_t* res);
// resp [P][2k+1] = z | om | z_R; d, delta [P][k] (secret); u [P][k]
int rs_responses_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* perms,
                     const uint32_t* b, const uint32_t* x, const uint32_t* y, const uint32_t* c, uint32_t* resp,
                     uint32_t* d, uint32_t* delta, uint32_t* u);
// D_i = y A_i + E_i over the verifier's table -> extended [P][k]
int rs_D_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* tbl, const uint32_t* y, uint32_t* out_p3);
// rho_p = from_wide(SHAKE256("bpperm-reshuffle-wt" || seed || le64 (first + p) || c_p)[0..64])
int rs_weights_dev(bpp_ctx* ctx, uint32_t P, const uint32_t* seed, uint64_t first, const uint32_t* c, uint32_t* rho);
// The weighted terms of checks (i) and (ii), `stride` per proof: 4k + 1 over
// the proof's table points (n0 + p (5k + 1) + ..), and u_j = y j + x^(j+1).
// stride = 4k + 1: the batch's B and Bb sums follow the last proof's terms;
// stride = 4k + 3: every proof's own B and Bb terms end its row, off [P + 1].
int rs_sigma_terms_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, uint32_t stride, const uint32_t* resp, const uint32_t* x,
                       const uint32_t* y, const uint32_t* c, const uint32_t* rho, uint32_t n0, uint32_t bidx,
                       uint32_t bbidx, uint32_t* scal, uint32_t* idx, uint32_t* off, uint32_t* u, uint32_t* scratch);
