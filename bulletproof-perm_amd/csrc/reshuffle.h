// Re-shuffle proofs, blind and masked: the device steps (reshuffle.hip) that the
// one prover and the one verifier sequence of reshuffle_api.hip queue on a
// context's stream.  All arrays are device memory unless named otherwise; a
// scalar is 8 canonical words.  A card is H points: one commitment (blind), or
// U then W (masked), and a table of cards holds them in that order (rows Hj ..
// Hj + H - 1 of card j).
#pragma once
#include <stdint.h>

#include "ctx.h"

// The two kinds of re-shuffle, as data: everything the sequences do differently
// follows from these fields.
struct RsKind {
  uint32_t H;           // points per card: 1, or 2 (U, W)
  uint32_t keys;        // table points in front of the first proof's: 0, or 1 (the key K)
  const char* name;     // what an error text starts with
  const char* dom;      // the transcript's dom-sep message
  const char* half[2];  // a card's points in an error text
  const char* tsum[2];  // the proof's H sum points in an error text
};
inline constexpr RsKind kRsBlind = {1, 0, "reshuffle", "reshuffle v1", {"", ""}, {"T_S 0", ""}};
inline constexpr RsKind kRsMasked = {2, 1, "masked reshuffle", "masked reshuffle v1", {"U of ", "W of "}, {"T_U", "T_W"}};

// Points per proof in the verifier's table, in this order: the cards in [k][H],
// the cards out [k][H], A[k] E[k] Ti[k], the H sums (T_S, or T_U T_W); the key,
// when there is one, is the table's point 0, before the first proof's
inline uint32_t rs_points(uint32_t H, uint32_t k) { return (3 + 2 * H) * k + H; }
// Terms per proof of the merged checks (i) and (ii): every point of the proof
// but A[k].  The H + 1 shared bases (B, Bb, and K with two points a card) follow
// once behind a batch's terms, or behind every proof's own (the _each fallback).
inline uint32_t rs_terms(uint32_t H, uint32_t k) { return (2 + 2 * H) * k + H; }
// Draws per proof; draw j is r, alpha, beta, t, w (k each), then t_R
inline uint32_t rs_draws(uint32_t k) { return 5 * k + 1; }

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
// r_i K (lanes 0 .. Pk - 1) and t_R K (lanes Pk .. Pk + P - 1) -> out [Pk + P]
// extended (secret), in constant time over the scalars; key: the Niels row of K
int mrs_key_mul_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* key, uint32_t* out);
// The output cards, their encodings [P][k][H] and their table rows [P][Hk]:
// H = 1: C'_i = C_perm[i] + R_i (rB extended [P][k] holds R_i = r_i Bb; rK unread);
// H = 2: (U'_i, W'_i) = (U_perm[i] + r_i B, W_perm[i] + r_i K), rB and rK extended [P][k].
// tbl_in: Niels [P][Hk]
int rs_outputs_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, const uint32_t* tbl_in, const uint32_t* perms,
                   const uint32_t* rB, const uint32_t* rK, uint32_t* out_enc, uint32_t* out_tbl);
// init: the 52 shared state words (first phase), or null: continue from states
int rs_transcript_dev(bpp_ctx* ctx, uint32_t P, const uint32_t* init, uint8_t* states, const RsPhase& ph,
                      uint32_t* ch_out);
// b_i = x^(perm[i] + 1)
int rs_exponents_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* x, const uint32_t* perms, uint32_t* b);
// The H sums per proof -> res [P][H] extended, in constant time over the secret
// t_i: prod [P][Hk] extended (secret) holds t_i times every row of tbl_out, the
// Niels table of the output cards.  H = 1: T_S = sum_i t_i C'_i - t_R Bb, tRB [P]
// extended is t_R Bb (tRK unread); H = 2: T_U = sum_i t_i U'_i - t_R B and T_W =
// sum_i t_i W'_i - t_R K, tRB and tRK [P] extended.
int rs_tsum_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* tbl_out,
                uint32_t* prod, const uint32_t* tRB, const uint32_t* tRK, uint32_t* res);
// resp [P][2k+1] = z | om | z_R; d, delta [P][k] (secret); u [P][k]
int rs_responses_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* perms,
                     const uint32_t* b, const uint32_t* x, const uint32_t* y, const uint32_t* c, uint32_t* resp,
                     uint32_t* d, uint32_t* delta, uint32_t* u);
// D_i = y A_i + E_i over the verifier's table (tbl: the first proof's row 0)
// -> extended [P][k]
int rs_D_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, const uint32_t* tbl, const uint32_t* y,
             uint32_t* out_p3);
// rho_p = from_wide(SHAKE256("bpperm-reshuffle-wt" || seed || le64 (first + p) || c_p)[0..64])
int rs_weights_dev(bpp_ctx* ctx, uint32_t P, const uint32_t* seed, uint64_t first, const uint32_t* c, uint32_t* rho);
// The weighted terms of checks (i) and (ii), and u_j = y j + x^(j+1): per proof
// rs_terms(H, k) over the proof's table points (H = 1: the first proof's first
// is n0; H = 2: K is table point n0 and the first proof's first n0 + 1), in the
// order T_i, E_i, the cards out (H = 2: every U'_i, then every W'_i), the cards
// in likewise, the H sums.
// each = false: rows of rs_terms, and the batch's sums for the H + 1 shared bases
// follow the last proof's terms; each = true: rows of rs_terms + H + 1, every
// proof's own shared-base terms ending its row, and off [P + 1].
// scratch: (2Pk + (H + 1) P) scalars.
int rs_sigma_terms_dev(bpp_ctx* ctx, uint32_t H, uint32_t P, uint32_t k, bool each, const uint32_t* resp,
                       const uint32_t* x, const uint32_t* y, const uint32_t* c, const uint32_t* rho, uint32_t n0,
                       uint32_t bidx, uint32_t bbidx, uint32_t* scal, uint32_t* idx, uint32_t* off, uint32_t* u,
                       uint32_t* scratch);
