// Masked re-shuffle proof: the device steps (masked_reshuffle.hip) that the
// prover and the verifiers of masked_reshuffle_api.hip queue on a context's
// stream beside the blind re-shuffle's own (reshuffle.h), which they reuse
// unchanged.  All arrays are device memory; a scalar is 8 canonical words; a
// card is two points, U then W, and a table of cards holds them in that order
// (rows 2j and 2j + 1 of card j).
#pragma once
#include <stdint.h>

#include "ctx.h"

// Points per proof in the verifier's table, in this order: (U W)[k] (U' W')[k]
// A[k] E[k] Ti[k] T_U T_W; the key K is the table's point 0, before the first
// proof's
inline uint32_t mrs_points(uint32_t k) { return 7 * k + 2; }

// r_i K (lanes 0 .. Pk - 1) and t_R K (lanes Pk .. Pk + P - 1) -> out [Pk + P]
// extended (secret), in constant time over the scalars; key: the Niels row of K
int mrs_key_mul_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* key, uint32_t* out);
// (U'_i, W'_i) = (U_perm[i] + r_i B, W_perm[i] + r_i K): tbl_in Niels [P][2k],
// rB and rK extended [P][k] -> encodings [P][k][2] and the table rows [P][2k]
int mrs_outputs_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* tbl_in, const uint32_t* perms,
                    const uint32_t* rB, const uint32_t* rK, uint32_t* out_enc, uint32_t* out_tbl);
// T_U = sum_i t_i U'_i - t_R B and T_W = sum_i t_i W'_i - t_R K per proof ->
// res [P][2] extended, in constant time over the secret t_i: prod [P][2k]
// extended (secret) holds t_i U'_i, t_i W'_i; tRB, tRK [P] extended
int mrs_tsum_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* draws, const uint32_t* tbl_out, uint32_t* prod,
                 const uint32_t* tRB, const uint32_t* tRK, uint32_t* res);
// D_i = y A_i + E_i over the verifier's table (tbl: the first proof's row 0)
// -> extended [P][k]
int mrs_D_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, const uint32_t* tbl, const uint32_t* y, uint32_t* out_p3);
// The weighted terms of checks (i), (ii-U) and (ii-W), `stride` per proof:
// 6k + 2 over the proof's table points (n0 + 1 + p (7k + 2) + ..) in the order
// T_i, E_i, U'_i, W'_i, U_j, W_j, T_U, T_W, and u_j = y j + x^(j+1).
// stride = 6k + 2: the batch's B, Bb and K sums follow the last proof's terms;
// stride = 6k + 5: every proof's own B, Bb and K terms end its row, off [P + 1].
// K is table point n0.  scratch: (2Pk + 3P) scalars.
int mrs_sigma_terms_dev(bpp_ctx* ctx, uint32_t P, uint32_t k, uint32_t stride, const uint32_t* resp,
                        const uint32_t* x, const uint32_t* y, const uint32_t* c, const uint32_t* rho, uint32_t n0,
                        uint32_t bidx, uint32_t bbidx, uint32_t* scal, uint32_t* idx, uint32_t* off, uint32_t* u,
                        uint32_t* scratch);
