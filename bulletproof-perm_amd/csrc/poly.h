// Device vector-polynomial stage of the batched prover (poly.hip).
#pragma once
#include <vector>

#include "ctx.h"
#include "host/perm.h"

// t_1, t_3..t_6 inputs: for P proofs, with d_sc the A_I/A_O/S scalar array
// ([P][per], per = 3 + 5 n_p: alpha, a_L, a_R, beta, a_O, rho, s_L, s_R,
// canonical), d_gamma the V blindings ([P][m], canonical) and ch =
// [P][y, y^-1, z] (canonical): t = [P][t_1..t_6, <z^Q W_V, gamma>].
// Keeps the l(X), r(X) coefficient vectors and the H factors y^-i on the
// device for poly_x_dev.
int poly_coef_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_sc, uint32_t per,
                  const uint32_t* d_gamma, const std::vector<hsc::Sc>& ch, std::vector<hsc::Sc>& t);

// l = l(x), r = r(x) ([P][n_p], canonical, on the device for the IPA), the
// H factors, and t_hat = <l, r> per proof.
int poly_x_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const std::vector<hsc::Sc>& x, uint32_t** d_l,
               uint32_t** d_r, uint32_t** d_hf, std::vector<hsc::Sc>& t_hat);

// What the verifier's scalar kernels (verify_scalars.hip) share with
// k_poly_coef: the circuit matrices' column-CSR and the lanes per proof
// (comments at their definitions, poly.hip).  Not exported: they were file-local
// while the two stages shared a file.
#define POLY_HIDDEN __attribute__((visibility("hidden")))
POLY_HIDDEN void build_csr(const perm::Circuit& C, std::vector<uint32_t>& cp, std::vector<uint32_t>& ce, bool with_v);
POLY_HIDDEN unsigned poly_block(uint32_t n_p);
POLY_HIDDEN unsigned poly_block(const perm::Circuit& C);
