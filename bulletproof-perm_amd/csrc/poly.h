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

// The batch verifier's MSM scalars for `count` proofs (k_verify_consts +
// k_verify_scalars + k_verify_merge): rec = [count][12 + lg] canonical
// scalars (x_perm, y, z, x, w, r, a, b, t_hat, tau_x, mu, -, u_j..); proof p
// is weighted by perm::batch_weight(seed, first + p, r_p); d_sc (device)
// receives the 2 n_p + 2 merged generator scalars then count x (m + 8 + 2 lg)
// weighted proof-point scalars, every proof's check scaled by
// (prod u_j)^2 y^(n_p - 1) (verify_dev.h).
int verify_scalars_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t count, const std::vector<uint32_t>& rec,
                       const uint8_t seed[32], uint64_t first, uint32_t* d_sc);

// The prover's blinding draws on the device (perm.h draw_scalar, one
// thread each) from per-proof sponge templates (d_tmpl [P][7] u64,
// draw_template; seed_len uniform over the batch, <= 32) -> gamma ([P][m],
// canonical) and alpha, beta, rho, s_L, s_R into their slots of the
// A_I/A_O/S scalar array d_sc ([P][per]).
// With d_v non-null, also the V commitment inputs from pi ([P][k] u32):
// d_v, d_g [P][2k] (values 1..k and pi + 1; gamma_0..2k-1) and d_gx_half [P]
// = gamma_2k / 2, in the same launch.
int draws_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint64_t* d_tmpl, uint32_t seed_len,
              uint32_t per, uint32_t* d_gamma, uint32_t* d_sc, const uint32_t* d_pi = nullptr,
              uint32_t* d_v = nullptr, uint32_t* d_g = nullptr, uint32_t* d_gx_half = nullptr);
void draw_template(const perm::Seed& seed, uint64_t tmpl[7]);

// The V commitment inputs from a caller's values (k_v_inputs), after draws_dev
// without d_v on the same stream: d_v [P][nv] = d_src[p * src_stride + index(j)]
// (canonical scalars; src_stride 0: one array shared by the call's proofs),
// with index(j) = j for the first n_id entries and d_perm[p][j - n_id] ([P][nv -
// n_id] u32, each a bijection) after them, or j throughout without a d_perm;
// d_g [P][nv] = the drawn gamma_0..nv-1 or, when d_gammas ([P][nv]) is non-null,
// the caller's, which then replace d_gamma's ([P][nv + 1]) too; d_gx_half [P]
// = gamma_nv / 2.  (Two-half shuffle: cards, stride k, perms, n_id = k; deck
// circuit: the call's deck, stride 0, perms, n_id = 0; caller-defined circuit:
// v, stride m_in, no perm.)
int v_inputs_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_src, uint32_t src_stride,
                 const uint32_t* d_perm, uint32_t n_id, const uint32_t* d_gammas, uint32_t* d_gamma, uint32_t* d_v,
                 uint32_t* d_g, uint32_t* d_gx_half);

// The witness a_L, a_R, a_O of every proof (x = x_perm [P] canonical, pi
// [P][k]) into their slots of d_sc.  With d_vals ([P][2k] canonical, d_v
// above) both chains take their values from it instead of 1..k and pi + 1
// (k_witness_cards; d_pi is not read).
int witness_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_pi, const uint32_t* d_x,
                uint32_t per, uint32_t* d_sc, const uint32_t* d_vals = nullptr);

// The deck circuit (perm.h build_deck).  witness_deck_dev (k_witness_deck):
// a_L, a_R, a_O of the one chain over d_vals ([P][k], d_v above) into their
// slots of d_sc, for k <= DECK_WITNESS_DEV_MAX; the host witness
// (perm::witness_deck) beyond.
constexpr uint32_t DECK_WITNESS_DEV_MAX = perm::chain_witness_dev_max(1);
int witness_deck_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_vals, const uint32_t* d_x,
                     uint32_t per, uint32_t* d_sc);

// A caller-defined circuit (host/circuit.h).
// witness_program_dev (k_witness_program): every proof's workgroup interprets
// C.program over its own values (d_vals [P][m_in], d_aux [P][n_aux], d_x [P],
// canonical): a_L, a_R, a_O into their slots of d_sc, and into fail[p] (pinned
// host memory, valid after the next ctx_sync) 1 + the first assert that does
// not hold, or 0.  The kernel is chosen by the wires' size and the circuit's
// TILED flag (circuit::witness_wide): k_witness_program_wide keeps them in the
// workspace "wp_wires", which prove_wipe zeroes; no size is refused.
int witness_program_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_vals,
                        const uint32_t* d_aux, const uint32_t* d_x, uint32_t per, uint32_t* d_sc, uint32_t* fail,
                        const uint32_t* d_pub = nullptr,  // (d_pub [P][n_pub] canonical: the public inputs)
                        bool derive_late = false);
// derive_late (aux derived from the circuit's hints, not a caller's): on a
// circuit with late hints the k_witness_program*_late kernels run, which
// evaluate each late hint where its gate is reached and never read its slot of
// d_aux (d_aux holds the early hints' values; not read at all when every hint
// is late).  Without it, and on every other circuit, d_aux is read as given.
// hint_aux_dev (k_hint_aux): the auxiliary values of a circuit with hints
// (C.program->hints), one lane per (proof, hint), from d_vals [P][m_in] and
// d_pub [P][n_pub] into d_aux [P][n_aux] (canonical), which witness_program_dev
// then reads as a caller's.  Enqueued on ctx's stream; d_aux is secret (the
// prover keeps it in "pb_aux_hint", which prove_wipe zeroes).
int hint_aux_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t P, const uint32_t* d_vals, const uint32_t* d_pub,
                 uint32_t* d_aux);
