// The prover's inputs and the built-in circuits' witnesses on the device
// (witness.hip).
#pragma once
#include "ctx.h"
#include "host/perm.h"

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
