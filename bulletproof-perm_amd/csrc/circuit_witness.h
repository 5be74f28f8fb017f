// The circuit interpreter on the device (circuit_witness.hip): the witness of
// a caller-defined circuit (host/circuit.h) and the auxiliary values its hints
// derive.
#pragma once
#include "ctx.h"
#include "host/perm.h"

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
