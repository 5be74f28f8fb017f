// Batch verification on the device (verify_dev.hip, verify_scalars.hip).
#pragma once
#include <stdint.h>

#include <vector>

#include "ctx.h"
#include "host/perm.h"

// Per-proof verifier record: [12 + lg] canonical scalars (8 words each).
// The verifier needs no inverse (DESIGN.md §5 "No inversions"): every
// proof's check is scaled by F = (u_0 .. u_{lg-1})^2 y^(n_p - 1), so y^-i,
// s_0 = prod u_j^-1 and u_j^-2 become y^(n_p-1-i), prod u_j and
// prod_{k != j} u_k^2.
#define VREC_XPERM 0
#define VREC_Y 1
#define VREC_Z 2
#define VREC_X 3
#define VREC_W 4
#define VREC_R 5
#define VREC_A 6
#define VREC_B 7
#define VREC_THAT 8
#define VREC_TAUX 9
#define VREC_MU 10
#define VREC_WT 11  // (unused: the weight is made by k_verify_consts)
#define VREC_U 12   // u_j (lg)
inline uint32_t vrec_n(const perm::Circuit& C) { return VREC_U + C.lg; }
// proof points per proof in MSM order: V_0..V_{m-1}, A_I, A_O, S, T1 T3 T4
// T5 T6, L_0.., R_0..
inline uint32_t vpts_n(const perm::Circuit& C) { return C.m + 8 + 2 * C.lg; }

// Replays `count` transcripts on the device, one per 16-lane group
// (k_verify_replay_g, then k_verify_reduce and k_verify_replay_post): d_proofs [count][proof_len] and d_V [count][m][32] on
// the device; init = the 52-word transcript state every proof shares (the
// label's Transcript::new and perm::transcript_prefix; verify_init_state).
// Writes d_rec (the challenges and the proof's scalars), r_out ([count][32],
// the t-check weight challenges) and bad ([count] u32, nonzero where a point
// is the identity encoding, a scalar is not canonical or a challenge is
// zero).  r_out and bad may be pinned host memory (written in place).
// d_pub (C.n_pub > 0): [count][n_pub][8] words, each proof's public inputs,
// absorbed as "pub" messages before its V_0.
int verify_replay_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t count, const uint32_t* d_init,
                      const uint32_t* d_proofs, const uint32_t* d_V, uint32_t* d_rec, uint32_t* r_out, uint32_t* bad,
                      const uint32_t* d_pub = nullptr);
// Decompresses the proof points of proofs [p0, p1) (p1 = ~0u: count) of the
// uploaded proofs / V into d_tbl ([count * vpts_n] Niels rows in MSM order);
// *d_bad = the smallest index of an undecodable encoding (set to ~0 by the
// caller first).  Independent of the replay (launched on another stream, one
// launch per upload chunk).
// [jlo, jlo + jn): the points of each proof to decode (V_0..V_{m-1} are
// points 0..m-1, the proof's own m..npt-1; default all of them).
// d_pdec (optional): [count] words, set nonzero by the caller first; proof
// p's word is cleared if one of its points does not decode.
int verify_decompress_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t count, const uint32_t* d_proofs,
                          const uint32_t* d_V, uint32_t* d_tbl, unsigned long long* d_bad, uint32_t p0 = 0,
                          uint32_t p1 = ~0u, uint32_t jlo = 0, uint32_t jn = ~0u, uint32_t* d_pdec = nullptr);
// The 52-word shared transcript prefix for verify_replay_dev.
void verify_init_state(const perm::Circuit& C, const uint8_t* label, size_t llen, uint32_t out[52]);
// out[i] = sum over the nb blocks (stride words apart) of block[b][i], i < n
// (the generator scalars of a gathered sliced verification).
int verify_sum_blocks_dev(bpp_ctx* ctx, uint32_t nb, uint32_t n, const uint32_t* d_blocks, uint32_t stride,
                          uint32_t* d_out);
// A mixed batch (bpp_verify_groups): up to VG_MAX groups of different
// circuits.  VerifyGroupTab: group g's generator block blk ([2 n_p + 2][8]
// words: G, H, B, Bb, the head of its context's "pv_s") and its n_p.
// VerifyGatherTab: segments of 16-byte units, segment s = pre[s + 1] - pre[s]
// units from src[s] to dst[s] (two per group: its proof-point scalars and its
// decompressed points).  Both are kernel arguments: nothing is uploaded.
#define VG_MAX BPP_VERIFY_GROUPS_MAX
struct VerifyGroupTab {
  uint32_t n = 0;
  struct {
    const uint32_t* blk;
    uint32_t n_p;
  } g[VG_MAX];
};
struct VerifyGatherTab {
  uint32_t n = 0;
  uint64_t pre[2 * VG_MAX + 1] = {0};
  const uint4* src[2 * VG_MAX];
  uint4* dst[2 * VG_MAX];
};
// d_out [2 n_max + 2][8] = the groups' generator scalars summed slot by slot
// (out[i] and out[n_max + i] over the groups with i < n_p, the two bases over
// all; mod l, canonical in and out), then the gather.  n_p <= n_max for every
// group (BPP_ERR_ARG otherwise, before any launch).
int verify_merge_groups_dev(bpp_ctx* ctx, const VerifyGroupTab& tab, uint32_t n_max, uint32_t* d_out,
                            const VerifyGatherTab& gt);
// k_verify_consts (each proof's weight perm::batch_weight(seed, first + p,
// r_p) and its constants) + k_verify_scalars + k_verify_merge over device
// records (verify_scalars.hip).  seed: 8 words, may be pinned host memory.  d_pub
// (C.n_pub > 0, k_verify_scalars_pub): [count][n_pub][8] words, canonical.
int verify_scalars_dev_rec(bpp_ctx* ctx, const perm::Circuit& C, uint32_t count, const uint32_t* d_rec,
                           const uint32_t* seed, uint64_t first, uint32_t* d_sc, const uint32_t* d_pub = nullptr);
// The batch verifier's MSM scalars for `count` proofs (k_verify_consts +
// k_verify_scalars + k_verify_merge): rec = [count][12 + lg] canonical
// scalars (x_perm, y, z, x, w, r, a, b, t_hat, tau_x, mu, -, u_j..); proof p
// is weighted by perm::batch_weight(seed, first + p, r_p); d_sc (device)
// receives the 2 n_p + 2 merged generator scalars then count x (m + 8 + 2 lg)
// weighted proof-point scalars, every proof's check scaled by
// (prod u_j)^2 y^(n_p - 1) (above).
int verify_scalars_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t count, const std::vector<uint32_t>& rec,
                       const uint8_t seed[32], uint64_t first, uint32_t* d_sc);
// Per-proof verdicts (bpp_perm_verify_batch_each).  Term lists of proofs [p0,
// p0 + M) for the multi-MSM engine: d_scal / d_idx [M][NG + npt] (generator
// scalars d_gen[p][NG] on generator slots of a set of gn generators, then the
// proof-point scalars d_sv[NG + p npt ..) on points n0 + p npt + j), d_off
// [M + 1] = m (NG + npt); zero scalars where d_rbad[p] (replay-rejected).
int verify_each_terms_dev(bpp_ctx* ctx, const perm::Circuit& C, uint32_t gn, uint32_t n0, uint32_t p0, uint32_t M,
                          const uint32_t* d_gen, const uint32_t* d_sv, const uint32_t* d_rbad, uint32_t* d_scal,
                          uint32_t* d_idx, uint32_t* d_off);
// ok[p] = d_enc[p] is 0^32 and d_pdec[p] != 0 and d_rbad[p] == 0, one byte per
// proof (ok may be pinned host memory, written in place).
int verify_each_verdict_dev(bpp_ctx* ctx, uint32_t count, const uint32_t* d_enc, const uint32_t* d_pdec,
                            const uint32_t* d_rbad, uint8_t* ok);
