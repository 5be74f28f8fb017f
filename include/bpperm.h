/*
 * bpperm.h — C ABI of the MI355X-native Bulletproof permutation hot path.
 *
 * Drop-in boundary for the three operations the reference
 * (ercembu/bulletproof-perm, Rust crate `bp-perm`) delegates to
 * curve25519-dalek-ng 4.1.1 / bulletproofs 4.0.0 / merlin 3.0.0:
 *
 *   Ristretto MSM      `VartimeMultiscalarMul::vartime_multiscalar_mul`
 *                      bp-perm/src/circuit_lib.rs:187,202,216,363,374,385,396,
 *                      407,498,504,509,525,535,552,568
 *   Pedersen commit    `PedersenGens::commit` weights.rs:58-61,
 *                      vector commitments A_I / A_O / S circuit_lib.rs:187-229
 *   point codec        `RistrettoPoint::compress` circuit_lib.rs:231-233,
 *                      `CompressedRistretto::decompress` circuit_lib.rs:532
 *   inner-product arg  `InnerProductProof::{create,verify}` (bulletproofs
 *                      4.0.0; hook fields ACEssentials.G_factors/H_factors,
 *                      circuit_lib.rs:62-63)
 *   transcript         merlin `Transcript` + TranscriptProtocol,
 *                      transcript_protocol.rs:26-67
 *   AC proof           `ACProof::ArithmeticCircuitProof`, circuit_lib.rs:139-585
 *
 * Conventions (inherited from the reference):
 *   - every function returns an int status (BPP_OK = 0); nothing unwinds;
 *   - scalars are 32-byte little-endian canonical integers mod l
 *     (dalek `Scalar::as_bytes`); points are 32-byte compressed ristretto255
 *     (dalek `CompressedRistretto`);
 *   - buffers are caller-owned; the library keeps no pointer after a call
 *     returns, except to the opaque objects it creates;
 *   - a context is bound to one GPU and one HIP stream; calls on one context
 *     must not overlap (the reference is single-threaded, `&mut Transcript`).
 *   - length mismatches are BPP_ERR_LEN where dalek panics (size-hint
 *     asserts); an undecodable point is BPP_ERR_DECOMPRESS where the
 *     reference `unwrap()`s (circuit_lib.rs:532); a failed check is
 *     BPP_ERR_VERIFY where the reference returns
 *     `ProofError::VerificationError` (circuit_lib.rs:519,543).
 */
#ifndef BPPERM_H
#define BPPERM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes.  No C++ exception leaves the library: a host allocation that
 * cannot be met returns BPP_ERR_NOMEM, any other internal exception
 * BPP_ERR_DEVICE (text in bpp_ctx_last_error when the call has a context). */
enum {
  BPP_OK = 0,
  BPP_ERR_ARG = 1,
  BPP_ERR_LEN = 2,
  BPP_ERR_DECOMPRESS = 3,
  BPP_ERR_NONCANONICAL = 4,
  BPP_ERR_DEVICE = 5,
  BPP_ERR_VERIFY = 6,
  BPP_ERR_NOMEM = 7,
  BPP_ERR_CALLBACK = 8, /* a caller's transcript hook returned nonzero */
};

typedef struct bpp_ctx bpp_ctx;
typedef struct bpp_points bpp_points;

/* ------------------------------------------------------------- context */
int bpp_ctx_create(int device, bpp_ctx** out);
void bpp_ctx_destroy(bpp_ctx* ctx);
/* Last error text for this context ("" if none). */
const char* bpp_ctx_last_error(const bpp_ctx* ctx);
/* The hipStream_t every kernel of this context is launched on. */
void* bpp_ctx_stream(bpp_ctx* ctx);
/* Per-kernel timing with HIP events on the context stream (0 = off). */
int bpp_ctx_profile(bpp_ctx* ctx, int enable);
/* Accumulated time (ms) and launch count of a named kernel stage
 * ("msm_accumulate", "msm_reduce", "msm_count", "msm_scatter", ...). */
int bpp_ctx_profile_get(bpp_ctx* ctx, const char* stage, double* ms, uint64_t* launches);
void bpp_ctx_profile_reset(bpp_ctx* ctx);
/* Algorithmic work issued on this context (and its child streams) since the
 * last reset, counted at launch time: "msm_terms" (scalar-point terms of every
 * MSM and Pedersen commitment), "madds" (mixed additions of a table point:
 * direct-table MSMs count every window of every term), "padds" (additions of
 * two extended points in trees and bucket reductions), "msm_launches", and
 * the direct-table kernel's own "dt_terms" / "dt_madds" / "dt_launches".  The
 * roofline of the proof path (96 B x terms) reads these.
 * "prove_stage_bytes": the bytes a prover batch staged and uploaded for its
 * draws and inputs (templates, pi, v, aux, gammas, pub). */
int bpp_ctx_work_get(bpp_ctx* ctx, const char* name, uint64_t* value);
void bpp_ctx_work_reset(bpp_ctx* ctx);

/* Opt-in host-process tuning (process-wide, so never done implicitly):
 * BPP_TUNE_MALLOC fixes glibc's mmap threshold at 64 MB, disables heap
 * trimming and pads arena growth by 64 MB, which keeps the prover's
 * per-batch host vectors in the arenas
 * (measured in a host profile of 8 batches in flight).
 * BPP_TUNE_HW_QUEUES asks HIP for 8 hardware queues per process
 * (GPU_MAX_HW_QUEUES=8 unless the caller set it): a prover keeping many
 * batches in flight, one context and stream each, needs more than HIP's
 * default 4.  HIP reads the variable once, when it starts, so this flag must
 * come before the first bpp_ctx_create and any other HIP use in the process.
 * BPP_ERR_ARG for unknown flags. */
#define BPP_TUNE_MALLOC 1u
#define BPP_TUNE_HW_QUEUES 2u
int bpp_host_tuning(uint32_t flags);
/* Threads of the library's host pool (transcripts, scalar bookkeeping),
 * calling threads included: BPP_HOST_THREADS, else a quarter of this
 * process's share of the granted CPUs (cgroup quota / LOCAL_WORLD_SIZE),
 * at most 4. */
uint32_t bpp_host_threads(void);

/* Device memory helpers, so callers can stage inputs resident in HBM. */
int bpp_dev_alloc(bpp_ctx* ctx, size_t bytes, void** dptr);
int bpp_dev_free(bpp_ctx* ctx, void* dptr);
int bpp_memcpy_htod(bpp_ctx* ctx, void* dst, const void* src, size_t bytes);
int bpp_memcpy_dtoh(bpp_ctx* ctx, void* dst, const void* src, size_t bytes);
int bpp_synchronize(bpp_ctx* ctx);

/* ------------------------------------------------ resident point tables */
/* Decompress n 32-byte encodings into a table kept in HBM.
 * BPP_ERR_DECOMPRESS if any encoding is invalid (*bad_index set when
 * bad_index != NULL).  Replaces CompressedRistretto::decompress. */
int bpp_points_decompress(bpp_ctx* ctx, const uint8_t* enc, size_t n, bpp_points** out, size_t* bad_index);
/* n points RistrettoPoint::from_uniform_bytes(64 bytes each), on the GPU. */
int bpp_points_from_uniform(bpp_ctx* ctx, const uint8_t* bytes64, size_t n, bpp_points** out);
/* Compress every point of the table (RistrettoPoint::compress). */
int bpp_points_compress(bpp_ctx* ctx, const bpp_points* pts, uint8_t* out);
size_t bpp_points_len(const bpp_points* pts);
void bpp_points_destroy(bpp_points* pts);

/* ------------------------------------------------------------------ MSM */
/* out = sum_i scalars[i] * points[i]; host scalars, host compressed points.
 * `RistrettoPoint::vartime_multiscalar_mul(scalars, points).compress()`. */
int bpp_msm(bpp_ctx* ctx, const uint8_t* scalars, const uint8_t* points, size_t n, uint8_t out[32]);
/* Same over the first n points of a resident table; host scalars. */
int bpp_msm_table(bpp_ctx* ctx, const uint8_t* scalars, const bpp_points* tbl, size_t n, uint8_t out[32]);
/* Same with the scalars already resident in HBM (n x 32 bytes at d_scalars,
 * canonical).  The throughput entry point used by bench.py. */
int bpp_msm_table_dev(bpp_ctx* ctx, const void* d_scalars, const bpp_points* tbl, size_t n, uint8_t out[32]);
/* Window-partitioned MSM for multi-GPU: computes the partial sum over
 * windows [w_begin, w_end) of the signed radix-2^c decomposition the
 * library picks for size n (bpp_msm_windows reports c and the window
 * count).  Partial results are raw extended points (128 bytes) so that
 * partials from different GPUs can be added exactly (bpp_point_add_raw). */
int bpp_msm_windows(size_t n, uint32_t* c, uint32_t* windows);
int bpp_msm_table_dev_partial(bpp_ctx* ctx, const void* d_scalars, const bpp_points* tbl, size_t n,
                              uint32_t w_begin, uint32_t w_end, uint8_t partial[128]);
/* Asynchronous single MSMs over a resident table, for a stream of
 * independent MSMs (e.g. successive batch verifications): submit enqueues
 * the whole device pipeline of one MSM (windows [w_begin, w_end); w_end = 0
 * means all windows) on its own stream and returns at once; collect waits
 * for that MSM, runs its host window combine and returns the compressed
 * result (`out`, full MSMs) and/or the raw 128-byte partial (`partial`, as
 * bpp_msm_table_dev_partial).  At most BPP_MSM_INFLIGHT MSMs may be
 * outstanding (submit fails with BPP_ERR_ARG otherwise), so the device runs
 * MSM i+1's digit sort beside MSM i's latency-bound bucket reduction while
 * the host combines MSM i-1's windows (two in flight measured best).  d_scalars must stay valid until
 * collect; each outstanding MSM needs its own scalar buffer contents.
 * Same-result guarantee: collect(submit(s)) == bpp_msm_table_dev(s). */
#define BPP_MSM_INFLIGHT 4
int bpp_msm_submit(bpp_ctx* ctx, const void* d_scalars, const bpp_points* tbl, size_t n, uint32_t w_begin,
                   uint32_t w_end, uint64_t* ticket);
int bpp_msm_collect(bpp_ctx* ctx, uint64_t ticket, uint8_t out[32], uint8_t partial[128]);
/* The same with host scalars (the shape of the reference's
 * vartime_multiscalar_mul(scalars, points), circuit_lib.rs:187): the n x 32
 * bytes are copied to the device on the MSM's own stream, so in a stream of
 * submits the upload of one MSM overlaps the others' kernels.  From pinned memory (bpp_host_alloc)
 * the copy is a direct DMA; pageable memory goes through a staging copy
 * first (host memcpy inside the call).  h_scalars must stay valid and
 * unchanged until collect. */
int bpp_msm_submit_host(bpp_ctx* ctx, const void* h_scalars, const bpp_points* tbl, size_t n, uint32_t w_begin,
                        uint32_t w_end, uint64_t* ticket);
/* Pinned (page-locked) host memory for bpp_msm_submit_host and
 * bpp_perm_verify_* inputs: the library recognises these buffers (a range
 * inside one goes up by direct DMA) from its own registry; other host memory
 * is looked up in the HIP runtime (memory the caller pinned itself also goes
 * by DMA) and otherwise staged as pageable. */
int bpp_host_alloc(bpp_ctx* ctx, size_t bytes, void** hptr);
int bpp_host_free(bpp_ctx* ctx, void* hptr);
/* Sum raw extended partial points (count x 128 bytes) and compress.
 * BPP_ERR_ARG for a partial whose Z coordinate is zero (not a point: e.g. an
 * all-zero buffer a failed rank never wrote). */
int bpp_partials_finish(const uint8_t* partials, size_t count, uint8_t out[32]);
/* Host batch encoding of doubled points: out[i] = compress(2 * P_i) for raw
 * extended points P_i (count x 128 bytes), one field inversion per call
 * instead of one inverse square root per point (the prover computes C / 2
 * from halved scalars and encodes C this way).  Replaces the per-point
 * RistrettoPoint::compress of the reference's commitments and IPA L/R
 * (circuit_lib.rs:231-233) where batches are small; host-only. */
int bpp_points_double_compress(const uint8_t* raw, size_t count, uint8_t* out);
/* count independent MSMs; MSM j covers terms [offsets[j], offsets[j+1]) of
 * `scalars` (32 bytes each) and `point_idx` (indices into tbl). */
int bpp_msm_batch(bpp_ctx* ctx, size_t count, const uint64_t* offsets, const uint8_t* scalars,
                  const uint32_t* point_idx, const bpp_points* tbl, uint8_t* out);

/* ----------------------------------------------------------- generators */
typedef struct bpp_gens bpp_gens;
/* BulletproofGens::new(n, 1) (G, H from the SHAKE256 GeneratorsChain) plus
 * PedersenGens::default() (B, B_blinding), generated on the GPU and kept
 * resident with fixed-base tables for B and B_blinding.
 * Reference: lib.rs:163 (BulletproofGens::new), weights.rs:58 (PedersenGens). */
int bpp_gens_create(bpp_ctx* ctx, size_t n, bpp_gens** out);
/* Explicit generators (the reference's test draws random G, H and a random
 * PedersenGens, lib.rs:164-180).  G_enc, H_enc: n x 32 bytes. */
int bpp_gens_from_points(bpp_ctx* ctx, const uint8_t* G_enc, const uint8_t* H_enc, size_t n,
                         const uint8_t B_enc[32], const uint8_t Bb_enc[32], bpp_gens** out);
size_t bpp_gens_len(const bpp_gens* g);
/* Compressed G[0..n), H[0..n), B, B_blinding: (2n + 2) x 32 bytes. */
int bpp_gens_export(bpp_ctx* ctx, const bpp_gens* g, uint8_t* out);
void bpp_gens_destroy(bpp_gens* g);

/* ------------------------------------------------- Pedersen commitments */
/* V_j = v_j * B + gamma_j * B_blinding for j < m (PedersenGens::commit,
 * weights.rs:58-61), fixed-base on the GPU. */
int bpp_pedersen_commit_batch(bpp_ctx* ctx, const bpp_gens* g, const uint8_t* v, const uint8_t* gamma, size_t m,
                              uint8_t* out);
/* blind * B_blinding + <a, G[0..n)> (+ <b, H[0..n)> when b != NULL):
 * A_I / A_O / S of circuit_lib.rs:187-229. */
int bpp_vec_commit(bpp_ctx* ctx, const bpp_gens* g, const uint8_t blind[32], const uint8_t* a, const uint8_t* b,
                   size_t n, uint8_t out[32]);

/* ------------------------------------------------------ Merlin transcript */
typedef struct bpp_transcript bpp_transcript;
/* merlin 3.0.0 Transcript::new(label); byte-exact (transcript_protocol.rs). */
bpp_transcript* bpp_transcript_new(const uint8_t* label, size_t len);
bpp_transcript* bpp_transcript_clone(const bpp_transcript* t);
void bpp_transcript_destroy(bpp_transcript* t);
int bpp_transcript_append_message(bpp_transcript* t, const uint8_t* label, size_t llen, const uint8_t* msg,
                                  size_t mlen);
int bpp_transcript_append_u64(bpp_transcript* t, const uint8_t* label, size_t llen, uint64_t x);
int bpp_transcript_challenge_bytes(bpp_transcript* t, const uint8_t* label, size_t llen, uint8_t* out, size_t n);
/* challenge_scalar: 64 challenge bytes -> Scalar::from_bytes_mod_order_wide
 * (transcript_protocol.rs:62-67). */
int bpp_transcript_challenge_scalar(bpp_transcript* t, const uint8_t* label, size_t llen, uint8_t out[32]);

/* ------------------------------------------------- scalar helpers (host) */
/* The caller-side scalar algebra the IPA's factors need: Scalar::invert
 * (circuit_lib.rs:274; BPP_ERR_ARG for zero) and x^0 .. x^(n-1) (util.rs:
 * 138-157 exp_iter; e.g. H_factors = powers of y^-1).  Canonical 32-byte
 * scalars in and out (BPP_ERR_NONCANONICAL otherwise). */
int bpp_scalar_invert(const uint8_t x[32], uint8_t out[32]);
int bpp_scalar_powers(const uint8_t x[32], size_t n, uint8_t* out);

/* ------------------------------------------------ inner-product argument */
/* bulletproofs 4.0.0 InnerProductProof::create over G[0..n), H[0..n) of g
 * (n a power of two, n <= bpp_gens_len): L_out, R_out receive log2(n)
 * compressed points each; G_factors / H_factors may be NULL (all ones).
 * Q may be any point: it is written into g's spare generator slot for the
 * call (BPP_ERR_DECOMPRESS if it does not decode), so concurrent
 * bpp_ipa_prove calls on one g (from several contexts) run one at a time.
 * On that path the kernels read a, b and the factors in place from ctx's
 * pinned host buffers (copied in at the call; the copies of a and b are
 * zeroed before it returns, on error paths too); the folded a, b stay in
 * ctx's device workspaces (the entropy prover's wipe zeroes them). */
int bpp_ipa_prove(bpp_ctx* ctx, const bpp_gens* g, bpp_transcript* tr, const uint8_t Q[32], const uint8_t* G_factors,
                  const uint8_t* H_factors, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* L_out,
                  uint8_t* R_out, uint8_t a_out[32], uint8_t b_out[32]);
/* InnerProductProof::verify: BPP_OK or BPP_ERR_VERIFY.  One GPU MSM of
 * 2n + 2log2(n) + 2 terms checked against the identity. */
int bpp_ipa_verify(bpp_ctx* ctx, const bpp_gens* g, bpp_transcript* tr, size_t n, const uint8_t* G_factors,
                   const uint8_t* H_factors, const uint8_t P[32], const uint8_t Q[32], const uint8_t* L,
                   const uint8_t* R, const uint8_t a[32], const uint8_t b[32]);

/* The same two calls over the CALLER's transcript (north_star: the bp-perm
 * crate keeps its merlin::Transcript; bulletproofs'
 * InnerProductProof::create(transcript: &mut Transcript, ..) and verify).
 * The library never owns the transcript: it calls back, on the calling
 * thread and in this order, exactly where bulletproofs 4.0.0 touches it
 * (transcript_protocol.rs:26-67):
 *   append_message("dom-sep", "ipp v1"), append_message("n", le64(n))
 *                                  -- innerproduct_domain_sep(n)
 *   per round j < log2(n):
 *     append_message("L", L_j), append_message("R", R_j)
 *                                  -- append_point / validate_and_append_point
 *     challenge_bytes("u", 64 B)   -- challenge_scalar("u"): the library
 *                                     reduces the 64 bytes mod l (from_bytes_mod_order_wide)
 * Labels are exactly those byte strings (no NUL counted in llen).  The
 * verifier refuses an identity L_j / R_j (BPP_ERR_VERIFY) before appending
 * it, as validate_and_append_point does.  A hook returning nonzero aborts
 * the call with BPP_ERR_CALLBACK (the transcript is then in an unspecified
 * state).  bpp_ipa_prove / bpp_ipa_verify are these with the library's own
 * Merlin (bpp_transcript) behind the hooks. */
typedef struct bpp_transcript_hooks {
  void* user;
  int (*append_message)(void* user, const uint8_t* label, size_t llen, const uint8_t* msg, size_t mlen);
  int (*challenge_bytes)(void* user, const uint8_t* label, size_t llen, uint8_t* out, size_t n);
} bpp_transcript_hooks;
int bpp_ipa_prove_cb(bpp_ctx* ctx, const bpp_gens* g, const bpp_transcript_hooks* tr, const uint8_t Q[32],
                     const uint8_t* G_factors, const uint8_t* H_factors, const uint8_t* a, const uint8_t* b, size_t n,
                     uint8_t* L_out, uint8_t* R_out, uint8_t a_out[32], uint8_t b_out[32]);
int bpp_ipa_verify_cb(bpp_ctx* ctx, const bpp_gens* g, const bpp_transcript_hooks* tr, size_t n,
                      const uint8_t* G_factors, const uint8_t* H_factors, const uint8_t P[32], const uint8_t Q[32],
                      const uint8_t* L, const uint8_t* R, const uint8_t a[32], const uint8_t b[32]);

/* ------------------------------------------- permutation proof (sound) */
/* Arithmetic-circuit proof that the second half of v = [1..k, pi(1..k), x]
 * is a permutation of the first (ACProof::ArithmeticCircuitProof,
 * circuit_lib.rs:139-585 over the circuit of weights.rs:26-204), in sound
 * form (SURVEY.md §2.2 defects fixed; DESIGN.md "Protocol").  Gates are
 * padded to n_p = next_pow2(2k) <= bpp_gens_len(g).  Every entry point takes
 * 2 <= k <= 2^20 (BPP_ERR_ARG otherwise).
 *
 * Proof bytes (bpp_perm_proof_len(k)): A_I A_O S T1 T3 T4 T5 T6 | tau_x mu
 * t_hat | L_0 R_0 .. L_{lg-1} R_{lg-1} | a b.  The 2k+1 Pedersen
 * commitments V go to V_out (public inputs, 32 bytes each).  All prover
 * randomness comes from the seed, the injected stand-in for the reference's
 * thread_rng (circuit_lib.rs:175): pi from SHAKE256("bpperm-prove" || seed)
 * (Fisher-Yates, one u64 per step), blinding scalar j (order gamma[2k+1],
 * alpha, beta, rho, s_L[n_p], s_R[n_p], tau[5]) from the first 64 bytes of
 * SHAKE256("bpperm-prove-sc" || seed || le32 j), reduced mod l. */
size_t bpp_perm_proof_len(uint32_t k);
int bpp_perm_prove(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, uint64_t seed, const uint8_t* label, size_t llen,
                   uint8_t* proof_out, uint8_t* V_out, uint32_t* perm_out);
int bpp_perm_prove_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint64_t* seeds,
                         const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out);
/* The u64 seeds above are deterministic TEST hooks (64 bits of entropy, so
 * a guessable seed reveals the witness).  Production proofs: 32 bytes of
 * entropy per proof from the caller (seeds32, count x 32 B), or seeds32 =
 * NULL to draw them from the OS CSPRNG (getrandom), as the reference draws
 * from thread_rng (circuit_lib.rs:175, weights.rs:39,59).  The draws are
 * those above with the 32-byte seed32 in place of the 8-byte seed.
 * Secret lifetime: after the batch the library zeroes what it kept of it --
 * the device workspaces holding draws, witness, blindings and the l / r
 * vectors, the staged draw templates, pi and (k > 768) host-path witness,
 * the T-commitment inputs, and the calling thread's reused prover states and
 * permutations; with BPP_PROVE_STREAMS > 1 each sub-batch thread does the same
 * on its child context before it exits (the caller's own seeds32 buffer is
 * the caller's to wipe). */
int bpp_perm_prove_batch_entropy(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* seeds32,
                                 const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out);
/* Proves a CALLER-SUPPLIED shuffle: the caller's deck, permutation and
 * (optionally) the blindings of commitments it has already published -- the
 * direction of the reference, whose deck is an explicit vector handed to
 * commit_variables and create_a (weights.rs:58-113).  Per proof p:
 *   cards   count x k x 32 B: the deck, canonical scalars (proof-major);
 *   perms   count x k u32: output slot i holds cards[perm[i]];
 *   gammas  NULL, or count x 2k x 32 B: the blindings of V_0..V_2k-1.
 * V_0..V_{k-1} commit to cards[i], V_k..V_{2k-1} to cards[perm[i]] and V_2k
 * to the transcript challenge x_perm, as above.  The circuit proves
 * prod (v_i - x) = prod (v'_i - x), i.e. that the two halves are equal as
 * MULTISETS: cards may be any canonical scalars, 0 and l - 1 and repeated
 * values included, and with repeated values the proof says nothing about
 * which of the equal cards went where.
 * Proof format, transcript order, bpp_perm_proof_len and the V_out layout are
 * those of the other provers; the proofs verify with bpp_perm_verify /
 * bpp_perm_verify_batch unchanged.
 * Randomness: seeds32 as bpp_perm_prove_batch_entropy (count x 32 B, or NULL
 * for the OS CSPRNG); blinding scalar j is the same indexed draw in the same
 * order; supplied gammas replace draws 0..2k-1, while gamma_2k, alpha, beta,
 * rho, s_L, s_R and tau stay drawn; no pi stream is read.  With cards = 1..k,
 * perms = the permutation bpp_perm_prove_batch_entropy derives from the same
 * seeds and gammas = NULL, proofs and V equal that call's bytes.
 * Checked before any device work and before any output byte is written:
 * a perm that is not a bijection on [0, k) -> BPP_ERR_ARG; a card or gamma
 * >= l -> BPP_ERR_NONCANONICAL (the witness is checked first: it needs
 * neither ctx nor g); then the k / g / null checks of the other provers.
 * Secret lifetime: always that of bpp_perm_prove_batch_entropy; the staged
 * and uploaded cards, perms and gammas are part of what is zeroed (the
 * caller's own arrays are the caller's to wipe). */
int bpp_perm_prove_shuffle_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* cards,
                                 const uint32_t* perms, const uint8_t* gammas, const uint8_t* seeds32,
                                 const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out);
/* Test hook for the secret lifetime above: the number of nonzero bytes left
 * in what the last bpp_perm_prove_batch_entropy zeroed on ctx and its child
 * contexts (device workspaces, pinned buffers and staging spans, including
 * the sub-batch contexts of BPP_PROVE_STREAMS > 1 and the host-witness
 * staging of k > 768).  Synchronises ctx. */
int bpp_debug_secret_residue(bpp_ctx* ctx, uint64_t* nonzero_bytes);
/* BPP_OK or BPP_ERR_VERIFY (ProofError::VerificationError). One GPU MSM. */
int bpp_perm_verify(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, const uint8_t* label, size_t llen,
                    const uint8_t* proof, size_t proof_len, const uint8_t* V);
/* Batch verification: all proofs' checks folded into ONE MSM (generator
 * scalars merged across proofs) with random weights w_p =
 * from_wide(SHAKE256("bp-perm-batch-wt" || seed || le64 p || r_p)[0..64]):
 * seed = 32 bytes of the verifier's own randomness (getrandom), mixed with
 * each proof's transcript challenge r_p as bulletproofs' r1cs batch verifier
 * mixes its rng into a TranscriptRng.  The transcripts are replayed on the
 * GPU and the whole batch runs with no host round trip (DESIGN.md §5 "Batch
 * weights", "No inversions"). */
int bpp_perm_verify_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* label,
                          size_t llen, const uint8_t* proofs, const uint8_t* V);
/* Batch verification that names the failing proofs: ok_out[p] (count bytes
 * of ordinary host memory) = 1 if proof p verifies, else 0 -- what
 * bpp_perm_verify returns for proof p alone.
 *   BPP_OK          every proof verifies; ok_out is all ones.
 *   BPP_ERR_VERIFY  at least one proof fails; ok_out is fully written.
 *   any other error ok_out is all zero (whenever it was given): no call
 *                   leaves a pass behind that it did not establish.
 * Arguments as bpp_perm_verify_batch, and ok_out == NULL with count > 0 is
 * BPP_ERR_ARG; all checked before any device work.  count == 0: BPP_OK,
 * nothing written.
 * A batch that passes costs what bpp_perm_verify_batch costs: the same
 * upload, replay and ONE merged MSM, no further launch or wait.  Only when
 * that check does not pass, every proof's own MSM (2 n_p + 2 generators +
 * its m + 8 + 2 log2 n_p points) runs over the scalars and decompressed
 * points the batch left on the device -- no second upload, replay,
 * decompression or scalar expansion -- in passes of at most 2^22 / terms
 * proofs (BPP_VERIFY_EACH_PROOFS=<n> overrides the proofs per pass), with one
 * more wait at the end (DESIGN.md §5 "Per-proof verdicts"). */
int bpp_perm_verify_batch_each(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* label,
                               size_t llen, const uint8_t* proofs, const uint8_t* V, uint8_t* ok_out);

/* ------------------------------------- public-deck shuffle proof (sound) */
/* The FIRST shuffle of a game starts from a deck every player knows.  These
 * entry points prove "V_0..V_{k-1} commit to a permutation of the PUBLIC deck
 * d_0..d_{k-1}" (V_k commits to the transcript challenge x_perm): k + 1
 * commitments instead of 2k + 1 and one product chain inside the proof -- the
 * deck's own product D = prod (d_i - x_perm) is computed by both sides -- so
 * n = k - 1 gates, Q = 2k rows, n_p = max(4, next_pow2(k - 1)) <=
 * bpp_gens_len(g) (64 for 52 cards, against 128).  The two-half statement
 * above remains the one for re-shuffling a deck that is already committed.
 *   deck    NULL (the cards 1..k), or k x 32 B canonical scalars, shared by
 *           every proof of the call.  Repeats, 0 and l - 1 are allowed;
 *           equality is as MULTISETS, as above.  A card >= l ->
 *           BPP_ERR_NONCANONICAL, in the verifiers too.
 *   perms   count x k u32: V_i commits to deck[perm[i]].
 *   gammas  NULL, or count x k x 32 B: the blindings of V_0..V_{k-1}.
 *   V_out / V   count x (k + 1) x 32 B.
 * Proof bytes (bpp_deck_proof_len(k); 800 at k = 52): the layout of
 * bpp_perm_proof_len with this circuit's lg = log2 n_p.
 * Transcript: Transcript(label), dom-sep("acp v1", n_p),
 * append_message("deck", SHAKE256("bpperm-deck" || le32 k || d_0 || .. ||
 * d_{k-1})[0..32]), V_0..V_{k-1}, challenge x_perm, V_k, A_I A_O S and on as
 * above.  The "deck" message binds the proof to the deck, and keeps a two-half
 * proof of k' cards and a deck proof of 2k' cards -- same commitment count,
 * n_p and byte length -- from verifying as each other.
 * Randomness: seeds32 as bpp_perm_prove_batch_entropy; indexed draws in the
 * order gamma[k + 1], alpha, beta, rho, s_L[n_p], s_R[n_p], tau[5] with this
 * circuit's n_p; supplied gammas replace draws 0..k-1; no pi stream is read.
 * Checks: those of bpp_perm_prove_shuffle_batch in its order, before any
 * device work and before any output byte is written -- a perm that is not a
 * bijection on [0, k) -> BPP_ERR_ARG; a deck card or gamma >= l ->
 * BPP_ERR_NONCANONICAL (neither needs ctx or g); then the k / g / null checks.
 * Secret lifetime: that of bpp_perm_prove_batch_entropy; the staged and
 * uploaded perms and gammas and the committed values are part of what is
 * zeroed and of what bpp_debug_secret_residue counts (the deck is public).
 * The verifiers mirror bpp_perm_verify, _verify_batch and _verify_batch_each
 * (the ok_out contract and count == 0 included).  The device witness covers
 * k <= 1536, the host witness beyond.  The multi-GPU job API takes two-half
 * proofs only. */
size_t bpp_deck_proof_len(uint32_t k);
int bpp_deck_prove_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* deck,
                         const uint32_t* perms, const uint8_t* gammas, const uint8_t* seeds32, const uint8_t* label,
                         size_t llen, uint8_t* proofs_out, uint8_t* V_out);
int bpp_deck_verify(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, const uint8_t* deck, const uint8_t* label,
                    size_t llen, const uint8_t* proof, size_t proof_len, const uint8_t* V);
int bpp_deck_verify_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* deck,
                          const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V);
int bpp_deck_verify_batch_each(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* deck,
                               const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                               uint8_t* ok_out);

/* ------------------------------------------ blind re-shuffle proof (sound) */
/* The step of a card game in which a player shuffles a deck somebody else
 * committed: the output cards are a permutation of the input cards, each
 * re-blinded, and the prover can open none of them.
 * Statement.  Public: input cards C_0..C_{k-1} and output cards C'_0..C'_{k-1},
 * any valid ristretto255 encodings.  The prover knows a bijection pi on [0, k)
 * and scalars r_i with C'_i = C_{pi(i)} + r_i Bb, Bb = B_blinding of g;
 * perms[i] = pi(i): output slot i holds input perm[i].
 * Argument (DESIGN.md "Protocol: blind re-shuffle"), T = Transcript(label):
 *   append_message("dom-sep", "reshuffle v1"), append_u64("k", k), C_j under
 *   "C", C'_i under "C'";  A_i = pi(i) B + alpha_i Bb under "A", x =
 *   challenge_scalar("x");  e_j = x^(j+1), b_i = e_pi(i), E_i = b_i B + beta_i Bb
 *   under "E", y = challenge_scalar("y");  T_i = t_i B + w_i Bb under "Ti", T_S
 *   = sum_i t_i C'_i - t_R Bb under "T", c = challenge_scalar("c");  z_i = t_i +
 *   c b_i, om_i = w_i + c beta_i, z_R = t_R + c sum_i b_i r_i;  and a proof of
 *   the shuffle_of_public(k) circuit (bpp_circuit_*_pub) under the same label
 *   with v_i = y pi(i) + b_i, blindings y alpha_i + beta_i and public inputs
 *   u_j = y j + e_j, whose commitments V_0..V_{k-1} are D_i = y A_i + E_i.
 * The verifier accepts iff z_i B + om_i Bb = T_i + c E_i for every i, sum_i z_i
 * C'_i - z_R Bb = T_S + c sum_j e_j C_j, and the circuit proof verifies for V =
 * (D_0..D_{k-1}, V_k) with the D_i it formed itself.
 * Proof bytes, bpp_reshuffle_proof_len(k) = 32 (5k + 3) + the circuit proof's
 * (9280 at k = 52; 0 for a k outside [2, 342]):
 *   A[k] | E[k] | Ti[k] | T_S | z[k] | om[k] | z_R | V_k | circuit proof.
 *   k           2 <= k <= 342 (the circuit's 2k - 2 gates within the plain bound
 *               of 682; BPP_ERR_LEN beyond, BPP_ERR_ARG below).  bpp_gens_len(g)
 *               >= max(4, next_pow2(2k - 2)), BPP_ERR_LEN otherwise.
 *   cards_in / cards_out   count x k x 32 B.
 *   perms       count x k u32;  blinds  NULL, or count x k x 32 B: the r_i.
 * Randomness: seeds32 as bpp_perm_prove_batch_entropy.  Draw j =
 * from_wide(SHAKE256("bpperm-reshuffle-sc" || seed32 || le32 j)[0..64]) in the
 * order r[k], alpha[k], beta[k], t[k], w[k], t_R; supplied blinds replace draws
 * 0..k-1; the circuit prover's seed is SHAKE256("bpperm-reshuffle-inner" ||
 * seed32)[0..32].
 * Checks of the prover, before any device work and before any output byte: a
 * perm that is not a bijection on [0, k) -> BPP_ERR_ARG; a blind >= l ->
 * BPP_ERR_NONCANONICAL (neither needs ctx or g); then the k / g / null checks.
 * An input card that does not decode -> BPP_ERR_DECOMPRESS, found on the device
 * before any secret is staged there and before any output byte.  count == 0: BPP_OK.
 * The verifiers mirror bpp_perm_verify, _verify_batch and _verify_batch_each
 * (the ok_out contract and count == 0 included), and refuse a response scalar z,
 * om or z_R >= l with BPP_ERR_NONCANONICAL before any device work, and a card or
 * a point A, E, Ti, T_S that does not decode with BPP_ERR_DECOMPRESS, found on
 * the device before anything else runs; _each instead fails that proof alone
 * (ok_out[p] = 0, BPP_ERR_VERIFY) and gives every other proof its own verdict.  A batch merges the first two checks
 * of all proofs into ONE MSM of 4k + 1 points per proof plus B and Bb, under
 * weights rho_p^1..rho_p^(k+1), rho_p = from_wide(SHAKE256("bpperm-reshuffle-wt"
 * || seed || le64 p || c_p)[0..64]), seed the verifier's own randomness; the
 * circuit proofs go through the circuit batch verifier.  _each: when the merged
 * MSM does not pass, one MSM of 4k + 3 terms per proof; a proof's verdict is
 * that AND the circuit verifier's.
 * Secret lifetime: that of bpp_perm_prove_batch_entropy; the perms, every draw,
 * b, v, the blindings, r_i Bb and t_i C'_i are part of what is zeroed and of what
 * bpp_debug_secret_residue counts. */
size_t bpp_reshuffle_proof_len(uint32_t k);
int bpp_reshuffle_prove_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* cards_in,
                              const uint32_t* perms, const uint8_t* blinds, const uint8_t* seeds32, const uint8_t* label,
                              size_t llen, uint8_t* cards_out, uint8_t* proofs_out);
int bpp_reshuffle_verify(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, const uint8_t* label, size_t llen,
                         const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proof, size_t proof_len);
int bpp_reshuffle_verify_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* label,
                               size_t llen, const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proofs);
int bpp_reshuffle_verify_batch_each(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* label,
                                    size_t llen, const uint8_t* cards_in, const uint8_t* cards_out,
                                    const uint8_t* proofs, uint8_t* ok_out);

/* ----------------------------------------- masked re-shuffle proof (sound) */
/* The blind re-shuffle over cards that can be dealt: a card is an ElGamal pair
 * (U, W) = (rho B, M + rho K) under the table's joint key K = sum_j K_j, and a
 * shuffle permutes and re-masks it.  A blindly re-shuffled commitment stays
 * closed for good (nobody holds the sum of its blindings); a masked card opens
 * as M = W - sum_j sk_j U once every player publishes its share sk_j U, with
 * nobody's permutation disclosed.  The open deck (identity, M_j) -- 32 zero
 * bytes, then the card's public point -- needs no proof, so every player, the
 * first included, runs this same step.  The decryption shares and their proofs
 * are not part of this library yet.
 * Statement.  Public: a key K, input cards (U_j, W_j) and output cards (U'_i,
 * W'_i), any valid ristretto255 encodings (the identity included; K = identity
 * is degenerate and not refused).  The prover knows a bijection pi on [0, k)
 * and scalars r_i with U'_i = U_{pi(i)} + r_i B and W'_i = W_{pi(i)} + r_i K, B
 * the Pedersen value base of g; perms[i] = pi(i).  One key per call.
 * Argument (DESIGN.md "Protocol: masked re-shuffle"), T = Transcript(label);
 * what is not named here is the blind re-shuffle's:
 *   append_message("dom-sep", "masked reshuffle v1"), append_u64("k", k), K
 *   under "K";  every input card as two messages, U_j then W_j, under "C", every
 *   output card the same way under "C'";  A_i, x, E_i, y as there;  T_i under
 *   "Ti", T_U = sum_i t_i U'_i - t_R B and T_W = sum_i t_i W'_i - t_R K under "T",
 *   T_U first, c = challenge_scalar("c");  z_i, om_i, z_R = t_R + c sum_i b_i r_i
 *   and the circuit proof as there.
 * The verifier accepts iff z_i B + om_i Bb = T_i + c E_i for every i, sum_i z_i
 * U'_i - z_R B = T_U + c sum_j e_j U_j, sum_i z_i W'_i - z_R K = T_W + c sum_j e_j
 * W_j, and the circuit proof verifies.  Both sums share z_i and z_R: one r_i
 * re-masks both halves of a card.
 * Proof bytes, bpp_masked_reshuffle_proof_len(k) = 32 (5k + 4) + the circuit
 * proof's (9312 at k = 52; 0 for a k outside [2, 342]):
 *   A[k] | E[k] | Ti[k] | T_U | T_W | z[k] | om[k] | z_R | V_k | circuit proof.
 *   k           as bpp_reshuffle_*, with its error codes.
 *   key         32 B.
 *   cards_in / cards_out   count x k x 64 B, U | W per card.
 *   perms       count x k u32;  blinds  NULL, or count x k x 32 B: the r_i.
 * Randomness: the draws (their indices, their order r, alpha, beta, t, w, t_R,
 * the blinds in place of draws 0..k-1), the circuit prover's seed and the batch
 * weights rho_p are bpp_reshuffle_prove_batch's and _verify_batch's, domain
 * strings included.  Seeds are single-use: a seed used for a plain re-shuffle
 * must not be used again for a masked one, nor the other way round.
 * Checks of the prover, before any device work and before any output byte: a
 * perm that is not a bijection on [0, k) -> BPP_ERR_ARG; a blind >= l ->
 * BPP_ERR_NONCANONICAL (neither needs ctx or g); then the k / g / null checks.
 * A key or a component of an input card that does not decode ->
 * BPP_ERR_DECOMPRESS, found on the device before any secret is staged there and
 * before any output byte.  count == 0: BPP_OK.
 * The verifiers mirror bpp_reshuffle_verify, _verify_batch and
 * _verify_batch_each: a response scalar >= l -> BPP_ERR_NONCANONICAL before any
 * device work; a card component or a point A, E, Ti, T_U, T_W that does not
 * decode -> BPP_ERR_DECOMPRESS, found on the device before anything else runs
 * (_each instead fails that proof alone); a key that does not decode refuses
 * the whole call, in _each too.  A batch merges the first three checks of all
 * proofs into ONE MSM of 6k + 2 points per proof plus B, Bb and K, under weights
 * rho_p^1..rho_p^k, rho_p^(k+1) for the U sum and rho_p^(k+2) for the W sum.
 * _each: when the merged MSM does not pass, one MSM of 6k + 5 terms per proof; a
 * proof's verdict is that AND the circuit verifier's.
 * Secret lifetime: that of bpp_reshuffle_prove_batch; r_i B, r_i K, t_i U'_i,
 * t_i W'_i, t_R B and t_R K are part of what is zeroed and of what
 * bpp_debug_secret_residue counts.  No secret goes through the bucket engine.
 * bpp_verify_groups and the multi-GPU job API do not take these proofs. */
size_t bpp_masked_reshuffle_proof_len(uint32_t k);
int bpp_masked_reshuffle_prove_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* key,
                                     const uint8_t* cards_in, const uint32_t* perms, const uint8_t* blinds,
                                     const uint8_t* seeds32, const uint8_t* label, size_t llen, uint8_t* cards_out,
                                     uint8_t* proofs_out);
int bpp_masked_reshuffle_verify(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, const uint8_t* key, const uint8_t* label,
                                size_t llen, const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proof,
                                size_t proof_len);
int bpp_masked_reshuffle_verify_batch(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count, const uint8_t* key,
                                      const uint8_t* label, size_t llen, const uint8_t* cards_in,
                                      const uint8_t* cards_out, const uint8_t* proofs);
int bpp_masked_reshuffle_verify_batch_each(bpp_ctx* ctx, const bpp_gens* g, uint32_t k, size_t count,
                                           const uint8_t* key, const uint8_t* label, size_t llen,
                                           const uint8_t* cards_in, const uint8_t* cards_out, const uint8_t* proofs,
                                           uint8_t* ok_out);

/* -------------------------------------- caller-defined circuits (sound) */
/* After the shuffle a game needs predicates over the commitments it produced
 * ("the card I play is one of these 13", "this value is below 2^6", "these two
 * hands hold the same multiset").  A statement is a gate program in the style
 * of an R1CS constraint system, compiled once (bpp_circuit_create) to the
 * arithmetic circuit W_L a_L + W_R a_R + W_O a_O = W_V v + c that the two
 * built-in statements are instances of, then proved and verified in batches
 * over the same GPU path.
 * Variables: the committed inputs v_0..v_{m_in-1} (per proof); the challenge x
 * (x_perm: squeezed after V_0..V_{m_in-1}, committed as V_{m_in} and bound by
 * the library's own last row); the wires l_h, r_h, o_h = l_h r_h of n_gates
 * multiplication gates.  A gate side is DEFINED -- a sparse linear combination
 * over {1, v_j, x, wires of gates h < g} -- or FREE: fed from the per-proof
 * auxiliary value aux_t, supplied before x exists (bits and other hints).
 * n_asserts assert rows each force a combination over ANY variable to 0.
 * Rows: defined left sides by gate, defined right sides by gate, the asserts,
 * then v_{m_in} = x.  Defined side of gate g at row q: 1 at (q, g) of its own
 * matrix, a wire term a -> -a in the wire's matrix, a v_j or x term -> W_V = a,
 * the constant -> c[q] = a.  Assert row: wire terms +a, v and x terms -a, the
 * constant -a.  Q = defined sides + n_asserts + 1, m = m_in + 1, n_p = max(4,
 * next_pow2(n_gates)) <= bpp_gens_len(g), proof bytes 32 (13 + 2 log2 n_p).
 * The two-half circuit written this way compiles to bpp_perm_*'s matrices; the
 * deck circuit cannot be written without public inputs (its constant depends
 * on x and on the deck; with them see bpp_circuit_create_pub below).
 * Inside one combination the variable ids are strictly increasing and every
 * coefficient is canonical and nonzero, so one description has one digest:
 * SHAKE256("bpperm-circuit" || le32 m_in || le32 n_gates || le32 n_aux ||
 * le32 n_asserts || side_aux || lc_off || lc_var || lc_coef)[0..32].
 * Transcript: Transcript(label), dom-sep("acp v1", n_p),
 * append_message("circuit", digest), V_0..V_{m_in-1}, challenge x_perm,
 * V_{m_in}, A_I A_O S and on as bpp_perm_*.  Draws: gamma[m], alpha, beta, rho,
 * s_L[n_p], s_R[n_p], tau[5] by index as above; supplied gammas replace draws
 * 0..m_in-1; no pi stream is read.
 * Bounds (BPP_ERR_LEN beyond them): every per-proof kernel keeps its tables in
 * one workgroup's 64 KB of LDS -- (Q + 1 + 2 min(n_p, 256)) x 32 B + 896 B for
 * the polynomial and verifier kernels, i.e. Q <= 1507 at n_p >= 256, and
 * 3 n_gates x 32 B + 32 B for the witness kernel, i.e. n_gates <= 682.  512
 * gates with both sides defined (Q = 1025 + n_asserts) fit.  Larger circuits:
 * bpp_circuit_create_ex with BPP_CIRCUIT_LARGE, below. */
typedef struct bpp_circuit bpp_circuit;
#define BPP_SIDE_LC 0xFFFFFFFFu
typedef struct {
  uint32_t m_in, n_gates, n_aux, n_asserts;
  const uint32_t* side_aux; /* [2n]: side 2g = left of gate g, 2g+1 = right; BPP_SIDE_LC = defined, else aux index */
  const uint32_t* lc_off;   /* [2n + A + 1] term offsets; LC 2g, 2g+1 = gate g's sides (empty when free), then the asserts */
  const uint32_t* lc_var;   /* 0 = one; 1+j = v_j; 1+m_in = x; 2+m_in+3h+{0,1,2} = l_h, r_h, o_h */
  const uint8_t* lc_coef;   /* [T][32] canonical, nonzero */
} bpp_circuit_desc;
/* Validates and compiles desc (no GPU; the arrays are copied).  BPP_ERR_ARG:
 * m_in = 0 or n_gates = 0, an id or aux index out of range, a definition that
 * reads a wire of gate h >= g, a nonempty combination on a free side, unsorted
 * or duplicate ids, a zero coefficient, a non-monotone lc_off;
 * BPP_ERR_NONCANONICAL: a coefficient >= l; BPP_ERR_LEN: beyond the bounds
 * above. */
int bpp_circuit_create(const bpp_circuit_desc* desc, bpp_circuit** out);
void bpp_circuit_destroy(bpp_circuit* c);
/* n_p, Q, m = m_in + 1 and the 32-byte digest (any of them may be NULL). */
int bpp_circuit_info(const bpp_circuit* c, uint32_t* n_p, uint32_t* Q, uint32_t* m, uint8_t digest[32]);
size_t bpp_circuit_proof_len(const bpp_circuit* c);
/* The compiled rows, for audit (no GPU).  which = 0..3: W_L, W_R, W_O, W_V as
 * (q, col, val) triplets; which = 4: c as (q, 0, c[q]) for every row (c[Q-1],
 * set per proof to -x, reads 0).  *count in: the capacity of q / col / val
 * (count x 4, x 4, x 32 B; they may be NULL with capacity 0); out: the number
 * of triplets.  BPP_ERR_LEN if the capacity is short (count is still set). */
int bpp_circuit_matrix(const bpp_circuit* c, uint32_t which, uint32_t* q, uint32_t* col, uint8_t* val, size_t* count);
/* The host witness (no GPU): a_L, a_R, a_O (n_p x 32 B each, padding gates
 * zero) from v (m_in x 32 B), aux (n_aux x 32 B) and x, canonical scalars
 * (BPP_ERR_NONCANONICAL otherwise); *bad_assert = 1 + the first assert that
 * does not hold, or 0.  The code BPP_CIRCUIT_HOST_WITNESS=1 runs in the prover. */
int bpp_circuit_eval(const bpp_circuit* c, const uint8_t* v, const uint8_t* aux, const uint8_t x[32], uint8_t* aL,
                     uint8_t* aR, uint8_t* aO, uint32_t* bad_assert);
/* Proves count statements of c:
 *   v       count x m_in x 32 B: the committed inputs (proof-major);
 *   aux     count x n_aux x 32 B: the free sides' values (NULL when n_aux = 0,
 *           or to have them derived from the circuit's hints, "circuit hints" below);
 *   gammas  NULL, or count x m_in x 32 B: the blindings of V_0..V_{m_in-1};
 *   seeds32, label, proofs_out as bpp_deck_prove_batch; V_out count x (m_in + 1) x 32 B.
 * Every v, aux and gamma is checked canonical before any device work
 * (BPP_ERR_NONCANONICAL).  If an assert does not hold for some proof the call
 * returns BPP_ERR_ARG, bpp_ctx_last_error names the proof and the assert, no
 * output byte is written, and the batch's secrets are wiped as on success
 * (the lifetime of bpp_perm_prove_batch_entropy; v, aux and gammas are part of
 * what is zeroed).  The witness is interpreted on the GPU (k_witness_program);
 * BPP_CIRCUIT_HOST_WITNESS=1 selects the host witness. */
int bpp_circuit_prove_batch(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, size_t count, const uint8_t* v,
                            const uint8_t* aux, const uint8_t* gammas, const uint8_t* seeds32, const uint8_t* label,
                            size_t llen, uint8_t* proofs_out, uint8_t* V_out);
/* The verifiers mirror bpp_deck_verify, _verify_batch and _verify_batch_each
 * with c in place of (k, deck): the same kernels and launches as
 * bpp_perm_verify*.  The multi-GPU job API takes two-half proofs only. */
int bpp_circuit_verify(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, const uint8_t* label, size_t llen,
                       const uint8_t* proof, size_t proof_len, const uint8_t* V);
int bpp_circuit_verify_batch(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, size_t count, const uint8_t* label,
                             size_t llen, const uint8_t* proofs, const uint8_t* V);
int bpp_circuit_verify_batch_each(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, size_t count,
                                  const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                                  uint8_t* ok_out);

/* ------------------------- caller-defined circuits with public inputs */
/* Public inputs u_0..u_{n_pub-1} are canonical 32-byte scalars given per proof
 * to the prover and to the verifier and never committed: "the card I play is
 * one of THESE cards", "V_3 opens to THIS card", "my hand sums to THIS total",
 * "V_0..V_{k-1} commit to a permutation of THIS table's deck" -- one compiled
 * circuit, one digest and one merged batch MSM for proofs whose public data all
 * differ.  bpp_circuit_desc is unchanged; n_pub is bpp_circuit_create_pub's own
 * argument, and the variable ids of lc_var become
 *   0 = one; 1+j = v_j; 1+m_in = x; 2+m_in+i = u_i;
 *   2+m_in+n_pub+3h+{0,1,2} = l_h, r_h, o_h
 * (ids still ascend: constants, inputs, x, public inputs, wires).  A term a u_i
 * may stand in any defined side and in any assert, not on a free side.  It
 * compiles to a sparse matrix W_U (Q x n_pub): +a at (q, i) for a defined side
 * at row q, -a for an assert row -- the signs the constant of the same
 * combination takes -- and proof p's constant vector is c + W_U u_p; nothing
 * else of the statement depends on u.
 * bpp_circuit_create(desc) equals bpp_circuit_create_pub(desc, 0, ..): same
 * matrices, digest and bytes.  With n_pub > 0 the digest is
 * SHAKE256("bpperm-pubcircuit" || le32 m_in || le32 n_pub || le32 n_gates ||
 * le32 n_aux || le32 n_asserts || side_aux || lc_off || lc_var ||
 * lc_coef)[0..32], and the transcript absorbs append_message("pub", u_i), 32
 * bytes each, i < n_pub, right after append_message("circuit", digest): before
 * V_0, x_perm and every other challenge, which binds the proof to them.
 * n_pub <= 2^16 (BPP_ERR_LEN beyond); the other bounds are unchanged.  Proof
 * format and bpp_circuit_proof_len are unchanged.
 * The entry points above without `pub` return BPP_ERR_ARG for a circuit with
 * n_pub > 0 (bpp_circuit_eval, _prove_batch, _verify, _verify_batch,
 * _verify_batch_each); the _pub ones take every circuit (pub is not read when
 * n_pub = 0). */
int bpp_circuit_create_pub(const bpp_circuit_desc* desc, uint32_t n_pub, bpp_circuit** out);
uint32_t bpp_circuit_n_pub(const bpp_circuit* c);
/* bpp_circuit_matrix(c, 5, ..) returns W_U as (q, i, val) triplets. */
/* bpp_circuit_eval with pub (n_pub x 32 B, canonical; NULL when n_pub = 0). */
int bpp_circuit_eval_pub(const bpp_circuit* c, const uint8_t* v, const uint8_t* aux, const uint8_t* pub,
                         const uint8_t x[32], uint8_t* aL, uint8_t* aR, uint8_t* aO, uint32_t* bad_assert);
/* bpp_circuit_prove_batch with pub: count x n_pub x 32 B, proof-major (NULL
 * when n_pub = 0; BPP_ERR_ARG if NULL with n_pub > 0).  Every pub scalar is
 * checked canonical before any device work (BPP_ERR_NONCANONICAL).  pub rides
 * the same upload as v and aux.  An assert that does not hold -- over the
 * public inputs too -- is BPP_ERR_ARG naming the proof and the assert, before
 * any output byte. */
int bpp_circuit_prove_batch_pub(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, size_t count, const uint8_t* v,
                                const uint8_t* aux, const uint8_t* pub, const uint8_t* gammas, const uint8_t* seeds32,
                                const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out);
/* The three verifiers with pub (count x n_pub x 32 B; one proof's for
 * bpp_circuit_verify_pub) after V: the same ok_out contract, count == 0
 * behaviour and order of checks; a NULL pub with n_pub > 0 is BPP_ERR_ARG, a
 * pub scalar >= l BPP_ERR_NONCANONICAL (ok_out all zero).  A proof verifies
 * only under the public inputs it was made for.  pub in pinned host memory
 * (bpp_host_alloc) goes up by DMA, as proofs and V do. */
int bpp_circuit_verify_pub(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, const uint8_t* label, size_t llen,
                           const uint8_t* proof, size_t proof_len, const uint8_t* V, const uint8_t* pub);
int bpp_circuit_verify_batch_pub(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, size_t count,
                                 const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                                 const uint8_t* pub);
int bpp_circuit_verify_batch_each_pub(bpp_ctx* ctx, const bpp_gens* g, const bpp_circuit* c, size_t count,
                                      const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                                      const uint8_t* pub, uint8_t* ok_out);

/* ----------------------------------------------------- large circuits */
/* The bounds of bpp_circuit_create and _create_pub (Q <= 1507, n_gates <= 682)
 * are the size of one workgroup's 64 KB of LDS in three kernels, not the
 * protocol's.  bpp_circuit_create_ex(desc, n_pub, flags, ..) is
 * bpp_circuit_create_pub(desc, n_pub, ..) with flags:
 *   BPP_CIRCUIT_LARGE  accept circuits beyond those bounds.  The bounds left
 *     are m_in, n_aux <= 2^20, n_gates, n_asserts, n_pub <= 2^16 (BPP_ERR_LEN
 *     beyond), the split row table's own LDS -- (256 + (Q >> 8) + 1 +
 *     2 min(n_p, 256)) x 32 B + 896 B, below 64 KB for every Q those allow --
 *     and n_p <= bpp_gens_len(g) at prove and verify time.  A batch of such a
 *     circuit launches, each by its own bound, the polynomial and verifier
 *     kernels that read z^e as lo[e mod 256] hi[e / 256] from two short tables
 *     (where (Q + 1 + 2 min(n_p, 256)) x 32 B + 896 B exceeds 64 KB) and the
 *     witness kernel that keeps its 3 n_gates wires in device memory (where
 *     3 n_gates x 32 B + 32 B does; that array is part of what the prover wipes).
 *     These paths are exercised up to n_p = 2048 and have not been run beyond it.
 *   BPP_CIRCUIT_TILED  use those kernels even where the narrow ones fit
 *     (implies LARGE; for tests and A/B measurements).
 * flags = 0 is bpp_circuit_create_pub, bounds included; unknown flag bits are
 * BPP_ERR_ARG.  Flags choose how a statement is computed and are no part of
 * it: the digest, the matrices, the transcript, the proof bytes and the proof
 * length do not depend on them, and a proof made under a circuit created with
 * LARGE or TILED verifies under the same description created without them
 * (where that can be created), and the reverse.  Every bpp_circuit_* entry
 * point and bpp_verify_groups[_each] take such a circuit with no new argument;
 * BPP_CIRCUIT_HOST_WITNESS=1 selects the host witness at every size. */
#define BPP_CIRCUIT_LARGE 1u
#define BPP_CIRCUIT_TILED 2u
int bpp_circuit_create_ex(const bpp_circuit_desc* desc, uint32_t n_pub, uint32_t flags, bpp_circuit** out);

/* ------------------------------------------------------- circuit hints */
/* Every free gate side is fed from aux, and aux is a pure function of v and the
 * public inputs: the bits of a range check, the inverse of a difference.  A
 * hint program, attached at creation, tells the PROVER how to derive each
 * aux_t, and bpp_circuit_prove_batch[_pub] then takes aux == NULL: the values
 * are produced on the GPU (k_hint_aux, one lane per proof and hint, in front of
 * k_witness_program) from the v and pub rows already uploaded, and none of
 * them is staged, checked, uploaded or wiped on the host.
 *   aux_t = op_t(w_t),  w_t = the hint's sparse combination over {1, v_j, u_i}
 *   mod l (an empty combination: w_t = 0).
 * A hint reads neither x -- aux exists before x does -- nor a wire nor another
 * hint.  One hint per auxiliary value, in aux order: op [n_aux], lc_off
 * [n_aux + 1]; hints == NULL is bpp_circuit_create_ex (no hints at all).
 * BPP_ERR_ARG: an unknown op, arg > 252, an arg on an op that takes none, an id
 * out of range or naming x or a wire, ids not strictly ascending, a zero
 * coefficient, a non-monotone lc_off; BPP_ERR_NONCANONICAL: a coefficient >= l.
 * Hints are no part of the statement: the digest, the matrices, the transcript
 * and the proof bytes do not see them; bpp_circuit_create_hinted(d, n_pub, f, h)
 * and bpp_circuit_create_ex(d, n_pub, f) give the same bpp_circuit_info, proofs
 * made under either verify under the other, and no verifier reads them.
 * Proving: aux == NULL with n_aux > 0 derives the values on a circuit with
 * hints and stays BPP_ERR_ARG on one without; aux != NULL is used as given on
 * both.  An assert that does not hold over derived values (not_equal on equal
 * cards: the hint is 0) is reported as any other: BPP_ERR_ARG naming the proof
 * and the assert, no output byte, secrets wiped -- the derived values, secret as
 * aux is, among them.  Under BPP_CIRCUIT_HOST_WITNESS=1 the host derives them
 * (bpp_circuit_hint_eval's code). */
#define BPP_HINT_VALUE    0u  /* aux_t = w                                            */
#define BPP_HINT_BIT      1u  /* aux_t = bit `arg` of w as an integer in [0, l)       */
#define BPP_HINT_NOT_BIT  2u  /* aux_t = 1 - that bit                                 */
#define BPP_HINT_INV      3u  /* aux_t = w^-1 mod l, 0 when w = 0                     */
#define BPP_HINT_IS_ZERO  4u  /* aux_t = 1 when w = 0, else 0                         */
typedef struct {
  const uint32_t* op;      /* [n_aux]  BPP_HINT_* | arg << 8 (arg <= 252, BIT / NOT_BIT only) */
  const uint32_t* lc_off;  /* [n_aux + 1] */
  const uint32_t* lc_var;  /* 0 = one, 1 + j = v_j, 2 + m_in + i = u_i; x and wires are refused */
  const uint8_t*  lc_coef; /* [T][32] canonical, nonzero; ids strictly ascending per hint */
} bpp_circuit_hints;
int bpp_circuit_create_hinted(const bpp_circuit_desc* desc, uint32_t n_pub, uint32_t flags,
                              const bpp_circuit_hints* hints, bpp_circuit** out);
int bpp_circuit_has_hints(const bpp_circuit* c);
/* The hints' host reference (no GPU): aux_out = n_aux x 32 B from v (m_in x
 * 32 B) and pub (n_pub x 32 B; NULL when n_pub = 0), canonical scalars
 * (BPP_ERR_NONCANONICAL otherwise); BPP_ERR_ARG on a circuit without hints. */
int bpp_circuit_hint_eval(const bpp_circuit* c, const uint8_t* v, const uint8_t* pub, uint8_t* aux_out);
/* Test hook beside bpp_debug_secret_residue: runs ONLY the device kernel over
 * count proofs (v count x m_in x 32 B, pub count x n_pub x 32 B) and copies the
 * derived values back (aux_out count x n_aux x 32 B); what it left on the
 * device and in staging is wiped before it returns. */
int bpp_debug_circuit_hints(bpp_ctx* ctx, const bpp_circuit* c, size_t count, const uint8_t* v, const uint8_t* pub,
                            uint8_t* aux_out);

/* ------------------------------------------------- circuit hints over wires */
/* bpp_circuit_create_wire_hinted takes the same bpp_circuit_hints, ops and arg
 * rule, and the flags of bpp_circuit_create_ex, but a hint's combination ranges
 * over the variable space of a defined side, with the ids of
 * bpp_circuit_desc.lc_var: {1, v_j, x, u_i, the wires l_h r_h o_h}.  A hint that
 * names x or a wire is LATE, every other is EARLY and is the hint above.  A_I
 * is committed after x_perm and after V_{m_in}, so a free side may depend on x
 * and on every earlier wire with no change to the statement, the transcript or
 * a verifier; what a late hint cannot be is supplied by a caller who has no x.
 *   - a late hint that reads a wire of gate h feeds sides of gates g > h only,
 *     checked for every side its aux index feeds; an id beyond the last wire
 *     (2 + m_in + n_pub + 3 n_gates) is refused: BPP_ERR_ARG, as is everything
 *     bpp_circuit_create_hinted refuses but an id that names x or a wire;
 *   - a late hint is evaluated once for each side it feeds, from the wires of
 *     earlier gates, when the witness reaches that gate; one that feeds no side
 *     is never evaluated;
 *   - a program without a late hint behaves as under bpp_circuit_create_hinted.
 * Hints remain no part of the statement: for one description the digest, the
 * matrices, bpp_circuit_info, the proof bytes and the verifiers are the same
 * whether it was created plain, hinted or wire-hinted.  A gate's dependency
 * level counts the gates its sides' late hints read (scheduling only).
 * Proving: aux == NULL derives every value -- the early ones by k_hint_aux, the
 * late ones inside the witness kernel (k_witness_program*_late), where they go
 * straight to the wires and are never stored as aux; aux != NULL is used as
 * given.  Under BPP_CIRCUIT_HOST_WITNESS=1 the host derives them
 * (bpp_circuit_hint_eval_x's code) once x exists. */
int bpp_circuit_create_wire_hinted(const bpp_circuit_desc* desc, uint32_t n_pub, uint32_t flags,
                                   const bpp_circuit_hints* hints, bpp_circuit** out);
/* The host reference with x (no GPU): all n_aux values -- early hints as
 * bpp_circuit_hint_eval gives them, late hints in gate order from the wires so
 * far (0 for a late hint that feeds no side).  bpp_circuit_eval[_pub] over
 * aux_out and the same x gives the witness.  x: 32 B canonical.  On a circuit
 * with a late hint bpp_circuit_hint_eval and bpp_debug_circuit_hints, which have
 * no x, return BPP_ERR_ARG. */
int bpp_circuit_hint_eval_x(const bpp_circuit* c, const uint8_t* v, const uint8_t* pub, const uint8_t x[32],
                            uint8_t* aux_out);
/* Test hook: ONLY the witness kernels over count proofs -- k_hint_aux where the
 * circuit has early hints, then the witness kernel a batch of this circuit
 * launches -- with x supplied by the caller (count x 32 B, canonical; v and pub
 * as above).  aL, aR, aO: count x n_p x 32 B canonical each; fail[p] = 1 + the
 * first assert of proof p that does not hold, or 0.  BPP_ERR_ARG on a circuit
 * with auxiliary values and no hints.  Staged through a recorded span and wiped
 * before it returns, as bpp_debug_circuit_hints. */
int bpp_debug_circuit_witness(bpp_ctx* ctx, const bpp_circuit* c, size_t count, const uint8_t* v, const uint8_t* pub,
                              const uint8_t* x, uint8_t* aL, uint8_t* aR, uint8_t* aO, uint32_t* fail);

/* Mixed batches: proofs of different statements verified in one call with ONE
 * GPU MSM.  A group is `count` proofs of one statement under one label: the
 * two-half shuffle of k cards, the public-deck shuffle of k cards (deck as
 * bpp_deck_verify_batch takes it), or a compiled circuit (pub as the _pub
 * verifiers take it when the circuit's n_pub > 0, NULL otherwise).  proofs, V
 * and pub have the layouts of that statement's _verify_batch.  Groups may
 * differ in n_p, m and proof length, may be empty, and two groups may name the
 * same statement; at most BPP_VERIFY_GROUPS_MAX groups per call (BPP_ERR_LEN
 * beyond; the caller splits).
 * One verifier seed serves the call: the proof at position p of group g is
 * weighted by its index in the call, (the counts of the groups before g) + p.
 * Every non-empty group's upload, replay and decompression run on a stream of
 * its own beside the others'; the generator scalars of all groups are summed
 * into one block of the widest circuit's width (the generator chain is one
 * sequence: a narrower circuit uses its first n_p) and one MSM of 2 n_max + 2
 * + sum count_g (m_g + 8 + 2 lg_g) terms decides.  g must cover n_max
 * (BPP_ERR_LEN otherwise).
 *   BPP_OK          every proof of every group verifies.
 *   BPP_ERR_VERIFY  at least one does not.
 * Refused before any device work, and with no effect on any job of ctx: what
 * the statement's own entry points refuse -- k outside [2, 2^20], a deck card or
 * a public input >= l (BPP_ERR_NONCANONICAL), a NULL circuit, a NULL pub with
 * n_pub > 0 -- and a pub given with n_pub = 0, an unknown kind, NULL proofs or
 * V with count > 0 (BPP_ERR_ARG; bpp_ctx_last_error names the group).
 * n_groups == 0 or every count 0: BPP_OK, nothing is launched.
 * bpp_verify_groups_each writes one verdict per proof (ok: sum of the counts
 * bytes, in group order) under the ok_out contract of
 * bpp_perm_verify_batch_each: a batch that passes costs what bpp_verify_groups
 * costs; otherwise each proof's own MSM runs over what the groups' jobs left on
 * the device, and bpp_ctx_last_error gives the count and the first failing
 * index in the call.  The per-kind entry points on the same ctx are not
 * affected by either call. */
#define BPP_STMT_PERM 0    /* two-half shuffle: k                    */
#define BPP_STMT_DECK 1    /* public-deck shuffle: k, deck (or NULL) */
#define BPP_STMT_CIRCUIT 2 /* circuit handle; pub iff its n_pub > 0  */
#define BPP_VERIFY_GROUPS_MAX 16
typedef struct {
  uint32_t kind, k;
  const uint8_t* deck;        /* DECK: k x 32 canonical, or NULL = 1..k */
  const bpp_circuit* circuit; /* CIRCUIT */
  const uint8_t* label;
  size_t label_len;
  size_t count;      /* may be 0 */
  const uint8_t* proofs; /* count x proof_len */
  const uint8_t* V;      /* count x m x 32 */
  const uint8_t* pub;    /* count x n_pub x 32, CIRCUIT with n_pub > 0 */
} bpp_verify_group;
int bpp_verify_groups(bpp_ctx* ctx, const bpp_gens* g, const bpp_verify_group* groups, size_t n_groups);
int bpp_verify_groups_each(bpp_ctx* ctx, const bpp_gens* g, const bpp_verify_group* groups, size_t n_groups,
                           uint8_t* ok);

/* Batch verification split for several GPUs (north_star: "the single large
 * verifier MSM partitions its bucket windows across GPUs"; reference verify
 * circuit_lib.rs:478-585).  Host phase, no GPU: parse `count` proofs, replay
 * their transcripts and return each proof's weight challenge r (count x 32
 * B, may be NULL).  BPP_ERR_VERIFY if a proof is malformed or its transcript
 * rejects a point encoding. */
typedef struct bpp_verify_job bpp_verify_job;
int bpp_perm_verify_begin(uint32_t k, size_t count, const uint8_t* label, size_t llen, const uint8_t* proofs,
                          const uint8_t* V, uint8_t* r_out, bpp_verify_job** out);
/* The same host interface with the replay on the GPU of ctx (one Merlin
 * transcript per 16-lane group, k_verify_replay_g): uploads the proofs and V, replays every
 * transcript, decompresses the proof points and returns r (count x 32 B, may
 * be NULL).  r is byte-identical to bpp_perm_verify_begin's.  The job keeps
 * its records and points in ctx's workspaces: it is valid for
 * bpp_perm_verify_partial on the same ctx until the next verification on
 * that ctx -- bpp_perm_verify_begin_dev, bpp_perm_verify,
 * bpp_perm_verify_batch or bpp_perm_verify_batch_each, which all replay
 * through the same workspaces
 * (BPP_ERR_ARG after that; a call refused for its arguments supersedes
 * nothing) -- and
 * bpp_perm_verify_scalars rejects it (BPP_ERR_ARG).  The proof points are
 * decompressed beside the replay; one that does not decode makes
 * bpp_perm_verify_partial return BPP_ERR_VERIFY. */
int bpp_perm_verify_begin_dev(bpp_ctx* ctx, uint32_t k, size_t count, const uint8_t* label, size_t llen,
                              const uint8_t* proofs, const uint8_t* V, uint8_t* r_out, bpp_verify_job** out);
/* Terms of the job's MSM: 2 n_p + 2 merged generators + count x (m + 8 +
 * 2 log2 n_p) proof points.  bpp_msm_windows(terms) gives c and W. */
int bpp_perm_verify_terms(const bpp_verify_job* job, size_t* terms);
/* 32 bytes of verifier randomness for a batch (the OS CSPRNG).  Every job,
 * slice and rank of ONE batch takes the same seed (rank 0 draws it and
 * broadcasts the 32 bytes); a seed the provers can predict voids the batch's
 * soundness. */
int bpp_verify_seed(uint8_t seed[32]);
/* The job's MSM terms (host): proof p of the job is batch proof first + p,
 * weighted by w = from_wide(SHAKE256("bp-perm-batch-wt" || seed || le64(first
 * + p) || r_p)[0..64]) (bpp_perm_verify_batch).  scalars_out: terms x 32 B
 * (G[0..n_p), H[0..n_p), B, B_blinding, then the proof points'); points_out:
 * the proof points' encodings ((terms - 2 n_p - 2) x 32 B).  Every proof's
 * check is scaled by (prod u_j)^2 y^(n_p - 1), so no inverse is formed. */
int bpp_perm_verify_scalars(const bpp_verify_job* job, const uint8_t seed[32], size_t first, uint8_t* scalars_out,
                            uint8_t* points_out);
/* The job's MSM over bucket windows [w_begin, w_end) on this GPU -> 128-B
 * raw partial point, its proofs being batch proofs [first, first + count)
 * weighted from `seed` as bpp_perm_verify_scalars.  The batch verifies iff
 * the partials of every window range (window split: every rank's job holds
 * all proofs) or of every proof slice (proof split: all windows each, no
 * exchange before the MSM) sum to the identity (bpp_partials_is_identity). */
int bpp_perm_verify_partial(bpp_ctx* ctx, const bpp_gens* g, const bpp_verify_job* job, const uint8_t seed[32],
                            size_t first, uint32_t w_begin, uint32_t w_end, uint8_t partial[128]);
/* Window split with the upload and decompression sharded too (config 5
 * over N GPUs, "windows_sharded").  Rank r of N, slice
 * [first, first + n) of the batch:
 *   1. bpp_perm_verify_begin_dev(_async) over the slice's proofs and V only
 *      (each rank uploads, decompresses and replays 1/N of the batch);
 *   2. bpp_perm_verify_slice_points copies the slice's decompressed points
 *      (bpp_perm_verify_slice_point_bytes(job): n x npt records of 128 B,
 *      proof-major) to device memory d_out; BPP_ERR_VERIFY if one did not
 *      decode; returns once d_out is complete (it waits for the
 *      decompression, not for an asynchronous begin's replay), so the point
 *      blocks' all-gather can run beside the replay and step 3;
 *   3. bpp_perm_verify_slice_scalars_at(job, seed, first) writes the slice's
 *      scalar block to device memory d_out (bpp_perm_verify_slice_bytes(job)
 *      bytes): the 2 n_p + 2 generator scalars summed over the slice, then
 *      the slice's n x (m + 8 + 2 lg) proof-point scalars (32 B each,
 *      canonical), the proofs weighted as batch proofs first + p; it
 *      synchronises ctx, so d_out is complete for a collective on return;
 *   4. the point blocks (pstride bytes apart) and the scalar blocks (stride
 *      apart) of all slices are all-gathered into device memory (RCCL
 *      all_gather over xGMI), slices contiguous and in proof order;
 *   5. bpp_perm_verify_partial_sharded runs the MSM of ALL proofs over windows
 *      [w_begin, w_end) from the gathered blocks (job: this rank's slice job,
 *      which must sit at proof offset `first` among counts[]);
 *   6. the 128-B partials are exchanged as for bpp_perm_verify_partial;
 *      a replay reject or an undecodable point on any rank vetoes the batch. */
/* bpp_perm_verify_begin_dev without waiting for the replay (no r_out): the
 * replay's verdicts are checked by the job's next synchronising call
 * (bpp_perm_verify_slice_scalars_at and bpp_perm_verify_partial return
 * BPP_ERR_VERIFY for a rejected proof); bpp_perm_verify_slice_points can run
 * meanwhile (it waits for the decompression only).  Pinned input buffers --
 * bpp_host_alloc's and any memory the caller page-locked itself
 * (hipHostRegister / hipHostMalloc), which the library also sends by DMA --
 * are read after the return: keep them alive and unchanged until that next
 * synchronising call; pageable ones are staged before it returns. */
int bpp_perm_verify_begin_dev_async(bpp_ctx* ctx, uint32_t k, size_t count, const uint8_t* label, size_t llen,
                                    const uint8_t* proofs, const uint8_t* V, bpp_verify_job** out);
size_t bpp_perm_verify_slice_bytes(const bpp_verify_job* job);
int bpp_perm_verify_slice_scalars_at(bpp_ctx* ctx, const bpp_verify_job* job, const uint8_t seed[32], size_t first,
                                     void* d_out);
size_t bpp_perm_verify_slice_point_bytes(const bpp_verify_job* job);
int bpp_perm_verify_slice_points(bpp_ctx* ctx, const bpp_verify_job* job, void* d_out);
int bpp_perm_verify_partial_sharded(bpp_ctx* ctx, const bpp_gens* g, const bpp_verify_job* job, size_t first,
                                    const void* d_blocks, size_t stride, const void* d_pblocks, size_t pstride,
                                    const size_t* counts, size_t nslices, uint32_t w_begin, uint32_t w_end,
                                    uint8_t partial[128]);
void bpp_perm_verify_end(bpp_verify_job* job);
/* BPP_OK if the partials add up to the identity, else BPP_ERR_VERIFY (also
 * for any partial with Z = 0, so an unwritten all-zero partial never passes;
 * callers still exchange a per-rank ok flag). */
int bpp_partials_is_identity(const uint8_t* partials, size_t count);

#ifdef __cplusplus
}
#endif
#endif
