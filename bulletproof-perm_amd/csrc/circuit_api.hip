// Caller-defined circuits: the C ABI (bpp_circuit_*, include/bpperm.h) --
// argument checks, bpp_guard and marshalling.  The compile and the host
// witness are host/circuit.cpp; the prover is perm_prove.hip with the circuit's
// rows of ProveInputs, the verifier perm_verify.hip; the _pub entry points carry
// each proof's public inputs to both.
#include <string>

#include "circuit_witness.h"
#include "host/circuit.h"
#include "perm_internal.h"

using namespace perm_impl;

static_assert(circuit::OK == BPP_OK && circuit::ERR_ARG == BPP_ERR_ARG && circuit::ERR_LEN == BPP_ERR_LEN &&
                  circuit::ERR_NONCANONICAL == BPP_ERR_NONCANONICAL && circuit::SIDE_LC == BPP_SIDE_LC &&
                  circuit::kLarge == BPP_CIRCUIT_LARGE && circuit::kTiled == BPP_CIRCUIT_TILED,
              "host/circuit.h restates these");

namespace {

// the entry points without `pub` take circuits without public inputs only
int no_pub(bpp_ctx* ctx, const bpp_circuit* c) {
  if (!c || !c->C.n_pub) return BPP_OK;
  if (ctx) ctx->err = "the circuit has public inputs: use the _pub entry point";
  return BPP_ERR_ARG;
}

int circuit_eval(const bpp_circuit* c, const uint8_t* v, const uint8_t* aux, const uint8_t* pub, const uint8_t x[32],
                 uint8_t* aL, uint8_t* aR, uint8_t* aO, uint32_t* bad_assert) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!c || !v || !x || !aL || !aR || !aO || !bad_assert) return BPP_ERR_ARG;
    const circuit::Program& P = *c->C.program;
    if ((!aux && P.n_aux) || (!pub && P.n_pub)) return BPP_ERR_ARG;
    std::vector<Sc> vs(P.m_in), as(P.n_aux), us(P.n_pub), L, R, O;
    Sc xs;
    for (uint32_t j = 0; j < P.m_in; ++j)
      if (!hsc::from_canonical(vs[j], v + 32 * (size_t)j)) return BPP_ERR_NONCANONICAL;
    for (uint32_t j = 0; j < P.n_aux; ++j)
      if (!hsc::from_canonical(as[j], aux + 32 * (size_t)j)) return BPP_ERR_NONCANONICAL;
    for (uint32_t j = 0; j < P.n_pub; ++j)
      if (!hsc::from_canonical(us[j], pub + 32 * (size_t)j)) return BPP_ERR_NONCANONICAL;
    if (!hsc::from_canonical(xs, x)) return BPP_ERR_NONCANONICAL;
    circuit::eval(P, c->C.n_p, vs.data(), as.data(), xs, L, R, O, bad_assert, us.data());
    memcpy(aL, L.data(), 32 * (size_t)c->C.n_p);  // (canonical Sc == its 32 bytes)
    memcpy(aR, R.data(), 32 * (size_t)c->C.n_p);
    memcpy(aO, O.data(), 32 * (size_t)c->C.n_p);
    for (auto* s : {&vs, &as, &L, &R, &O}) std::fill(s->begin(), s->end(), hsc::zero());
    return BPP_OK;
  });
}

// bpp_circuit_hint_eval (x == nullptr; not for a circuit with late hints) and bpp_circuit_hint_eval_x
int circuit_hint_eval(const bpp_circuit* c, const uint8_t* v, const uint8_t* pub, const uint8_t* x, bool with_x,
                      uint8_t* aux_out) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!c || !v || (with_x && !x)) return BPP_ERR_ARG;
    const circuit::Program& P = *c->C.program;
    if (!P.hints || (!pub && P.n_pub) || (!aux_out && P.n_aux)) return BPP_ERR_ARG;
    if (!with_x && circuit::has_late_hints(P)) return BPP_ERR_ARG;
    std::vector<Sc> vs(P.m_in), us(P.n_pub), as(P.n_aux);
    Sc xs = hsc::zero();
    for (uint32_t j = 0; j < P.m_in; ++j)
      if (!hsc::from_canonical(vs[j], v + 32 * (size_t)j)) return BPP_ERR_NONCANONICAL;
    for (uint32_t j = 0; j < P.n_pub; ++j)
      if (!hsc::from_canonical(us[j], pub + 32 * (size_t)j)) return BPP_ERR_NONCANONICAL;
    if (with_x && !hsc::from_canonical(xs, x)) return BPP_ERR_NONCANONICAL;
    if (with_x)
      circuit::hint_eval_x(P, vs.data(), us.data(), xs, as.data());
    else
      circuit::hint_eval(P, vs.data(), us.data(), as.data());
    if (P.n_aux) memcpy(aux_out, as.data(), 32 * (size_t)P.n_aux);  // (canonical Sc == its 32 bytes)
    for (auto* s : {&vs, &as}) std::fill(s->begin(), s->end(), hsc::zero());
    return BPP_OK;
  });
}

// The test hooks' inputs on the device as a batch's are: count proofs' v | pub
// [| x] (x == nullptr: no x rows) in one upload through the batch's own upload
// workspace and a staging span that prove_wipe zeroes, as draws_upload stages
// them.  *d_pub: nullptr on a circuit without public inputs.
int stage_inputs(bpp_ctx* ctx, const circuit::Program& P, size_t count, const uint8_t* v, const uint8_t* pub,
                 const uint8_t* x, const uint32_t** d_v, const uint32_t** d_pub, const uint32_t** d_x) {
  const size_t vb = count * 32 * (size_t)P.m_in, ub = count * 32 * (size_t)P.n_pub, xb = x ? count * 32 : 0;
  void* d_in = nullptr;
  uint8_t* stage = nullptr;
  BPP_TRY(ctx_ws(ctx, "pb_rng_in", vb + ub + xb, &d_in));
  BPP_TRY(ctx_h2d_stage(ctx, vb + ub + xb, &stage));
  ctx_secret_span(ctx, stage, vb + ub + xb);
  memcpy(stage, v, vb);
  if (ub) memcpy(stage + vb, pub, ub);
  if (xb) memcpy(stage + vb + ub, x, xb);
  *d_v = (const uint32_t*)d_in;
  *d_pub = ub ? (const uint32_t*)((const uint8_t*)d_in + vb) : nullptr;
  if (d_x) *d_x = (const uint32_t*)((const uint8_t*)d_in + vb + ub);
  return ctx_h2d_staged(ctx, d_in, stage, vb + ub + xb);
}

int create_hinted(const bpp_circuit_desc* desc, uint32_t n_pub, uint32_t flags, const bpp_circuit_hints* hints,
                  bool wire_hints, bpp_circuit** out) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!desc || !out) return BPP_ERR_ARG;
    *out = nullptr;
    circuit::Desc d = {desc->m_in,   desc->n_gates, desc->n_aux,  desc->n_asserts,
                       desc->side_aux, desc->lc_off,  desc->lc_var, desc->lc_coef};
    d.n_pub = n_pub;
    d.flags = flags;
    circuit::HintDesc h = {};
    if (hints) h = {hints->op, hints->lc_off, hints->lc_var, hints->lc_coef};
    std::unique_ptr<bpp_circuit> c(new bpp_circuit());
    std::string err;
    BPP_TRY(circuit::compile(d, c->C, err, hints ? &h : nullptr, wire_hints));
    *out = c.release();
    return BPP_OK;
  });
}

}  // namespace

extern "C" {

int bpp_circuit_create_hinted(const bpp_circuit_desc* desc, uint32_t n_pub, uint32_t flags,
                              const bpp_circuit_hints* hints, bpp_circuit** out) {
  return create_hinted(desc, n_pub, flags, hints, false, out);
}

int bpp_circuit_create_wire_hinted(const bpp_circuit_desc* desc, uint32_t n_pub, uint32_t flags,
                                   const bpp_circuit_hints* hints, bpp_circuit** out) {
  return create_hinted(desc, n_pub, flags, hints, true, out);
}

int bpp_circuit_create_ex(const bpp_circuit_desc* desc, uint32_t n_pub, uint32_t flags, bpp_circuit** out) {
  return bpp_circuit_create_hinted(desc, n_pub, flags, nullptr, out);
}

int bpp_circuit_create_pub(const bpp_circuit_desc* desc, uint32_t n_pub, bpp_circuit** out) {
  return bpp_circuit_create_ex(desc, n_pub, 0, out);
}

int bpp_circuit_create(const bpp_circuit_desc* desc, bpp_circuit** out) {
  return bpp_circuit_create_pub(desc, 0, out);
}

void bpp_circuit_destroy(bpp_circuit* c) { delete c; }

uint32_t bpp_circuit_n_pub(const bpp_circuit* c) { return c ? c->C.n_pub : 0; }

int bpp_circuit_has_hints(const bpp_circuit* c) { return c && c->C.program->hints ? 1 : 0; }

int bpp_circuit_hint_eval(const bpp_circuit* c, const uint8_t* v, const uint8_t* pub, uint8_t* aux_out) {
  return circuit_hint_eval(c, v, pub, nullptr, false, aux_out);
}

int bpp_circuit_hint_eval_x(const bpp_circuit* c, const uint8_t* v, const uint8_t* pub, const uint8_t x[32],
                            uint8_t* aux_out) {
  return circuit_hint_eval(c, v, pub, x, true, aux_out);
}

// Test hook: k_hint_aux alone over count proofs' v and pub, the derived values
// back to the host; the workspaces it used are wiped as a batch's are.
int bpp_debug_circuit_hints(bpp_ctx* ctx, const bpp_circuit* c, size_t count, const uint8_t* v, const uint8_t* pub,
                            uint8_t* aux_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !c || !c->C.program->hints) return BPP_ERR_ARG;
    const circuit::Program& P = *c->C.program;
    if (circuit::has_late_hints(P)) {
      ctx->err = "the circuit has late hints, which have no value without x: bpp_debug_circuit_witness";
      return BPP_ERR_ARG;
    }
    if (!count || !P.n_aux) return BPP_OK;
    if (!v || !aux_out || (!pub && P.n_pub) || count > 0xFFFFFFFFu) return BPP_ERR_ARG;
    std::vector<int> bad(count, BPP_OK);
    check_canonical(v, P.m_in, count, bad);
    check_canonical(pub, P.n_pub, count, bad);
    if (first_bad(bad) != SIZE_MAX) return BPP_ERR_NONCANONICAL;
    BPP_HIP(hipSetDevice(ctx->device));
    void* d_aux = nullptr;
    const uint32_t *d_v = nullptr, *d_pub = nullptr;
    int rc = stage_inputs(ctx, P, count, v, pub, nullptr, &d_v, &d_pub, nullptr);
    if (rc == BPP_OK) rc = ctx_ws(ctx, "pb_aux_hint", count * 32 * (size_t)P.n_aux, &d_aux);
    if (rc == BPP_OK) rc = hint_aux_dev(ctx, c->C, (uint32_t)count, d_v, d_pub, (uint32_t*)d_aux);
    if (rc == BPP_OK) rc = ctx_sync(ctx);
    if (rc == BPP_OK && hipMemcpy(aux_out, d_aux, count * 32 * (size_t)P.n_aux, hipMemcpyDeviceToHost) != hipSuccess)
      rc = BPP_ERR_DEVICE;
    const int wrc = prove_wipe(ctx);
    return rc ? rc : wrc;
  });
}

// Test hook: the witness kernels alone.  k_hint_aux where the circuit has early
// hints, then the witness kernel a batch of this circuit launches, over count
// proofs' v, pub and the caller's x; a_L, a_R, a_O ([count][n_p], canonical)
// and each proof's fail word back to the host.  Staged and wiped as a batch is.
int bpp_debug_circuit_witness(bpp_ctx* ctx, const bpp_circuit* c, size_t count, const uint8_t* v, const uint8_t* pub,
                              const uint8_t* x, uint8_t* aL, uint8_t* aR, uint8_t* aO, uint32_t* fail) {
  return bpp_guard(ctx, [&]() -> int {
    if (!ctx || !c) return BPP_ERR_ARG;
    const circuit::Program& P = *c->C.program;
    if (P.n_aux && !P.hints) {
      ctx->err = "bpp_debug_circuit_witness: the circuit's auxiliary values have no hints";
      return BPP_ERR_ARG;
    }
    if (!count) return BPP_OK;
    if (!v || !x || !aL || !aR || !aO || !fail || (!pub && P.n_pub) || count > 0xFFFFFFFFu) return BPP_ERR_ARG;
    std::vector<int> bad(count, BPP_OK);
    check_canonical(v, P.m_in, count, bad);
    check_canonical(pub, P.n_pub, count, bad);
    check_canonical(x, 1, count, bad);
    if (first_bad(bad) != SIZE_MAX) return BPP_ERR_NONCANONICAL;
    BPP_HIP(hipSetDevice(ctx->device));
    const uint32_t n_p = c->C.n_p, per = 3 + 5 * n_p;  // (the prover's A_I / A_O / S scalar rows)
    void *d_aux = nullptr, *d_s = nullptr;
    uint32_t* h_fail = nullptr;
    const uint32_t *d_v = nullptr, *d_pub = nullptr, *d_x = nullptr;
    int rc = stage_inputs(ctx, P, count, v, pub, x, &d_v, &d_pub, &d_x);
    if (rc == BPP_OK) rc = ctx_ws(ctx, "mt_s", count * (size_t)per * 32 + 32, &d_s);
    if (rc == BPP_OK) rc = ctx_zc_out(ctx, "wp_fail_h", count * 4, &h_fail);
    if (rc == BPP_OK && P.n_aux) {
      rc = ctx_ws(ctx, "pb_aux_hint", count * 32 * (size_t)P.n_aux, &d_aux);
      if (rc == BPP_OK) rc = hint_aux_dev(ctx, c->C, (uint32_t)count, d_v, d_pub, (uint32_t*)d_aux);
    }
    if (rc == BPP_OK)
      rc = witness_program_dev(ctx, c->C, (uint32_t)count, d_v, (const uint32_t*)d_aux, d_x, per, (uint32_t*)d_s, h_fail,
                               d_pub, true);
    if (rc == BPP_OK) rc = ctx_sync(ctx);
    if (rc == BPP_OK) {
      std::vector<uint8_t> rows(count * (size_t)per * 32);
      if (hipMemcpy(rows.data(), d_s, rows.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = BPP_ERR_DEVICE;
      for (size_t p = 0; p < count && rc == BPP_OK; ++p) {
        const uint8_t* row = rows.data() + p * (size_t)per * 32;
        memcpy(aL + p * 32 * (size_t)n_p, row + 32 * (size_t)1, 32 * (size_t)n_p);
        memcpy(aR + p * 32 * (size_t)n_p, row + 32 * (size_t)(1 + n_p), 32 * (size_t)n_p);
        memcpy(aO + p * 32 * (size_t)n_p, row + 32 * (size_t)(2 + 2 * n_p), 32 * (size_t)n_p);
        fail[p] = h_fail[p];
      }
      std::fill(rows.begin(), rows.end(), 0);
    }
    const int wrc = prove_wipe(ctx);
    return rc ? rc : wrc;
  });
}

int bpp_circuit_info(const bpp_circuit* c, uint32_t* n_p, uint32_t* Q, uint32_t* m, uint8_t digest[32]) {
  if (!c) return BPP_ERR_ARG;
  if (n_p) *n_p = c->C.n_p;
  if (Q) *Q = c->C.Q;
  if (m) *m = c->C.m;
  if (digest) memcpy(digest, c->C.program_digest, 32);
  return BPP_OK;
}

size_t bpp_circuit_proof_len(const bpp_circuit* c) { return c ? perm::proof_len(c->C) : 0; }

int bpp_circuit_matrix(const bpp_circuit* c, uint32_t which, uint32_t* q, uint32_t* col, uint8_t* val, size_t* count) {
  return bpp_guard(nullptr, [&]() -> int {
    if (!c || !count || which > 5) return BPP_ERR_ARG;
    const std::vector<perm::Entry>* const W[6] = {&c->C.WL, &c->C.WR, &c->C.WO, &c->C.WV, nullptr, &c->C.WU};
    const size_t cap = *count, n = which != 4 ? W[which]->size() : c->C.c.size();
    *count = n;
    if (cap < n) return BPP_ERR_LEN;
    if (n && (!q || !col || !val)) return BPP_ERR_ARG;
    for (size_t i = 0; i < n; ++i) {
      q[i] = which != 4 ? (*W[which])[i].q : (uint32_t)i;
      col[i] = which != 4 ? (*W[which])[i].col : 0;
      hsc::to_bytes(val + 32 * i, which != 4 ? (*W[which])[i].val : c->C.c[i]);
    }
    return BPP_OK;
  });
}

int bpp_circuit_eval(const bpp_circuit* c, const uint8_t* v, const uint8_t* aux, const uint8_t x[32], uint8_t* aL,
                     uint8_t* aR, uint8_t* aO, uint32_t* bad_assert) {
  if (c && c->C.n_pub) return BPP_ERR_ARG;
  return circuit_eval(c, v, aux, nullptr, x, aL, aR, aO, bad_assert);
}

int bpp_circuit_eval_pub(const bpp_circuit* c, const uint8_t* v, const uint8_t* aux, const uint8_t* pub,
                         const uint8_t x[32], uint8_t* aL, uint8_t* aR, uint8_t* aO, uint32_t* bad_assert) {
  return circuit_eval(c, v, aux, pub, x, aL, aR, aO, bad_assert);
}

int bpp_circuit_prove_batch_pub(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, size_t count, const uint8_t* v,
                                const uint8_t* aux, const uint8_t* pub, const uint8_t* gammas, const uint8_t* seeds32,
                                const uint8_t* label, size_t llen, uint8_t* proofs_out, uint8_t* V_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (!c || (!label && llen)) return BPP_ERR_ARG;
    const uint32_t m_in = c->C.nv, n_aux = c->C.program->n_aux;
    // aux == NULL on a circuit with hints: the values are derived on the GPU
    const bool derive = circuit::aux_derived(*c->C.program, aux);
    if ((!v || (!aux && n_aux && !derive) || !proofs_out || !V_out) && count) return BPP_ERR_ARG;
    if (!pub && c->C.n_pub && count) return BPP_ERR_ARG;
    // every scalar of the witness is checked before any device work and
    // before any output byte is written (it needs neither the context nor
    // the generators, whose null checks follow)
    std::vector<int> bad(count, BPP_OK);
    check_canonical(v, m_in, count, bad);
    check_canonical(aux, n_aux, count, bad);
    check_canonical(gammas, m_in, count, bad);
    if (const size_t p = first_bad(bad); p != SIZE_MAX) {
      if (ctx) ctx->err = "circuit proof " + std::to_string(p) + ": non-canonical value, auxiliary value or blinding";
      return bad[p];
    }
    {
      size_t p = 0;
      const int rc = pub_check(c, count, pub, &p);
      if (rc == BPP_ERR_NONCANONICAL && ctx) ctx->err = "circuit proof " + std::to_string(p) + ": non-canonical public input";
      BPP_TRY(rc);
    }
    if (!ctx || !G) return BPP_ERR_ARG;
    if (!count) return BPP_OK;
    ProveInputs in;
    in.values = {v, m_in};
    in.aux = {n_aux ? aux : nullptr, n_aux};  // (p = nullptr with n_aux > 0: derived from the circuit's hints)
    in.gammas = {gammas, m_in};
    in.pub = {c->C.n_pub ? pub : nullptr, c->C.n_pub};
    return prove_batch_entropy(ctx, G, c->C, count, seeds32, label, llen, proofs_out, V_out, &in);
  });
}

int bpp_circuit_prove_batch(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, size_t count, const uint8_t* v,
                            const uint8_t* aux, const uint8_t* gammas, const uint8_t* seeds32, const uint8_t* label,
                            size_t llen, uint8_t* proofs_out, uint8_t* V_out) {
  BPP_TRY(no_pub(ctx, c));
  return bpp_circuit_prove_batch_pub(ctx, G, c, count, v, aux, nullptr, gammas, seeds32, label, llen, proofs_out,
                                     V_out);
}

int bpp_circuit_verify_pub(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, const uint8_t* label, size_t llen,
                           const uint8_t* proof, size_t proof_len, const uint8_t* V, const uint8_t* pub) {
  size_t bad = 0;
  return verify_entry({ctx, G, label, llen, 1, proof, V, pub}, c != nullptr, proof_len == bpp_circuit_proof_len(c),
                      [&] { return pub_check(c, 1, pub, &bad); }, [&]() -> const perm::Circuit& { return c->C; });
}

int bpp_circuit_verify_batch_pub(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, size_t count,
                                 const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                                 const uint8_t* pub) {
  size_t bad = 0;
  return verify_entry({ctx, G, label, llen, count, proofs, V, pub}, c != nullptr, true,
                      [&] { return pub_check(c, count, pub, &bad); }, [&]() -> const perm::Circuit& { return c->C; });
}

int bpp_circuit_verify_batch_each_pub(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, size_t count,
                                      const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                                      const uint8_t* pub, uint8_t* ok_out) {
  size_t bad = 0;
  return verify_entry({ctx, G, label, llen, count, proofs, V, pub, true, ok_out}, c != nullptr, true,
                      [&] { return pub_check(c, count, pub, &bad); }, [&]() -> const perm::Circuit& { return c->C; });
}

int bpp_circuit_verify(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, const uint8_t* label, size_t llen,
                       const uint8_t* proof, size_t proof_len, const uint8_t* V) {
  BPP_TRY(no_pub(ctx, c));
  return bpp_circuit_verify_pub(ctx, G, c, label, llen, proof, proof_len, V, nullptr);
}

int bpp_circuit_verify_batch(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, size_t count, const uint8_t* label,
                             size_t llen, const uint8_t* proofs, const uint8_t* V) {
  BPP_TRY(no_pub(ctx, c));
  return bpp_circuit_verify_batch_pub(ctx, G, c, count, label, llen, proofs, V, nullptr);
}

int bpp_circuit_verify_batch_each(bpp_ctx* ctx, const bpp_gens* G, const bpp_circuit* c, size_t count,
                                  const uint8_t* label, size_t llen, const uint8_t* proofs, const uint8_t* V,
                                  uint8_t* ok_out) {
  if (ok_out && count) memset(ok_out, 0, count);
  BPP_TRY(no_pub(ctx, c));
  return bpp_circuit_verify_batch_each_pub(ctx, G, c, count, label, llen, proofs, V, nullptr, ok_out);
}

}  // extern "C"
