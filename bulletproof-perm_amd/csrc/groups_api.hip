// Mixed batches: the C ABI (bpp_verify_groups, _each; include/bpperm.h) --
// every group's argument checks, as its kind's own entry points make them, and
// the statements the groups name.  The verifier is perm_verify.hip
// verify_groups.
#include <string>

#include "perm_internal.h"

using namespace perm_impl;

namespace {

// Both entry points: every refusal for the arguments comes before any device
// work and before any context's job generation moves; ok_out (each) never
// keeps a pass of a call that fails.
int groups_entry(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_group* groups, size_t n, bool each,
                 uint8_t* ok_out) {
  return bpp_guard(ctx, [&]() -> int {
    if (n > BPP_VERIFY_GROUPS_MAX) return BPP_ERR_LEN;
    if (!ctx || !G || (!groups && n)) return BPP_ERR_ARG;
    size_t total = 0;
    for (size_t g = 0; g < n; ++g) total += groups[g].count;
    if (each && !ok_out && total) return BPP_ERR_ARG;
    ok_clear(ok_out, total);  // (nullptr unless each)
    auto named = [&](size_t g, int rc) {  // (keeps a text the check itself left)
      ctx->err = "group " + std::to_string(g) + (ctx->err.empty() ? "" : ": " + ctx->err);
      return rc;
    };
    for (size_t g = 0; g < n; ++g) {
      const bpp_verify_group& a = groups[g];
      ctx->err.clear();
      if (((!a.proofs || !a.V) && a.count) || (!a.label && a.label_len)) return named(g, BPP_ERR_ARG);
      switch (a.kind) {
        case BPP_STMT_PERM:
          if (!k_in_range(a.k)) return named(g, BPP_ERR_ARG);
          break;
        case BPP_STMT_DECK:
          if (!k_in_range(a.k)) return named(g, BPP_ERR_ARG);
          if (int rc = deck_canonical(ctx, a.k, a.deck)) return named(g, rc);
          break;
        case BPP_STMT_CIRCUIT: {
          if (!a.circuit) return named(g, BPP_ERR_ARG);
          if (a.pub && !a.circuit->C.n_pub) {
            ctx->err = "public inputs given for a circuit that has none";
            return named(g, BPP_ERR_ARG);
          }
          size_t bad = 0;
          if (int rc = pub_check(a.circuit, a.count, a.pub, &bad)) {
            if (rc == BPP_ERR_NONCANONICAL) ctx->err = "proof " + std::to_string(bad) + ": non-canonical public input";
            return named(g, rc);
          }
          break;
        }
        default:
          ctx->err = "unknown statement kind";
          return named(g, BPP_ERR_ARG);
      }
    }
    if (!total) return BPP_OK;
    // the statements: built for the call (a circuit handle is the caller's)
    std::vector<perm::Circuit> built;
    built.reserve(n);
    VerifyGroup vg[BPP_VERIFY_GROUPS_MAX];
    for (size_t g = 0; g < n; ++g) {
      const bpp_verify_group& a = groups[g];
      const perm::Circuit* C = nullptr;
      if (a.kind == BPP_STMT_CIRCUIT) {
        C = &a.circuit->C;
      } else if (a.count) {
        built.push_back(a.kind == BPP_STMT_PERM ? perm::build(a.k) : perm::build_deck(a.k, a.deck));
        C = &built.back();
      }
      vg[g] = {C, a.label, a.label_len, a.count, a.proofs, a.V, a.pub};
    }
    BPP_HIP(hipSetDevice(ctx->device));
    return ok_settle(verify_groups(ctx, G, vg, n, ok_out), ok_out, total);
  });
}

}  // namespace

extern "C" {

int bpp_verify_groups(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_group* groups, size_t n_groups) {
  return groups_entry(ctx, G, groups, n_groups, false, nullptr);
}

int bpp_verify_groups_each(bpp_ctx* ctx, const bpp_gens* G, const bpp_verify_group* groups, size_t n_groups,
                           uint8_t* ok) {
  return groups_entry(ctx, G, groups, n_groups, true, ok);
}

}  // extern "C"
