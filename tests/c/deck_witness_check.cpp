// Host side of bpp_deck_prove_batch / bpp_deck_verify* under ASan + UBSan
// (tests/test_deck_host.py): perm::build_deck, perm::witness_deck (the
// k > 1536 path) and perm::deck_product (the host replay's c[Q-2]).
//   - the circuit's shape: n = k - 1, Q = 2k, m = k + 1, nv = k, n_p =
//     max(4, next_pow2(k - 1)), proof_len = 32 (13 + 2 lg);
//   - over the default deck and full-width decks with 0, l - 1 and a repeated
//     card, every row q of W_L a_L + W_R a_R + W_O a_O = W_V v + c holds with
//     c[Q-2] = deck_product(x), c[Q-1] = -x; padding gates are zero;
//   - one output card changed violates row 2k - 2 and nothing else;
//   - the deck digest changes with a card and with k.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/perm.h"

using hsc::Sc;

static Sc rnd(uint64_t& s) {
  uint8_t b[64];
  for (int i = 0; i < 64; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    b[i] = (uint8_t)(s >> 56);
  }
  return hsc::from_wide(b);
}

static bool eq(const Sc& a, const Sc& b) { return memcmp(&a, &b, sizeof(Sc)) == 0; }

// rows that do not hold
static std::vector<uint32_t> violated(const perm::Circuit& C, const std::vector<Sc>& v, const std::vector<Sc>& aL,
                                      const std::vector<Sc>& aR, const std::vector<Sc>& aO, const Sc& x) {
  std::vector<Sc> lhs(C.Q, hsc::zero()), rhs = C.c;
  rhs[C.Q - 1] = hsc::neg(x);
  rhs[C.Q - 2] = perm::deck_product(C, x);
  for (const perm::Entry& e : C.WL) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aL[e.col]));
  for (const perm::Entry& e : C.WR) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aR[e.col]));
  for (const perm::Entry& e : C.WO) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aO[e.col]));
  for (const perm::Entry& e : C.WV) rhs[e.q] = hsc::add(rhs[e.q], hsc::mul(e.val, v[e.col]));
  std::vector<uint32_t> out;
  for (uint32_t q = 0; q < C.Q; ++q)
    if (!eq(lhs[q], rhs[q])) out.push_back(q);
  return out;
}

int main() {
  uint64_t s = 0xdec4;
  long bad = 0;
  for (uint32_t k : {2u, 3u, 5u, 6u, 9u, 52u, 1537u}) {
    for (int full = 0; full < 2; ++full) {
      std::vector<Sc> cards(k);
      for (uint32_t i = 0; i < k; ++i) cards[i] = full ? rnd(s) : hsc::from_u64(i + 1);
      if (full) {
        cards[0] = hsc::zero();
        cards[1] = hsc::neg(hsc::one());
        if (k > 3) cards[3] = cards[2];
      }
      const perm::Circuit C = perm::build_deck(k, full ? (const uint8_t*)cards.data() : nullptr);
      uint32_t n_p = 4, lg = 2;
      for (; n_p < k - 1; n_p *= 2) ++lg;
      bad += !C.deck || C.n != k - 1 || C.Q != 2 * k || C.m != k + 1 || C.nv != k || C.n_p != n_p || C.lg != lg;
      bad += perm::proof_len(C) != 32 * (13 + 2 * (size_t)lg) || C.cards.size() != k || C.c.size() != C.Q;
      for (uint32_t i = 0; i < k; ++i) bad += !eq(C.cards[i], cards[i]);
      perm::Rng rng("deck-witness-check", (uint64_t)k);
      const std::vector<uint32_t> pi = perm::fisher_yates(k, rng);
      const Sc x = rnd(s);
      std::vector<Sc> v, aL, aR, aO;
      perm::witness_deck(C, pi, x, v, aL, aR, aO);
      bad += v.size() != C.m || aL.size() != C.n_p || aR.size() != C.n_p || aO.size() != C.n_p;
      for (uint32_t i = 0; i < k; ++i) bad += !eq(v[i], cards[pi[i]]);
      bad += !eq(v[k], x);
      for (uint32_t g = 0; g < C.n_p; ++g) bad += !eq(aO[g], hsc::mul(aL[g], aR[g]));
      for (uint32_t g = C.n; g < C.n_p; ++g) bad += !hsc::is_zero(aL[g]) + !hsc::is_zero(aR[g]);
      bad += !violated(C, v, aL, aR, aO, x).empty();
      // not a shuffle of the deck: one output card replaced (a perm that repeats an index)
      std::vector<uint32_t> pj = pi;
      pj[k - 1] = pj[0];
      if (!eq(cards[pi[k - 1]], cards[pi[0]])) {
        perm::witness_deck(C, pj, x, v, aL, aR, aO);
        const std::vector<uint32_t> rows = violated(C, v, aL, aR, aO, x);
        bad += rows.size() != 1 || rows[0] != 2 * k - 2;
      }
      // the digest binds every card and k
      std::vector<Sc> other = cards;
      other[k - 1] = hsc::add(other[k - 1], hsc::one());
      const perm::Circuit D = perm::build_deck(k, (const uint8_t*)other.data());
      bad += memcmp(C.deck_digest, D.deck_digest, 32) == 0;
      other.push_back(hsc::one());
      const perm::Circuit E = perm::build_deck(k + 1, (const uint8_t*)other.data());
      bad += memcmp(D.deck_digest, E.deck_digest, 32) == 0;
    }
  }
  // the two-half circuit keeps its count of pre-challenge commitments
  bad += perm::build(52).nv != 104 || perm::build(52).deck || perm::proof_len(perm::build(52)) != perm::proof_len(52);
  printf("mismatches: %ld\n", bad);
  return bad ? 1 : 0;
}
