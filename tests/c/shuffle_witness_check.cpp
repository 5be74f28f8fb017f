// Host side of bpp_perm_prove_shuffle_batch under ASan + UBSan
// (tests/test_shuffle_host.py): perm::witness over a caller's deck
// (host/perm_circuit.cpp, the k > 768 path) and draw_prover_host_x8 without
// the pi stream.
//   - cards = 1..k gives the seeded witness, value for value;
//   - over random full-width decks with 0, l - 1 and a repeated card, every
//     gate has a_O = a_L a_R, the chains start at v - x, and the last gate's
//     a_L (prod A - prod B) is zero for a true shuffle, nonzero once one
//     output card is changed;
//   - with_pi = false draws the same alpha, beta, rho, tau and leaves pi alone.
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
static bool eqv(const std::vector<Sc>& a, const std::vector<Sc>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!eq(a[i], b[i])) return false;
  return true;
}

int main() {
  uint64_t s = 0x5eed;
  long bad = 0;
  for (uint32_t k : {2u, 3u, 5u, 8u, 52u, 769u}) {
    const perm::Circuit C = perm::build(k);
    perm::Rng rng("shuffle-witness-check", (uint64_t)k);
    const std::vector<uint32_t> pi = perm::fisher_yates(k, rng);
    const Sc x = rnd(s);
    std::vector<Sc> v0, l0, r0, o0, v1, l1, r1, o1;
    // the seeded deck
    std::vector<Sc> cards(k);
    for (uint32_t i = 0; i < k; ++i) cards[i] = hsc::from_u64(i + 1);
    perm::witness(C, pi, x, v0, l0, r0, o0);
    perm::witness(C, cards.data(), pi, x, v1, l1, r1, o1);
    bad += !eqv(v0, v1) + !eqv(l0, l1) + !eqv(r0, r1) + !eqv(o0, o1);
    // a full-width deck with edge cards
    for (auto& c : cards) c = rnd(s);
    cards[0] = hsc::zero();
    cards[1] = hsc::neg(hsc::one());
    if (k > 3) cards[3] = cards[2];
    perm::witness(C, cards.data(), pi, x, v1, l1, r1, o1);
    bad += v1.size() != C.m || l1.size() != C.n_p;
    for (uint32_t i = 0; i < k; ++i) bad += !eq(v1[i], cards[i]) + !eq(v1[k + i], cards[pi[i]]);
    bad += !eq(v1[2 * k], x);
    for (uint32_t g = 0; g < C.n_p; ++g) bad += !eq(o1[g], hsc::mul(l1[g], r1[g]));
    bad += !eq(l1[0], hsc::sub(cards[0], x)) + !eq(l1[k - 1], hsc::sub(cards[pi[0]], x));
    bad += !hsc::is_zero(l1[2 * k - 1]);
    for (uint32_t g = 2 * k; g < C.n_p; ++g) bad += !hsc::is_zero(l1[g]) + !hsc::is_zero(r1[g]);
    // not a shuffle: one output card replaced (through a perm that repeats an index)
    std::vector<uint32_t> pj = pi;
    pj[k - 1] = pj[0];
    if (!eq(cards[pi[k - 1]], cards[pi[0]])) {
      perm::witness(C, cards.data(), pj, x, v1, l1, r1, o1);
      bad += hsc::is_zero(l1[2 * k - 1]);
    }
  }
  // the host's share of the draws without the pi stream
  {
    const perm::Circuit C = perm::build(52);
    perm::Seed sd[8];
    perm::RandomDraws a[8], b[8];
    perm::RandomDraws *ap[8], *bp[8];
    for (int j = 0; j < 8; ++j) {
      uint8_t e[32];
      for (int i = 0; i < 32; ++i) e[i] = (uint8_t)(17 * j + i);
      sd[j] = perm::Seed::bytes32(e);
      ap[j] = &a[j];
      bp[j] = &b[j];
      b[j].pi.assign(52, 7u);
    }
    perm::draw_prover_host_x8(C, sd, ap);
    perm::draw_prover_host_x8(C, sd, bp, false);
    for (int j = 0; j < 8; ++j) {
      bad += !eq(a[j].alpha, b[j].alpha) + !eq(a[j].beta, b[j].beta) + !eq(a[j].rho, b[j].rho) + !eqv(a[j].taus, b[j].taus);
      bad += a[j].pi.size() != 52 || b[j].pi != std::vector<uint32_t>(52, 7u);
      bad += !eq(a[j].alpha, perm::draw_scalar(sd[j], perm::draw_alpha_index(C)));
    }
  }
  printf("mismatches: %ld\n", bad);
  return bad ? 1 : 0;
}
