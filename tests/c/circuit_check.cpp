// Host side of bpp_circuit_* under ASan + UBSan (tests/test_circuit_host.py):
// circuit::compile, circuit::digest and circuit::eval of
// csrc/host/circuit.cpp.
//   - the two-half circuit written as a program compiles to perm::build(k)'s
//     entries (as sorted triplets) and c, for k = 2..9 and 52;
//   - a circuit with free sides, asserts and every kind of term: every row q
//     of W_L a_L + W_R a_R + W_O a_O = W_V v + c holds for the evaluated
//     witness, padding gates are zero, the level schedule covers every gate
//     once; one wrong input makes eval name the assert and violates its row;
//   - every refusal: its code, and no circuit left behind;
//   - the digest changes with a coefficient.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <tuple>
#include <vector>

#include "host/circuit.h"

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

// a description under construction: one combination after another
struct Builder {
  uint32_t m_in = 0, n = 0, n_aux = 0, A = 0;
  std::vector<uint32_t> side_aux, lc_off{0}, lc_var;
  std::vector<Sc> lc_coef;
  void term(uint32_t var, const Sc& c) {
    lc_var.push_back(var);
    lc_coef.push_back(c);
  }
  void end() { lc_off.push_back((uint32_t)lc_var.size()); }
  circuit::Desc desc() const {
    return {m_in, n, n_aux, A, side_aux.data(), lc_off.data(), lc_var.data(), (const uint8_t*)lc_coef.data()};
  }
};

static Builder two_half(uint32_t k) {
  Builder b;
  b.m_in = 2 * k, b.n = 2 * k, b.A = 1;
  const Sc one = hsc::one(), neg1 = hsc::neg(one);
  auto o = [&](uint32_t h) { return circuit::var_wire(b.m_in, h, 2); };
  for (uint32_t g = 0; g < 2 * k; ++g) {
    b.side_aux.insert(b.side_aux.end(), {circuit::SIDE_LC, circuit::SIDE_LC});
    // left
    if (g == 0 || g == k - 1) {
      b.term(circuit::var_v(g == 0 ? 0 : k), one);
      b.term(circuit::var_x(b.m_in), neg1);
    } else if (g == 2 * k - 1) {
      b.term(o(k - 2), one);
      b.term(o(2 * k - 2), one);
    } else {
      b.term(o(g - 1), one);
    }
    b.end();
    // right
    if (g + 2 < 2 * k) {
      b.term(circuit::var_v(g + 2 <= k ? g + 1 : g + 2), one);
      b.term(circuit::var_x(b.m_in), neg1);
    } else {
      b.term(circuit::var_one(), g == 2 * k - 2 ? neg1 : one);
    }
    b.end();
  }
  b.term(o(2 * k - 1), one);
  b.end();
  return b;
}

typedef std::tuple<uint32_t, uint32_t, std::array<uint64_t, 4>> Trip;
static std::vector<Trip> sorted(const std::vector<perm::Entry>& W) {
  std::vector<Trip> t;
  for (const perm::Entry& e : W) t.push_back({e.q, e.col, {e.val.v[0], e.val.v[1], e.val.v[2], e.val.v[3]}});
  std::sort(t.begin(), t.end());
  return t;
}

static std::vector<uint32_t> violated(const perm::Circuit& C, const std::vector<Sc>& v, const std::vector<Sc>& aL,
                                      const std::vector<Sc>& aR, const std::vector<Sc>& aO, const Sc& x) {
  std::vector<Sc> lhs(C.Q, hsc::zero()), rhs = C.c;
  rhs[C.Q - 1] = hsc::neg(x);
  for (const perm::Entry& e : C.WL) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aL[e.col]));
  for (const perm::Entry& e : C.WR) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aR[e.col]));
  for (const perm::Entry& e : C.WO) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aO[e.col]));
  for (const perm::Entry& e : C.WV) rhs[e.q] = hsc::add(rhs[e.q], hsc::mul(e.val, v[e.col]));
  std::vector<uint32_t> out;
  for (uint32_t q = 0; q < C.Q; ++q)
    if (!eq(lhs[q], rhs[q])) out.push_back(q);
  return out;
}

// v_0 < 8 by three free bit gates, then gate 3 = (v_1 - x + 5)(2 l_0 + 3 r_1 + o_2 + v_0), an assert on it
static Builder mixed() {
  Builder b;
  b.m_in = 2, b.n = 4, b.n_aux = 6;
  const Sc one = hsc::one(), neg1 = hsc::neg(one);
  for (uint32_t i = 0; i < 3; ++i) {
    b.side_aux.insert(b.side_aux.end(), {2 * i, 2 * i + 1});
    b.end();
    b.end();
  }
  b.side_aux.insert(b.side_aux.end(), {circuit::SIDE_LC, circuit::SIDE_LC});
  b.term(circuit::var_one(), hsc::from_u64(5));
  b.term(circuit::var_v(1), one);
  b.term(circuit::var_x(2), neg1);
  b.end();
  b.term(circuit::var_v(0), one);
  b.term(circuit::var_wire(2, 0, 0), hsc::from_u64(2));
  b.term(circuit::var_wire(2, 1, 1), hsc::from_u64(3));
  b.term(circuit::var_wire(2, 2, 2), one);
  b.end();
  for (uint32_t i = 0; i < 3; ++i) {  // o_i = 0, l_i + r_i - 1 = 0
    b.term(circuit::var_wire(2, i, 2), one);
    b.end();
    b.term(circuit::var_one(), neg1);
    b.term(circuit::var_wire(2, i, 0), one);
    b.term(circuit::var_wire(2, i, 1), one);
    b.end();
  }
  b.term(circuit::var_v(0), neg1);  // l_0 + 2 l_1 + 4 l_2 - v_0 = 0
  for (uint32_t i = 0; i < 3; ++i) b.term(circuit::var_wire(2, i, 0), hsc::from_u64(1u << i));
  b.end();
  b.A = 7;
  return b;
}

int main() {
  uint64_t s = 0xc19c;
  long bad = 0;
  std::string err;
  for (uint32_t k : {2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 52u}) {
    const Builder b = two_half(k);
    perm::Circuit C;
    bad += circuit::compile(b.desc(), C, err) != circuit::OK;
    const perm::Circuit W = perm::build(k);
    bad += C.n != W.n || C.n_p != W.n_p || C.lg != W.lg || C.Q != W.Q || C.m != W.m || C.nv != W.nv || !C.program;
    bad += sorted(C.WL) != sorted(W.WL) || sorted(C.WR) != sorted(W.WR) || sorted(C.WO) != sorted(W.WO) ||
           sorted(C.WV) != sorted(W.WV);
    for (uint32_t q = 0; q < W.Q; ++q) bad += !eq(C.c[q], W.c[q]);
    bad += perm::proof_len(C) != perm::proof_len(k);
    // the host witness equals the two-half circuit's own over the same cards
    std::vector<Sc> cards(k), v, aL, aR, aO, wL, wR, wO;
    for (Sc& c : cards) c = rnd(s);
    perm::Rng rng("circuit-check", (uint64_t)k);
    const std::vector<uint32_t> pi = perm::fisher_yates(k, rng);
    const Sc x = rnd(s);
    perm::witness(W, cards.data(), pi, x, v, wL, wR, wO);
    uint32_t ba = 9;
    circuit::eval(*C.program, C.n_p, v.data(), nullptr, x, aL, aR, aO, &ba);
    bad += ba != 0 || aL.size() != C.n_p;
    for (uint32_t g = 0; g < C.n_p; ++g) bad += !eq(aL[g], wL[g]) || !eq(aR[g], wR[g]) || !eq(aO[g], wO[g]);
    bad += !violated(C, v, aL, aR, aO, x).empty();
    // the schedule: a chain per half, every gate once
    std::vector<uint32_t> seen(C.n, 0);
    for (uint32_t g : C.program->level_gate) bad += g >= C.n || seen[g]++;
    bad += C.program->level_off.back() != C.n || C.program->level_off.size() != (size_t)k + 2;
  }
  {
    const Builder b = mixed();
    perm::Circuit C;
    bad += circuit::compile(b.desc(), C, err) != circuit::OK;
    bad += C.n != 4 || C.n_p != 4 || C.Q != 2 + 7 + 1 || C.m != 3 || C.nv != 2;
    for (uint32_t val = 0; val < 8; ++val) {
      const Sc x = rnd(s);
      std::vector<Sc> v = {hsc::from_u64(val), rnd(s), x}, aux(6), aL, aR, aO;
      for (uint32_t i = 0; i < 3; ++i) {
        aux[2 * i] = hsc::from_u64((val >> i) & 1);
        aux[2 * i + 1] = hsc::from_u64(1 - ((val >> i) & 1));
      }
      uint32_t ba = 9;
      circuit::eval(*C.program, C.n_p, v.data(), aux.data(), x, aL, aR, aO, &ba);
      bad += ba != 0 || !violated(C, v, aL, aR, aO, x).empty();
      for (uint32_t g = 0; g < 4; ++g) bad += !eq(aO[g], hsc::mul(aL[g], aR[g]));
      v[0] = hsc::from_u64(val + 8);  // out of range: the bit sum (assert 6, row 2 + 6) alone
      circuit::eval(*C.program, C.n_p, v.data(), aux.data(), x, aL, aR, aO, &ba);
      const std::vector<uint32_t> rows = violated(C, v, aL, aR, aO, x);
      bad += ba != 7 || rows.size() != 1 || rows[0] != 8;
    }
    // the digest binds every coefficient
    Builder d = b;
    d.lc_coef[3] = hsc::add(d.lc_coef[3], hsc::one());
    perm::Circuit D;
    bad += circuit::compile(d.desc(), D, err) != circuit::OK;
    bad += memcmp(C.program_digest, D.program_digest, 32) == 0;
  }
  // refusals
  auto refuse = [&](const Builder& b, int want) {
    perm::Circuit C;
    const int rc = circuit::compile(b.desc(), C, err);
    bad += rc != want || C.program;
  };
  {
    Builder b = mixed();
    b.m_in = 0;
    refuse(b, circuit::ERR_ARG);
    b = mixed(), b.n = 0, refuse(b, circuit::ERR_ARG);
    b = mixed(), b.lc_var[1] = 2 + 2 + 3 * 4, refuse(b, circuit::ERR_ARG);           // id out of range
    b = mixed(), b.side_aux[0] = 6, refuse(b, circuit::ERR_ARG);                     // aux out of range
    b = mixed(), b.lc_var[5] = circuit::var_wire(2, 3, 0), refuse(b, circuit::ERR_ARG);  // gate 3 reads l_3
    b = mixed(), std::swap(b.lc_var[4], b.lc_var[5]), refuse(b, circuit::ERR_ARG);   // unsorted
    b = mixed(), b.lc_var[5] = b.lc_var[4], refuse(b, circuit::ERR_ARG);             // duplicate
    b = mixed(), b.lc_coef[2] = hsc::zero(), refuse(b, circuit::ERR_ARG);            // zero coefficient
    b = mixed(), b.lc_off[8] = b.lc_off[7] - 1, refuse(b, circuit::ERR_ARG);         // non-monotone
    b = mixed(), b.side_aux[6] = 0, refuse(b, circuit::ERR_ARG);                     // a free side with terms
    b = mixed(), b.lc_coef[2] = hsc::L, refuse(b, circuit::ERR_NONCANONICAL);
    // 683 free gates: the witness kernel's LDS; 512 defined gates and 500 asserts: the row tables'
    Builder big;
    big.m_in = 1, big.n = 683, big.n_aux = 2;
    for (uint32_t g = 0; g < 683; ++g) {
      big.side_aux.insert(big.side_aux.end(), {0u, 1u});
      big.end(), big.end();
    }
    refuse(big, circuit::ERR_LEN);
    Builder rows;
    rows.m_in = 1, rows.n = 512;
    for (uint32_t g = 0; g < 512; ++g) {
      rows.side_aux.insert(rows.side_aux.end(), {circuit::SIDE_LC, circuit::SIDE_LC});
      rows.term(circuit::var_v(0), hsc::one()), rows.end();
      rows.term(circuit::var_v(0), hsc::one()), rows.end();
    }
    {
      perm::Circuit C;  // 512 gates, both sides defined: supported
      bad += circuit::compile(rows.desc(), C, err) != circuit::OK || C.Q != 1025 || C.n_p != 512;
    }
    rows.A = 483;  // Q = 1508
    for (uint32_t a = 0; a < rows.A; ++a) rows.term(circuit::var_v(0), hsc::one()), rows.end();
    refuse(rows, circuit::ERR_LEN);
  }
  printf("mismatches: %ld\n", bad);
  return bad ? 1 : 0;
}
