// Host side of bpp_circuit_*_pub under ASan + UBSan (tests/test_circuit_pub_host.py):
// circuit::compile, circuit::digest and circuit::eval of csrc/host/circuit.cpp
// with public inputs.
//   - a circuit with a free gate, defined sides and asserts reading u_0, u_1:
//     W_U's entries and signs, every row q of W_L a_L + W_R a_R + W_O a_O =
//     W_V v + c + W_U u holds for the evaluated witness over u in {0, l - 1,
//     random}; one wrong public input makes eval name the assert and violates
//     its row alone;
//   - n_pub = 0 through the same path: the digest and rows of the plain compile;
//     n_pub = 1, 2 over the same arrays: three different digests;
//   - every refusal: its code, and no circuit left behind.
#include <algorithm>
#include <cstdio>
#include <cstring>
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

struct Builder {
  uint32_t m_in = 0, n = 0, n_aux = 0, A = 0, n_pub = 0;
  std::vector<uint32_t> side_aux, lc_off{0}, lc_var;
  std::vector<Sc> lc_coef;
  void term(uint32_t var, const Sc& c) {
    lc_var.push_back(var);
    lc_coef.push_back(c);
  }
  void end() { lc_off.push_back((uint32_t)lc_var.size()); }
  circuit::Desc desc() const {
    circuit::Desc d = {m_in, n, n_aux, A, side_aux.data(), lc_off.data(), lc_var.data(), (const uint8_t*)lc_coef.data()};
    d.n_pub = n_pub;
    return d;
  }
};

static std::vector<uint32_t> violated(const perm::Circuit& C, const std::vector<Sc>& v, const std::vector<Sc>& aL,
                                      const std::vector<Sc>& aR, const std::vector<Sc>& aO, const std::vector<Sc>& u,
                                      const Sc& x) {
  std::vector<Sc> lhs(C.Q, hsc::zero()), rhs = C.c;
  rhs[C.Q - 1] = hsc::neg(x);
  for (const perm::Entry& e : C.WL) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aL[e.col]));
  for (const perm::Entry& e : C.WR) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aR[e.col]));
  for (const perm::Entry& e : C.WO) lhs[e.q] = hsc::add(lhs[e.q], hsc::mul(e.val, aO[e.col]));
  for (const perm::Entry& e : C.WV) rhs[e.q] = hsc::add(rhs[e.q], hsc::mul(e.val, v[e.col]));
  for (const perm::Entry& e : C.WU) rhs[e.q] = hsc::add(rhs[e.q], hsc::mul(e.val, u[e.col]));
  std::vector<uint32_t> out;
  for (uint32_t q = 0; q < C.Q; ++q)
    if (!eq(lhs[q], rhs[q])) out.push_back(q);
  return out;
}

// m_in = 2, n_pub = 2, 3 gates: gate 0 free (aux 0, 1); gate 1 = (v_0 - x + 3 u_0)(o_0 + 2 u_1 + 5);
// gate 2 = (o_1)(v_1 - u_0); asserts: l_0 - u_1 = 0 (the free side is the public u_1), v_0 + v_1 - 7 u_0 - u_1 + 1 = 0
static Builder mixed() {
  Builder b;
  b.m_in = 2, b.n = 3, b.n_aux = 2, b.n_pub = 2, b.A = 2;
  const Sc one = hsc::one(), neg1 = hsc::neg(one);
  auto w = [&](uint32_t h, uint32_t lro) { return circuit::var_wire(2, h, lro, 2); };
  b.side_aux = {0, 1, circuit::SIDE_LC, circuit::SIDE_LC, circuit::SIDE_LC, circuit::SIDE_LC};
  b.end(), b.end();
  b.term(circuit::var_v(0), one), b.term(circuit::var_x(2), neg1), b.term(circuit::var_pub(2, 0), hsc::from_u64(3)), b.end();
  b.term(circuit::var_one(), hsc::from_u64(5)), b.term(circuit::var_pub(2, 1), hsc::from_u64(2)), b.term(w(0, 2), one), b.end();
  b.term(w(1, 2), one), b.end();
  b.term(circuit::var_v(1), one), b.term(circuit::var_pub(2, 0), neg1), b.end();
  b.term(circuit::var_pub(2, 1), neg1), b.term(w(0, 0), one), b.end();
  b.term(circuit::var_one(), one), b.term(circuit::var_v(0), one), b.term(circuit::var_v(1), one),
      b.term(circuit::var_pub(2, 0), hsc::neg(hsc::from_u64(7))), b.term(circuit::var_pub(2, 1), neg1), b.end();
  return b;
}

int main() {
  uint64_t s = 0x9b1c;
  long bad = 0;
  std::string err;
  {
    const Builder b = mixed();
    perm::Circuit C;
    bad += circuit::compile(b.desc(), C, err) != circuit::OK;
    bad += C.n != 3 || C.n_p != 4 || C.Q != 4 + 2 + 1 || C.m != 3 || C.nv != 2 || C.n_pub != 2 || !C.program ||
           C.program->n_pub != 2;
    // W_U: rows 0, 1 = the left sides of gates 1, 2; rows 2, 3 = their right sides; rows 4, 5 = the asserts
    struct E { uint32_t q, col; Sc val; };
    const Sc neg1 = hsc::neg(hsc::one());
    const std::vector<E> want = {{0, 0, hsc::from_u64(3)}, {2, 1, hsc::from_u64(2)}, {3, 0, neg1},
                                 {4, 1, hsc::one()},       {5, 0, hsc::from_u64(7)}, {5, 1, hsc::one()}};
    bad += C.WU.size() != want.size();
    for (size_t i = 0; i < want.size() && i < C.WU.size(); ++i)
      bad += C.WU[i].q != want[i].q || C.WU[i].col != want[i].col || !eq(C.WU[i].val, want[i].val) ||
             !eq(C.WU[i].valR, hsc::to_mont(want[i].val));
    const Sc lm1 = hsc::neg(hsc::one());
    for (int kind = 0; kind < 6; ++kind) {
      // u_0, u_1 over {0, l - 1, random}
      const Sc u0 = kind % 3 == 0 ? hsc::zero() : kind % 3 == 1 ? lm1 : rnd(s);
      const Sc u1 = kind < 2 ? rnd(s) : kind < 4 ? hsc::zero() : lm1;
      const Sc x = rnd(s), v0 = rnd(s);
      // v_1 = 7 u_0 + u_1 - 1 - v_0
      const Sc v1 = hsc::sub(hsc::sub(hsc::add(hsc::mul(hsc::from_u64(7), u0), u1), hsc::one()), v0);
      std::vector<Sc> v = {v0, v1, x}, aux = {u1, rnd(s)}, u = {u0, u1}, aL, aR, aO;
      uint32_t ba = 9;
      circuit::eval(*C.program, C.n_p, v.data(), aux.data(), x, aL, aR, aO, &ba, u.data());
      bad += ba != 0 || !violated(C, v, aL, aR, aO, u, x).empty() || aL.size() != 4;
      for (uint32_t g = 0; g < 3; ++g) bad += !eq(aO[g], hsc::mul(aL[g], aR[g]));
      bad += !eq(aL[1], hsc::add(hsc::sub(v0, x), hsc::mul(hsc::from_u64(3), u0)));
      bad += !eq(aR[2], hsc::sub(v1, u0)) || !hsc::is_zero(aL[3]) || !hsc::is_zero(aO[3]);
      // another u_1: the witness (evaluated under it) breaks assert 0 first, and both asserts' rows
      std::vector<Sc> u2 = {u0, hsc::add(u1, hsc::one())};
      circuit::eval(*C.program, C.n_p, v.data(), aux.data(), x, aL, aR, aO, &ba, u2.data());
      const std::vector<uint32_t> rows = violated(C, v, aL, aR, aO, u2, x);
      bad += ba != 1 || rows != std::vector<uint32_t>({4, 5});
      // another u_0: assert 1 alone (row 5)
      std::vector<Sc> u3 = {hsc::add(u0, hsc::one()), u1};
      circuit::eval(*C.program, C.n_p, v.data(), aux.data(), x, aL, aR, aO, &ba, u3.data());
      bad += ba != 2 || violated(C, v, aL, aR, aO, u3, x) != std::vector<uint32_t>({5});
    }
  }
  {  // n_pub = 0, 1, 2 over arrays without a public term or a wire: the first is the plain digest
    Builder b;
    b.m_in = 1, b.n = 1, b.A = 1;
    b.side_aux = {circuit::SIDE_LC, circuit::SIDE_LC};
    b.term(circuit::var_v(0), hsc::one()), b.end();
    b.term(circuit::var_one(), hsc::one()), b.end();
    b.term(circuit::var_one(), hsc::neg(hsc::from_u64(4))), b.term(circuit::var_v(0), hsc::from_u64(2)), b.end();
    uint8_t dg[3][32], plain[32];
    for (uint32_t np = 0; np < 3; ++np) {
      b.n_pub = np;
      perm::Circuit C;
      bad += circuit::compile(b.desc(), C, err) != circuit::OK || C.n_pub != np || !C.WU.empty();
      memcpy(dg[np], C.program_digest, 32);
    }
    b.n_pub = 0;
    circuit::Desc d = b.desc();
    circuit::digest(d, plain);
    bad += memcmp(plain, dg[0], 32) != 0;
    bad += !memcmp(dg[0], dg[1], 32) || !memcmp(dg[0], dg[2], 32) || !memcmp(dg[1], dg[2], 32);
  }
  auto refuse = [&](const Builder& b, int want) {
    perm::Circuit C;
    const int rc = circuit::compile(b.desc(), C, err);
    bad += rc != want || C.program;
  };
  {
    Builder b = mixed();
    b.side_aux[2] = 0, refuse(b, circuit::ERR_ARG);                       // a free side with a public term
    b = mixed(), b.n_pub = 1, refuse(b, circuit::ERR_ARG);                // wire ids shifted by the wrong n_pub: gate 1 reads "o_0" = l_1
    b = mixed(), b.lc_var.back() = circuit::var_wire(2, 3, 0, 2), refuse(b, circuit::ERR_ARG);  // id out of range
    b = mixed(), b.lc_var[2] = circuit::var_pub(2, 0), b.lc_var[1] = circuit::var_pub(2, 1), refuse(b, circuit::ERR_ARG);  // unsorted
    b = mixed(), b.n_pub = (1u << 16) + 1, refuse(b, circuit::ERR_LEN);
    b = mixed(), b.lc_coef[2] = hsc::L, refuse(b, circuit::ERR_NONCANONICAL);
    b = mixed(), b.lc_coef[2] = hsc::zero(), refuse(b, circuit::ERR_ARG);
  }
  {  // n_pub = 2^16 is taken
    Builder b = mixed();
    // ids of the wires move with n_pub: rebuild them
    const uint32_t np = 1u << 16;
    for (uint32_t& v : b.lc_var)
      if (v >= 2 + 2 + 2) v += np - 2;
    b.n_pub = np;
    perm::Circuit C;
    bad += circuit::compile(b.desc(), C, err) != circuit::OK || C.n_pub != np || C.WU.size() != 6;
  }
  printf("mismatches: %ld\n", bad);
  return bad ? 1 : 0;
}
