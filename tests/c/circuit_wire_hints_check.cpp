// Hints over wires and x on the host under ASan + UBSan
// (tests/test_circuit_wire_hints_host.py): circuit::compile with wire_hints,
// circuit::hint_eval_x and circuit::eval of csrc/host/circuit.cpp.
//   - a chain of n gates whose right sides are late hints of every op over x
//     and over the previous gate's wires, one aux index feeding two sides and
//     one late hint that feeds none: the hints' defining relations hold on the
//     evaluated witness (inv * w = 1, bit + not_bit = 1, is_zero * w = 0), the
//     level schedule covers every gate once and puts every gate above the gates
//     its hint reads, and the device image has the size its tables add up to;
//   - the refusals of the late rule, each with its code, and hint_eval_x on a
//     program without late hints equal to hint_eval.
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

struct Lcs {
  std::vector<uint32_t> off{0}, var;
  std::vector<Sc> coef;
  void term(uint32_t v, const Sc& c) {
    var.push_back(v);
    coef.push_back(c);
  }
  void end() { off.push_back((uint32_t)var.size()); }
};

struct Builder {
  uint32_t m_in = 3, n = 0, n_aux = 0, A = 0;
  std::vector<uint32_t> side_aux, op;
  Lcs d, h;
  uint32_t hint(uint32_t word) {
    op.push_back(word);
    return n_aux++;
  }
  circuit::Desc desc() const {
    return {m_in, n, n_aux, A, side_aux.data(), d.off.data(), d.var.data(), (const uint8_t*)d.coef.data()};
  }
  circuit::HintDesc hints() const { return {op.data(), h.off.data(), h.var.data(), (const uint8_t*)h.coef.data()}; }
};

// gate g: left = v_{g mod 3} + (g + 1) [+ o_{g-1}], right = a late hint cycling through the ops
static Builder chain(uint32_t n) {
  Builder b;
  const Sc one = hsc::one(), neg1 = hsc::neg(one);
  const uint32_t x = circuit::var_x(b.m_in);
  auto w = [&](uint32_t g, uint32_t s) { return circuit::var_wire(b.m_in, g, s); };
  uint32_t unused = b.hint(circuit::kHintInv);  // reads x, feeds no side
  b.h.term(x, one);
  b.h.end();
  (void)unused;
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t kind = g % 5;
    uint32_t t;
    if (g == 0 || kind == 0) {  // INV(x - v_1)
      t = b.hint(circuit::kHintInv);
      b.h.term(circuit::var_v(1), neg1);
      b.h.term(x, one);
    } else if (kind == 1 || kind == 2) {  // BIT / NOT_BIT 7 of l_{g-1}
      t = b.hint((kind == 1 ? circuit::kHintBit : circuit::kHintNotBit) | 7u << 8);
      b.h.term(w(g - 1, 0), one);
    } else if (kind == 3) {  // IS_ZERO(l_{g-1})
      t = b.hint(circuit::kHintIsZero);
      b.h.term(w(g - 1, 0), one);
    } else {  // INV(o_{g-1})
      t = b.hint(circuit::kHintInv);
      b.h.term(w(g - 1, 2), one);
    }
    b.h.end();
    const bool twice = g % 7 == 6;  // the previous gate's aux value on the left side too
    b.side_aux.push_back(twice ? t - 1 : circuit::SIDE_LC);
    if (!twice) {
      b.d.term(circuit::var_one(), hsc::from_u64(g + 1));
      b.d.term(circuit::var_v(g % 3), one);
      if (g) b.d.term(w(g - 1, 2), one);
    }
    b.d.end();
    b.side_aux.push_back(t);
    b.d.end();
    ++b.n;
  }
  return b;
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) {
    if (!ok) {
      ++bad;
      printf("FAIL %s\n", what);
    }
  };
  uint64_t seed = 42;
  for (uint32_t n : {1u, 2u, 7u, 40u, 130u}) {
    Builder b = chain(n);
    circuit::Desc d = b.desc();
    circuit::HintDesc h = b.hints();
    perm::Circuit C;
    std::string err;
    expect(circuit::compile(d, C, err, &h, true) == circuit::OK, "compile");
    if (!C.program) continue;
    expect(circuit::compile(d, C, err, &h, false) == circuit::ERR_ARG, "the old entry point refuses x and wires");
    expect(circuit::compile(d, C, err, &h, true) == circuit::OK, "compile again");
    const circuit::Program& P = *C.program;
    expect(circuit::has_late_hints(P) && P.hints->n_late == b.n_aux, "every hint is late");
    // levels: every gate once, above the gates its definitions and its hint read
    std::vector<uint32_t> level(n, 0xFFFFFFFFu);
    for (uint32_t l = 0; l + 1 < P.level_off.size(); ++l)
      for (uint32_t u = P.level_off[l]; u < P.level_off[l + 1]; ++u) {
        expect(level[P.level_gate[u]] == 0xFFFFFFFFu, "a gate in two levels");
        level[P.level_gate[u]] = l;
      }
    for (uint32_t g = 0; g < n; ++g) {
      expect(level[g] != 0xFFFFFFFFu, "a gate in no level");
      if (g && g % 5 != 0) expect(level[g] > level[g - 1], "a gate not above the gate its hint reads");
    }
    // the image: side_aux, lc_off, lc_wire, level_off, level_gate, late records, ids (padded), coefficients
    size_t fed_terms = 0;
    std::vector<uint8_t> fed(b.n_aux, 0);
    for (uint32_t a : b.side_aux)
      if (a != circuit::SIDE_LC && !fed[a]) {
        fed[a] = 1;
        fed_terms += b.h.off[a + 1] - b.h.off[a];
      }
    const size_t T = b.d.var.size() + fed_terms;
    size_t words = 2 * n + (2 * n + 1) + 2 * n + P.level_off.size() + n + 6 * n + T;
    words = (words + 7) / 8 * 8 + 8 * T;
    expect(P.dev.size() == words && P.dev_late == 2 * n + (2 * n + 1) + 2 * n + P.level_off.size() + n, "image size");
    for (int rep = 0; rep < 3; ++rep) {
      std::vector<Sc> v = {rnd(seed), rnd(seed), rnd(seed)}, aux(b.n_aux), aL, aR, aO;
      const Sc x = rep == 2 ? v[1] : rnd(seed);  // (x = v_1: the inverse of zero)
      circuit::hint_eval_x(P, v.data(), nullptr, x, aux.data());
      uint32_t fail = 1;
      circuit::eval(P, C.n_p, v.data(), aux.data(), x, aL, aR, aO, &fail);
      expect(fail == 0, "no assert, none fails");
      expect(hsc::is_zero(aux[0]), "a late hint that feeds no side stays 0");
      for (uint32_t g = 0; g < n; ++g) {
        const uint32_t kind = g == 0 ? 0 : g % 5;
        const Sc r = aR[g];
        if (kind == 0) {
          const Sc w = hsc::sub(x, v[1]);
          expect(eq(hsc::mul(r, w), hsc::is_zero(w) ? hsc::zero() : hsc::one()), "INV over x");
        } else if (kind == 1 || kind == 2) {
          const uint64_t bit = (aL[g - 1].v[0] >> 7) & 1;
          expect(eq(r, hsc::from_u64(kind == 1 ? bit : 1 - bit)), "BIT / NOT_BIT over a wire");
        } else if (kind == 3) {
          expect(eq(r, hsc::from_u64(hsc::is_zero(aL[g - 1]) ? 1 : 0)), "IS_ZERO over a wire");
        } else {
          expect(eq(hsc::mul(r, aO[g - 1]), hsc::is_zero(aO[g - 1]) ? hsc::zero() : hsc::one()), "INV over o_{g-1}");
        }
        if (g % 7 == 6) expect(eq(aL[g], aR[g - 1]), "an aux index feeding two sides");
        expect(eq(aO[g], hsc::mul(aL[g], aR[g])), "o = l r");
      }
      for (uint32_t g = n; g < C.n_p; ++g) expect(hsc::is_zero(aL[g]) && hsc::is_zero(aR[g]) && hsc::is_zero(aO[g]), "padding");
    }
    // refusals: the hint of the last gate reads a wire of its own gate / an id past the last wire
    Builder own = chain(n);
    own.h.var.back() = circuit::var_wire(own.m_in, n - 1, 0);
    if (n > 1 && (n - 1) % 5 != 0) {
      circuit::Desc d2 = own.desc();
      circuit::HintDesc h2 = own.hints();
      perm::Circuit C2;
      expect(circuit::compile(d2, C2, err, &h2, true) == circuit::ERR_ARG && !C2.program, "own gate's wire refused");
      own.h.var.back() = circuit::var_wire(own.m_in, n, 0);
      h2 = own.hints();
      expect(circuit::compile(d2, C2, err, &h2, true) == circuit::ERR_ARG && !C2.program, "id past the last wire refused");
    }
  }
  // a program without late hints: hint_eval_x is hint_eval
  {
    Builder b;
    const Sc one = hsc::one();
    for (uint32_t g = 0; g < 4; ++g) {
      const uint32_t t = b.hint(g % 2 ? (uint32_t)circuit::kHintInv : circuit::kHintBit | (3u + g) << 8);
      b.h.term(circuit::var_v(g % 3), one);
      b.h.end();
      b.side_aux.insert(b.side_aux.end(), {circuit::SIDE_LC, t});
      b.d.term(circuit::var_v(0), one);
      b.d.end();
      b.d.end();
      ++b.n;
    }
    circuit::Desc d = b.desc();
    circuit::HintDesc h = b.hints();
    perm::Circuit C;
    std::string err;
    expect(circuit::compile(d, C, err, &h, true) == circuit::OK && !circuit::has_late_hints(*C.program), "early program");
    perm::Circuit C0;
    expect(circuit::compile(d, C0, err, &h, false) == circuit::OK && C0.program->dev == C.program->dev &&
               C0.program->hints->dev == C.program->hints->dev,
           "the same device images as the old entry point's");
    std::vector<Sc> v = {rnd(seed), rnd(seed), rnd(seed)}, a(4), a2(4);
    circuit::hint_eval(*C.program, v.data(), nullptr, a.data());
    circuit::hint_eval_x(*C.program, v.data(), nullptr, rnd(seed), a2.data());
    for (int i = 0; i < 4; ++i) expect(eq(a[i], a2[i]), "hint_eval_x == hint_eval");
  }
  printf("mismatches: %d\n", bad);
  return bad != 0;
}
