// What circuit::compile builds, pinned (tests/test_circuit_images.py; ASan +
// UBSan): a fixed list of descriptions is compiled with csrc/host/circuit.cpp
// and, for each, SHAKE256 digests are printed of the program's device image
// and its table offsets, the hints' device image, the level schedule, the
// entries of W_L, W_R, W_O, W_V and W_U, the constant vector c, the circuit's
// shape and the program digest -- one line "name key hex" each.  The expected
// lines are tests/golden/circuit_images.json; the witness kernels read nothing
// of a circuit but these images, so equal images and equal kernels are equal
// witnesses.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host/circuit.h"

using hsc::Sc;

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
  uint32_t m_in = 3, n = 0, n_aux = 0, A = 0, n_pub = 0, flags = 0;
  std::vector<uint32_t> side_aux, op;
  Lcs d, h;
  uint32_t hint(uint32_t word) {
    op.push_back(word);
    return n_aux++;
  }
  circuit::Desc desc() const {
    circuit::Desc r = {m_in, n, n_aux, A, side_aux.data(), d.off.data(), d.var.data(), (const uint8_t*)d.coef.data()};
    r.n_pub = n_pub;
    r.flags = flags;
    return r;
  }
  circuit::HintDesc hints() const { return {op.data(), h.off.data(), h.var.data(), (const uint8_t*)h.coef.data()}; }
};

// The late-hint chain of circuit_wire_hints_check.cpp -- gate g: left = v_{g mod
// 3} + (g + 1) [+ o_{g-1}], right = a late hint cycling through the ops; every
// seventh gate's left side takes the previous gate's aux value (an index feeding
// two sides), hint 0 feeds none.  early: the hints' x and wire terms left out
// (what the entry point without wire hints takes).
static Builder chain(uint32_t n, bool early) {
  Builder b;
  const Sc one = hsc::one(), neg1 = hsc::neg(one);
  const uint32_t x = circuit::var_x(b.m_in);
  auto w = [&](uint32_t g, uint32_t s) { return circuit::var_wire(b.m_in, g, s); };
  auto hterm = [&](uint32_t var, const Sc& c) {
    if (!early || var < x) b.h.term(var, c);
  };
  b.hint(circuit::kHintInv);  // reads x, feeds no side
  hterm(x, one);
  b.h.end();
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t kind = g % 5;
    uint32_t t;
    if (g == 0 || kind == 0) {  // INV(x - v_1)
      t = b.hint(circuit::kHintInv);
      hterm(circuit::var_v(1), neg1);
      hterm(x, one);
    } else if (kind == 1 || kind == 2) {  // BIT / NOT_BIT 7 of l_{g-1}
      t = b.hint((kind == 1 ? circuit::kHintBit : circuit::kHintNotBit) | 7u << 8);
      hterm(w(g - 1, 0), one);
    } else if (kind == 3) {  // IS_ZERO(l_{g-1})
      t = b.hint(circuit::kHintIsZero);
      hterm(w(g - 1, 0), one);
    } else {  // INV(o_{g-1})
      t = b.hint(circuit::kHintInv);
      hterm(w(g - 1, 2), one);
    }
    b.h.end();
    const bool twice = g % 7 == 6;
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

// n gates, every side defined: l_g = (g + 2) v_{g mod m_in} - o_{g-1} + u_{g mod
// n_pub}, r_g = x + 5 l_{g-1} - 1; asserts over the last gate's wires, a v and a u
static Builder products(uint32_t n, uint32_t n_pub, uint32_t A) {
  Builder b;
  b.n_pub = n_pub;
  const Sc one = hsc::one(), neg1 = hsc::neg(one);
  auto w = [&](uint32_t g, uint32_t s) { return circuit::var_wire(b.m_in, g, s, n_pub); };
  for (uint32_t g = 0; g < n; ++g) {
    b.side_aux.insert(b.side_aux.end(), {circuit::SIDE_LC, circuit::SIDE_LC});
    b.d.term(circuit::var_v(g % b.m_in), hsc::from_u64(g + 2));
    if (n_pub) b.d.term(circuit::var_pub(b.m_in, g % n_pub), one);
    if (g) b.d.term(w(g - 1, 2), neg1);
    b.d.end();
    b.d.term(circuit::var_one(), neg1);
    b.d.term(circuit::var_x(b.m_in), one);
    if (g) b.d.term(w(g - 1, 0), hsc::from_u64(5));
    b.d.end();
    ++b.n;
  }
  for (uint32_t a = 0; a < A; ++a) {
    b.d.term(circuit::var_one(), hsc::from_u64(7 + a));
    b.d.term(circuit::var_v(a % b.m_in), neg1);
    if (n_pub) b.d.term(circuit::var_pub(b.m_in, (a + 1) % n_pub), hsc::from_u64(3));
    b.d.term(w(n - 1, a % 3), one);
    b.d.end();
    ++b.A;
  }
  return b;
}

// an early hint of every op over {1, v_j, u_i}, each feeding a right side whose gate's left side is defined
static Builder early_every_op() {
  Builder b;
  b.n_pub = 2;
  const Sc one = hsc::one(), neg1 = hsc::neg(one);
  const uint32_t ops[6] = {circuit::kHintValue,          circuit::kHintBit | 5u << 8, circuit::kHintNotBit | 252u << 8,
                           circuit::kHintInv,            circuit::kHintIsZero,        circuit::kHintBit};
  for (uint32_t g = 0; g < 6; ++g) {
    const uint32_t t = b.hint(ops[g]);
    if (g != 4) b.h.term(circuit::var_one(), hsc::from_u64(9 + g));
    b.h.term(circuit::var_v(g % b.m_in), g % 2 ? neg1 : one);
    if (g >= 2) b.h.term(circuit::var_pub(b.m_in, g % 2), hsc::from_u64(1000 + g));
    b.h.end();
    b.side_aux.insert(b.side_aux.end(), {circuit::SIDE_LC, t});
    b.d.term(circuit::var_v(g % b.m_in), one);
    if (g) b.d.term(circuit::var_wire(b.m_in, g - 1, 1, b.n_pub), neg1);
    b.d.end();
    b.d.end();
    ++b.n;
  }
  b.d.term(circuit::var_pub(b.m_in, 1), neg1);
  b.d.term(circuit::var_wire(b.m_in, 5, 2, b.n_pub), one);
  b.d.end();
  ++b.A;
  return b;
}

// three gates, one term a side, a public input: the smallest with an entry in
// every matrix (W_O and W_L through gate 1's sides, W_R through gate 2's left)
static Builder three_gates() {
  Builder b;
  b.m_in = 1;
  b.n_pub = 1;
  auto w = [&](uint32_t g, uint32_t s) { return circuit::var_wire(b.m_in, g, s, b.n_pub); };
  const uint32_t vars[6] = {circuit::var_v(0), circuit::var_pub(b.m_in, 0), w(0, 2), w(0, 0), w(1, 1),
                            circuit::var_x(b.m_in)};
  for (uint32_t i = 0; i < 6; ++i) {
    b.side_aux.push_back(circuit::SIDE_LC);
    b.d.term(vars[i], hsc::from_u64(2 + i));
    b.d.end();
  }
  b.n = 3;
  return b;
}

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

struct Hash {
  merlin::Shake256 sh;
  void u32(const std::vector<uint32_t>& v) {
    const uint64_t n = v.size();
    sh.update((const uint8_t*)&n, 8);
    if (n) sh.update((const uint8_t*)v.data(), 4 * v.size());
  }
  void u32(std::initializer_list<uint32_t> v) { u32(std::vector<uint32_t>(v)); }
  void sc(const Sc& s) { sh.update((const uint8_t*)s.v, 32); }
  std::string done() {
    uint8_t out[32];
    sh.read(out, 32);
    return hex(out, 32);
  }
};

static int emit(const char* name, const Builder& b, bool with_hints, bool wire_hints) {
  const circuit::Desc d = b.desc();
  const circuit::HintDesc h = b.hints();
  perm::Circuit C;
  std::string err;
  const int rc = circuit::compile(d, C, err, with_hints ? &h : nullptr, wire_hints);
  if (rc != circuit::OK) {
    printf("%s compile %d %s\n", name, rc, err.c_str());
    return 1;
  }
  const circuit::Program& P = *C.program;
  auto line = [&](const char* key, const std::string& v) { printf("%s %s %s\n", name, key, v.c_str()); };
  {
    Hash x;
    x.u32(P.dev);
    line("program_dev", x.done());
  }
  {
    Hash x;
    x.u32({P.dev_lc_off, P.dev_lc_wire, P.dev_level_off, P.dev_level_gate, P.dev_vars, P.dev_coefs, P.dev_late});
    line("program_dev_offsets", x.done());
  }
  if (P.hints) {
    Hash x;
    x.u32(P.hints->dev);
    x.u32({P.hints->dev_vars, P.hints->dev_coefs, P.hints->n_late});
    line("hints_dev", x.done());
  } else {
    line("hints_dev", "none");
  }
  {
    Hash x;
    x.u32(P.level_off);
    x.u32(P.level_gate);
    line("levels", x.done());
  }
  const std::vector<perm::Entry>* const W[5] = {&C.WL, &C.WR, &C.WO, &C.WV, &C.WU};
  const char* const Wn[5] = {"WL", "WR", "WO", "WV", "WU"};
  for (int i = 0; i < 5; ++i) {
    Hash x;
    x.u32({(uint32_t)W[i]->size()});
    for (const perm::Entry& e : *W[i]) {
      x.u32({e.q, e.col});
      x.sc(e.val);
      x.sc(e.valR);
    }
    line(Wn[i], x.done());
  }
  {
    Hash x;
    x.u32({(uint32_t)C.c.size()});
    for (const Sc& s : C.c) x.sc(s);
    line("c", x.done());
  }
  {
    Hash x;
    x.u32({C.k, C.n, C.n_p, C.lg, C.Q, C.m, C.nv, C.n_pub, (uint32_t)C.tiled, P.m_in, P.n, P.n_aux, P.A, P.n_pub});
    line("shape", x.done());
  }
  line("digest", hex(P.digest, 32));
  return memcmp(P.digest, C.program_digest, 32) != 0;
}

int main() {
  int bad = 0;
  bad += emit("no_aux", products(5, 0, 2), false, false);
  bad += emit("public_inputs", products(6, 2, 3), false, false);
  bad += emit("early_hint_of_every_op", early_every_op(), true, false);
  bad += emit("early_hint_of_every_op_wire_entry", early_every_op(), true, true);
  for (uint32_t n : {7u, 40u}) {
    const std::string s = std::to_string(n);
    bad += emit(("late_chain_" + s).c_str(), chain(n, false), true, true);
    bad += emit(("late_chain_" + s + "_unhinted").c_str(), chain(n, false), false, false);
    bad += emit(("late_chain_" + s + "_early_old_entry").c_str(), chain(n, true), true, false);
  }
  {
    Builder b = products(300, 1, 2);
    b.flags = circuit::kLarge | circuit::kTiled;
    bad += emit("large_tiled", b, false, false);
  }
  bad += emit("three_gates", three_gates(), false, false);
  printf("failures: %d\n", bad);
  return bad != 0;
}
