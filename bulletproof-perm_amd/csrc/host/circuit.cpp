// Caller-defined circuits -- see circuit.h.  The checkers this must agree with
// are tests/circuit_ref.py (compile_program / eval_program / circuit_digest),
// with public inputs tests/circuit_pub_ref.py, past the one-workgroup bounds
// tests/circuit_large_ref.py, the hints tests/circuit_hints_ref.py and the
// hints over wires and x tests/circuit_wire_hints_ref.py.
#include "circuit.h"

#include <algorithm>

namespace circuit {

using hsc::Sc;

void digest(const Desc& d, uint8_t out[32]) {
  merlin::Shake256 sh;
  if (d.n_pub) {
    sh.update((const uint8_t*)"bpperm-pubcircuit", 17);
    const uint32_t head[5] = {d.m_in, d.n_pub, d.n_gates, d.n_aux, d.n_asserts};  // (little-endian host)
    sh.update((const uint8_t*)head, 20);
  } else {
    sh.update((const uint8_t*)"bpperm-circuit", 14);
    const uint32_t head[4] = {d.m_in, d.n_gates, d.n_aux, d.n_asserts};
    sh.update((const uint8_t*)head, 16);
  }
  const size_t nlc = 2 * (size_t)d.n_gates + d.n_asserts, T = d.lc_off[nlc];
  sh.update((const uint8_t*)d.side_aux, 8 * (size_t)d.n_gates);
  sh.update((const uint8_t*)d.lc_off, 4 * (nlc + 1));
  if (T) sh.update((const uint8_t*)d.lc_var, 4 * T);
  if (T) sh.update(d.lc_coef, 32 * T);
  sh.read(out, 32);
}

namespace {

// The checks of a caller's term table (nlc combinations: lc_off [nlc + 1], lc_var
// [T], lc_coef [T][32]), the description's and the hint program's alike, in the
// order the return codes depend on: lc_off[0] = 0, lc_off monotone, no null
// table; then per combination head(i) and per term id(i, var), ids strictly
// increasing, the coefficient below l (ERR_NONCANONICAL; every other refusal
// ERR_ARG) and nonzero.  head (what combination i hangs on: a side's aux index,
// a hint's op) and id (the ids it may name) are the caller's and return what is
// wrong, or "".  coef receives the T coefficients.
template <class Fail, class Where, class Head, class Id>
int check_terms(const uint32_t* lc_off, const uint32_t* lc_var, const uint8_t* lc_coef, size_t nlc, std::vector<Sc>& coef,
                Fail fail, Where where, Head head, Id id) {
  if (lc_off[0] != 0) return fail(ERR_ARG, "lc_off[0] is not 0");
  for (size_t i = 0; i < nlc; ++i)
    if (lc_off[i + 1] < lc_off[i]) return fail(ERR_ARG, "lc_off decreases at " + std::to_string(i + 1));
  const size_t T = lc_off[nlc];
  if (T && (!lc_var || !lc_coef)) return fail(ERR_ARG, "null lc_var or lc_coef");
  coef.resize(T);
  for (size_t i = 0; i < nlc; ++i) {
    if (const std::string what = head(i); !what.empty()) return fail(ERR_ARG, where(i) + ": " + what);
    for (size_t t = lc_off[i]; t < lc_off[i + 1]; ++t) {
      if (const std::string what = id(i, lc_var[t]); !what.empty()) return fail(ERR_ARG, where(i) + ": " + what);
      if (t > lc_off[i] && lc_var[t] <= lc_var[t - 1]) return fail(ERR_ARG, where(i) + ": ids not strictly increasing");
      if (!hsc::from_canonical(coef[t], lc_coef + 32 * t))
        return fail(ERR_NONCANONICAL, where(i) + ": coefficient not below l");
      if (hsc::is_zero(coef[t])) return fail(ERR_ARG, where(i) + ": zero coefficient");
    }
  }
  return OK;
}

// A term table's tail of a device image: the terms' variable ids, flagged |
// kTermOne for the coefficient 1 and | kTermNeg for -1 (no multiply), zeros to
// a multiple of 8 words, then the Montgomery coefficients [T][8]; the two word
// offsets to o_vars and o_coefs.
void dev_terms(std::vector<uint32_t>& dev, const std::vector<uint32_t>& var, const std::vector<Sc>& coef,
               uint32_t& o_vars, uint32_t& o_coefs) {
  const Sc one = hsc::one(), neg1 = hsc::neg(hsc::one());
  o_vars = (uint32_t)dev.size();
  for (size_t t = 0; t < var.size(); ++t)
    dev.push_back(var[t] | (coef[t] == one ? kTermOne : coef[t] == neg1 ? kTermNeg : 0u));
  dev.resize((dev.size() + 7) & ~(size_t)7, 0);
  o_coefs = (uint32_t)dev.size();
  for (const Sc& c : coef) {
    uint32_t w[8];
    const Sc cR = hsc::to_mont(c);
    memcpy(w, cR.v, 32);
    dev.insert(dev.end(), w, w + 8);
  }
}

// Validates the hint program of a circuit with m_in inputs, n_pub public inputs,
// n gates and n_aux auxiliary values, and builds its device image.  wire_hints:
// ids range over x and the 3n wires too, and a hint that names one is late.
int compile_hints(const HintDesc& h, uint32_t m_in, uint32_t n_pub, uint32_t n, uint32_t n_aux, bool wire_hints,
                  std::shared_ptr<const Hints>& out, std::string& err) {
  auto fail = [&](int rc, std::string what) {
    err = "circuit hints: " + what;
    return rc;
  };
  if (!n_aux) {  // (no aux value, no hint: an empty program)
    out = std::make_shared<Hints>();
    return OK;
  }
  if (!h.op || !h.lc_off) return fail(ERR_ARG, "null op or lc_off");
  const uint32_t x_id = 1 + m_in, wbase = 2 + m_in + n_pub, nvar = wbase + 3 * n;
  auto H = std::make_shared<Hints>();
  const int rc = check_terms(
      h.lc_off, h.lc_var, h.lc_coef, n_aux, H->lc_coef, fail, [](size_t t) { return "hint " + std::to_string(t); },
      [&](size_t t) -> std::string {
        const uint32_t op = h.op[t] & 0xFFu, arg = h.op[t] >> 8;
        if (op >= kHintOps) return "unknown op";
        if (arg && op != kHintBit && op != kHintNotBit) return "an arg on an op that takes none";
        return arg > kHintMaxBit ? "bit index above 252" : "";
      },
      [&](size_t, uint32_t var) -> std::string {
        if (wire_hints) return var >= nvar ? "variable id beyond the last wire" : "";
        if (var >= wbase) return "variable id out of range, or a wire";
        return var == x_id ? "reads x (aux exists before x does)" : "";
      });
  if (rc != OK) return rc;
  const size_t T = h.lc_off[n_aux];
  H->op.assign(h.op, h.op + n_aux);
  H->lc_off.assign(h.lc_off, h.lc_off + n_aux + 1);
  H->lc_var.assign(h.lc_var, h.lc_var + T);
  H->late.assign(n_aux, 0);  // late: the hint names x or a wire (wire_hints only: refused above without)
  for (uint32_t t = 0; t < n_aux; ++t)
    for (size_t e = H->lc_off[t]; e < H->lc_off[t + 1]; ++e)
      if (H->lc_var[e] == x_id || H->lc_var[e] >= wbase) H->late[t] = 1;
  for (uint8_t l : H->late) H->n_late += l;
  if (!H->n_late) H->late.clear();
  // the lane order: by op, INV first, hints of one op in index order (a late
  // hint: the empty VALUE, a 0 that nothing reads)
  auto is_late = [&](uint32_t t) { return !H->late.empty() && H->late[t]; };
  std::vector<uint32_t> order(n_aux);
  for (uint32_t t = 0; t < n_aux; ++t) order[t] = t;
  auto rank = [&](uint32_t t) {
    const uint32_t op = is_late(t) ? (uint32_t)kHintValue : H->op[t] & 0xFFu;
    return op == kHintInv ? 0u : 1u + op;
  };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rank(a) < rank(b); });
  for (uint32_t t : order) {
    const uint32_t rec[4] = {t, is_late(t) ? (uint32_t)kHintValue : H->op[t], is_late(t) ? 0u : H->lc_off[t],
                             is_late(t) ? 0u : H->lc_off[t + 1]};
    H->dev.insert(H->dev.end(), rec, rec + 4);
  }
  dev_terms(H->dev, H->lc_var, H->lc_coef, H->dev_vars, H->dev_coefs);
  out = H;
  return OK;
}

}  // namespace

int compile(const Desc& d, perm::Circuit& C, std::string& err, const HintDesc* hints, bool wire_hints) {
  auto fail = [&](int rc, std::string what) {
    err = "circuit: " + what;
    return rc;
  };
  if (d.flags & ~(kLarge | kTiled)) return fail(ERR_ARG, "unknown flag bits");
  if (!d.m_in || !d.n_gates) return fail(ERR_ARG, "no inputs or no gates");
  if (d.m_in > kMaxInputs || d.n_gates > kMaxGates || d.n_asserts > kMaxAsserts || d.n_aux > kMaxAux)
    return fail(ERR_LEN, "more inputs, gates, asserts or auxiliary values than any circuit that fits");
  if (d.n_pub > kMaxPub) return fail(ERR_LEN, "more than 2^16 public inputs");
  if (!d.side_aux || !d.lc_off) return fail(ERR_ARG, "null side_aux or lc_off");
  const uint32_t m_in = d.m_in, n = d.n_gates, A = d.n_asserts;
  const size_t nlc = 2 * (size_t)n + A;
  const uint32_t wbase = 2 + m_in + d.n_pub, nvar = wbase + 3 * n;  // (the first wire id)
  auto P = std::make_shared<Program>();
  P->m_in = m_in, P->n = n, P->n_aux = d.n_aux, P->A = A, P->n_pub = d.n_pub;
  const auto is_side = [&](size_t i) { return i < 2 * (size_t)n; };
  const auto where = [&](size_t i) {
    return is_side(i) ? "gate " + std::to_string(i / 2) + (i & 1 ? " right" : " left")
                      : "assert " + std::to_string(i - 2 * (size_t)n);
  };
  int rc = check_terms(
      d.lc_off, d.lc_var, d.lc_coef, nlc, P->lc_coef, fail, where,
      [&](size_t i) -> std::string {
        if (!is_side(i) || d.side_aux[i] == SIDE_LC) return "";
        if (d.side_aux[i] >= d.n_aux) return "aux index out of range";
        return d.lc_off[i + 1] != d.lc_off[i] ? "a free side with a combination" : "";
      },
      [&](size_t i, uint32_t var) -> std::string {  // a side of gate g: the wires of gates h < g only
        if (var >= nvar) return "variable id out of range";
        return is_side(i) && var >= wbase + 3 * (uint32_t)(i / 2) ? "reads a wire of gate " + std::to_string((var - wbase) / 3)
                                                                   : "";
      });
  if (rc != OK) return rc;
  if (hints) {
    rc = compile_hints(*hints, m_in, d.n_pub, n, d.n_aux, wire_hints, P->hints, err);
    if (rc != OK) return rc;
  }
  // the gates' levels, the hint program known: a side reads the wires that its
  // definition names or, fed by a late hint, that the hint names -- of gates
  // before its own (a definition's ids were held to that above, a hint's are
  // here, at every side its aux index feeds)
  const Hints* const late = has_late_hints(*P) ? P->hints.get() : nullptr;
  std::vector<uint32_t> level(n, 0);
  for (size_t i = 0; i < 2 * (size_t)n; ++i) {
    const uint32_t g = (uint32_t)(i / 2), a = d.side_aux[i];
    const bool def = a == SIDE_LC;
    if (!def && !(late && late->late[a])) continue;
    const uint32_t *var = def ? d.lc_var : late->lc_var.data(), *off = def ? d.lc_off + i : late->lc_off.data() + a;
    for (size_t t = off[0]; t < off[1]; ++t) {
      if (var[t] < wbase) continue;
      const uint32_t h = (var[t] - wbase) / 3;
      if (h >= g) return fail(ERR_ARG, where(i) + ": its late hint reads a wire of gate " + std::to_string(h));
      level[g] = std::max(level[g], level[h] + 1);
    }
  }
  C = perm::Circuit();
  C.k = 0;  // (no cards: nothing downstream of the witness reads k)
  C.n = n;
  C.n_p = 4;
  while (C.n_p < n) C.n_p *= 2;
  while ((1u << C.lg) < C.n_p) ++C.lg;
  C.Q = (uint32_t)std::count(d.side_aux, d.side_aux + 2 * (size_t)n, SIDE_LC) + A + 1;
  C.m = m_in + 1;
  C.nv = m_in;
  C.n_pub = d.n_pub;
  C.tiled = (d.flags & kTiled) != 0;
  if (!d.flags && !lds_fits(C.Q, C.n_p, n))
    return fail(ERR_LEN, "Q = " + std::to_string(C.Q) + ", n = " + std::to_string(n) +
                             " beyond the one-workgroup kernels' LDS (BPP_CIRCUIT_LARGE lifts this)");
  const size_t T = d.lc_off[nlc];
  P->side_aux.assign(d.side_aux, d.side_aux + 2 * (size_t)n);
  P->lc_off.assign(d.lc_off, d.lc_off + nlc + 1);
  P->lc_var.assign(d.lc_var, d.lc_var + T);
  digest(d, P->digest);
  memcpy(C.program_digest, P->digest, 32);

  // rows: defined left sides, defined right sides, asserts, v_{m_in} = x
  C.c.assign(C.Q, hsc::zero());
  std::vector<perm::Entry>* const Wire[3] = {&C.WL, &C.WR, &C.WO};
  auto emit = [&](uint32_t q, size_t lc, bool is_assert) {
    for (size_t t = P->lc_off[lc]; t < P->lc_off[lc + 1]; ++t) {
      const uint32_t var = P->lc_var[t];
      const Sc a = P->lc_coef[t], na = hsc::neg(a);
      if (var == 0)
        C.c[q] = is_assert ? na : a;
      else if (var <= 1 + m_in)
        C.WV.push_back({q, var - 1, is_assert ? na : a});
      else if (var < wbase)
        C.WU.push_back({q, var - 2 - m_in, is_assert ? na : a});
      else
        Wire[(var - wbase) % 3]->push_back({q, (var - wbase) / 3, is_assert ? a : na});
    }
  };
  uint32_t q = 0;
  for (uint32_t s = 0; s < 2; ++s)
    for (uint32_t g = 0; g < n; ++g)
      if (P->side_aux[2 * g + s] == SIDE_LC) {
        Wire[s]->push_back({q, g, hsc::one()});
        emit(q++, 2 * (size_t)g + s, false);
      }
  for (uint32_t a = 0; a < A; ++a) emit(q++, 2 * (size_t)n + a, true);
  C.WV.push_back({q, m_in, hsc::one()});
  for (auto* W : {&C.WL, &C.WR, &C.WO, &C.WV, &C.WU})
    for (perm::Entry& e : *W) e.valR = hsc::to_mont(e.val);

  // the level schedule and the device image
  const uint32_t nlev = *std::max_element(level.begin(), level.end()) + 1;
  P->level_off.assign(nlev + 1, 0);
  for (uint32_t g = 0; g < n; ++g) ++P->level_off[level[g] + 1];
  for (uint32_t l = 0; l < nlev; ++l) P->level_off[l + 1] += P->level_off[l];
  P->level_gate.resize(n);
  {
    std::vector<uint32_t> at(P->level_off.begin(), P->level_off.end() - 1);
    for (uint32_t g = 0; g < n; ++g) P->level_gate[at[level[g]]++] = g;
  }
  std::vector<uint32_t>& dev = P->dev;
  dev = P->side_aux;
  P->dev_lc_off = (uint32_t)dev.size();
  dev.insert(dev.end(), P->lc_off.begin(), P->lc_off.end());
  P->dev_lc_wire = (uint32_t)dev.size();
  for (size_t i = 0; i < nlc; ++i) {
    uint32_t t = P->lc_off[i];
    while (t < P->lc_off[i + 1] && P->lc_var[t] < wbase) ++t;
    dev.push_back(t);
  }
  P->dev_level_off = (uint32_t)dev.size();
  dev.insert(dev.end(), P->level_off.begin(), P->level_off.end());
  P->dev_level_gate = (uint32_t)dev.size();
  dev.insert(dev.end(), P->level_gate.begin(), P->level_gate.end());
  // the image's term tables: the description's T terms and, with late hints (a
  // record per side), the hints' terms behind them
  std::vector<uint32_t> tvar = P->lc_var;
  std::vector<Sc> tcoef = P->lc_coef;
  if (late) {
    std::vector<uint32_t> at(d.n_aux, 0xFFFFFFFFu);  // where hint a's terms begin (one copy however many sides it feeds)
    P->dev_late = (uint32_t)dev.size();
    for (size_t i = 0; i < 2 * (size_t)n; ++i) {
      const uint32_t a = P->side_aux[i];
      uint32_t rec[3] = {kNoLateHint, 0, 0};
      if (a != SIDE_LC && late->late[a]) {
        if (at[a] == 0xFFFFFFFFu) {
          at[a] = (uint32_t)tvar.size();
          tvar.insert(tvar.end(), late->lc_var.begin() + late->lc_off[a], late->lc_var.begin() + late->lc_off[a + 1]);
          tcoef.insert(tcoef.end(), late->lc_coef.begin() + late->lc_off[a], late->lc_coef.begin() + late->lc_off[a + 1]);
        }
        rec[0] = late->op[a], rec[1] = at[a], rec[2] = at[a] + (late->lc_off[a + 1] - late->lc_off[a]);
      }
      dev.insert(dev.end(), rec, rec + 3);
    }
  }
  dev_terms(dev, tvar, tcoef, P->dev_vars, P->dev_coefs);
  C.program = P;
  return OK;
}

namespace {

// op(w) of a hint's op word
Sc hint_op(uint32_t word, const Sc& w) {
  const uint32_t op = word & 0xFFu, arg = word >> 8;
  const uint64_t bit = (w.v[arg >> 6] >> (arg & 63)) & 1;  // (arg = 0 for the ops without one)
  return op == kHintValue    ? w
         : op == kHintBit    ? hsc::from_u64(bit)
         : op == kHintNotBit ? hsc::from_u64(1 - bit)
         : op == kHintInv    ? hsc::invert(w)  // (w^(l - 2): 0 for w = 0)
                             : hsc::from_u64(hsc::is_zero(w) ? 1 : 0);
}

// One proof's evaluation, what eval, hint_eval and hint_eval_x are made of: the
// value of a combination and the walk over the gates.  v [m_in], pub [n_pub]
// and x are the proof's; wires holds l_h, r_h, o_h at 3h + {0, 1, 2} and is
// scrubbed when the walk goes.
struct Walk {
  const Program& P;
  const Sc *v, *pub;
  const Sc& x;
  std::vector<Sc> wires;
  ~Walk() { std::fill(wires.begin(), wires.end(), hsc::zero()); }

  // combination i of a term table over {1, v_j, x, u_i, wires}
  Sc lc(const std::vector<uint32_t>& off, const std::vector<uint32_t>& vars, const std::vector<Sc>& coef, size_t i) const {
    const uint32_t m_in = P.m_in, wbase = 2 + m_in + P.n_pub;
    Sc acc = hsc::zero();
    for (size_t t = off[i]; t < off[i + 1]; ++t) {
      const uint32_t var = vars[t];
      const Sc val = var == 0          ? hsc::one()
                     : var <= m_in     ? v[var - 1]
                     : var == 1 + m_in ? x
                     : var < wbase     ? pub[var - 2 - m_in]
                                       : wires[var - wbase];
      acc = hsc::add(acc, hsc::mul(coef[t], val));
    }
    return acc;
  }
  bool late(uint32_t t) const { return !P.hints->late.empty() && P.hints->late[t]; }
  Sc hint(uint32_t t) const {
    const Hints& H = *P.hints;
    Sc w = lc(H.lc_off, H.lc_var, H.lc_coef, t);
    const Sc r = hint_op(H.op[t], w);
    w = hsc::zero();
    return r;
  }
  // the early hints' values; a late hint's slot 0
  void early(Sc* aux) const {
    for (uint32_t t = 0; t < P.n_aux; ++t) aux[t] = late(t) ? hsc::zero() : hint(t);
  }
  // The gates in order (a definition reads gates h < g only): a defined side
  // from its combination, a free side from aux.  late_aux (null: aux is
  // complete): a late hint is evaluated into it first, from the wires so far,
  // at every side it feeds.
  void gates(const Sc* aux, Sc* late_aux) {
    wires.assign(3 * (size_t)P.n, hsc::zero());
    for (uint32_t g = 0; g < P.n; ++g) {
      for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t a = P.side_aux[2 * g + s];
        if (a != SIDE_LC && late_aux && late(a)) late_aux[a] = hint(a);
        wires[3 * (size_t)g + s] = a == SIDE_LC ? lc(P.lc_off, P.lc_var, P.lc_coef, 2 * (size_t)g + s) : aux[a];
      }
      wires[3 * (size_t)g + 2] = hsc::mul(wires[3 * (size_t)g], wires[3 * (size_t)g + 1]);
    }
  }
};

}  // namespace

void eval(const Program& P, uint32_t n_p, const Sc* v, const Sc* aux, const Sc& x, std::vector<Sc>& aL,
          std::vector<Sc>& aR, std::vector<Sc>& aO, uint32_t* bad_assert, const Sc* pub) {
  Walk w{P, v, pub, x, {}};
  w.gates(aux, nullptr);
  std::vector<Sc>* const Wire[3] = {&aL, &aR, &aO};
  for (uint32_t s = 0; s < 3; ++s) {
    Wire[s]->assign(n_p, hsc::zero());
    for (uint32_t g = 0; g < P.n; ++g) (*Wire[s])[g] = w.wires[3 * (size_t)g + s];
  }
  *bad_assert = 0;
  for (uint32_t a = 0; a < P.A; ++a)
    if (!hsc::is_zero(w.lc(P.lc_off, P.lc_var, P.lc_coef, 2 * (size_t)P.n + a))) {
      *bad_assert = a + 1;
      break;
    }
}

void hint_eval(const Program& P, const Sc* v, const Sc* pub, Sc* aux) {
  const Sc no_x = hsc::zero();  // (an early hint names neither x nor a wire)
  Walk{P, v, pub, no_x, {}}.early(aux);
}

void hint_eval_x(const Program& P, const Sc* v, const Sc* pub, const Sc& x, Sc* aux) {
  Walk w{P, v, pub, x, {}};
  w.early(aux);
  if (P.hints->n_late) w.gates(aux, aux);
}

}  // namespace circuit
