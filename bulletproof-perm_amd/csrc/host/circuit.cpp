// Caller-defined circuits -- see circuit.h.  The checker this must agree with
// is tests/circuit_ref.py (compile_program / eval_program / circuit_digest),
// with public inputs tests/circuit_pub_ref.py.
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

// the flagged variable id of a term for the device images: | kTermOne for the
// coefficient 1, | kTermNeg for -1 (no multiply)
uint32_t dev_term(uint32_t var, const Sc& a) {
  const Sc one = hsc::one(), neg1 = hsc::neg(hsc::one());
  return var | (a == one ? kTermOne : a == neg1 ? kTermNeg : 0u);
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
  if (h.lc_off[0] != 0) return fail(ERR_ARG, "lc_off[0] is not 0");
  for (uint32_t t = 0; t < n_aux; ++t)
    if (h.lc_off[t + 1] < h.lc_off[t]) return fail(ERR_ARG, "lc_off decreases at " + std::to_string(t + 1));
  const size_t T = h.lc_off[n_aux];
  if (T && (!h.lc_var || !h.lc_coef)) return fail(ERR_ARG, "null lc_var or lc_coef");
  auto H = std::make_shared<Hints>();
  H->op.assign(h.op, h.op + n_aux);
  H->lc_off.assign(h.lc_off, h.lc_off + n_aux + 1);
  H->lc_var.assign(h.lc_var, h.lc_var + T);
  H->lc_coef.resize(T);
  const uint32_t x_id = 1 + m_in, wbase = 2 + m_in + n_pub, nvar = wbase + 3 * n;
  if (wire_hints) H->late.assign(n_aux, 0);
  for (uint32_t t = 0; t < n_aux; ++t) {
    const std::string where = "hint " + std::to_string(t);
    const uint32_t op = h.op[t] & 0xFFu, arg = h.op[t] >> 8;
    if (op >= kHintOps) return fail(ERR_ARG, where + ": unknown op");
    if (arg && op != kHintBit && op != kHintNotBit) return fail(ERR_ARG, where + ": an arg on an op that takes none");
    if (arg > kHintMaxBit) return fail(ERR_ARG, where + ": bit index above 252");
    for (size_t e = h.lc_off[t]; e < h.lc_off[t + 1]; ++e) {
      const uint32_t var = h.lc_var[e];
      if (wire_hints) {
        if (var >= nvar) return fail(ERR_ARG, where + ": variable id beyond the last wire");
        if (var == x_id || var >= wbase) H->late[t] = 1;
      } else {
        if (var >= wbase) return fail(ERR_ARG, where + ": variable id out of range, or a wire");
        if (var == x_id) return fail(ERR_ARG, where + ": reads x (aux exists before x does)");
      }
      if (e > h.lc_off[t] && var <= h.lc_var[e - 1]) return fail(ERR_ARG, where + ": ids not strictly increasing");
      if (!hsc::from_canonical(H->lc_coef[e], h.lc_coef + 32 * e))
        return fail(ERR_NONCANONICAL, where + ": coefficient not below l");
      if (hsc::is_zero(H->lc_coef[e])) return fail(ERR_ARG, where + ": zero coefficient");
    }
  }
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
  std::vector<uint32_t>& dev = H->dev;
  for (uint32_t t : order) {
    const uint32_t rec[4] = {t, is_late(t) ? (uint32_t)kHintValue : H->op[t], is_late(t) ? 0u : H->lc_off[t],
                             is_late(t) ? 0u : H->lc_off[t + 1]};
    dev.insert(dev.end(), rec, rec + 4);
  }
  H->dev_vars = (uint32_t)dev.size();
  for (size_t e = 0; e < T; ++e) dev.push_back(dev_term(H->lc_var[e], H->lc_coef[e]));
  dev.resize((dev.size() + 7) & ~(size_t)7, 0);
  H->dev_coefs = (uint32_t)dev.size();
  for (size_t e = 0; e < T; ++e) {
    uint32_t w[8];
    const Sc cR = hsc::to_mont(H->lc_coef[e]);
    memcpy(w, cR.v, 32);
    dev.insert(dev.end(), w, w + 8);
  }
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
  if (d.lc_off[0] != 0) return fail(ERR_ARG, "lc_off[0] is not 0");
  for (size_t i = 0; i < nlc; ++i)
    if (d.lc_off[i + 1] < d.lc_off[i]) return fail(ERR_ARG, "lc_off decreases at " + std::to_string(i + 1));
  const size_t T = d.lc_off[nlc];
  if (T && (!d.lc_var || !d.lc_coef)) return fail(ERR_ARG, "null lc_var or lc_coef");
  const uint32_t wbase = 2 + m_in + d.n_pub, nvar = wbase + 3 * n;  // (the first wire id)
  auto P = std::make_shared<Program>();
  P->m_in = m_in, P->n = n, P->n_aux = d.n_aux, P->A = A, P->n_pub = d.n_pub;
  P->lc_coef.resize(T);
  uint32_t defined = 0;
  std::vector<uint32_t> level(n, 0);
  for (size_t i = 0; i < nlc; ++i) {
    const bool side = i < 2 * (size_t)n;
    const uint32_t g = (uint32_t)(i / 2);
    const std::string where = side ? "gate " + std::to_string(g) + (i & 1 ? " right" : " left")
                                   : "assert " + std::to_string(i - 2 * (size_t)n);
    if (side) {
      const uint32_t a = d.side_aux[i];
      if (a != SIDE_LC) {
        if (a >= d.n_aux) return fail(ERR_ARG, where + ": aux index out of range");
        if (d.lc_off[i + 1] != d.lc_off[i]) return fail(ERR_ARG, where + ": a free side with a combination");
      } else {
        ++defined;
      }
    }
    for (size_t t = d.lc_off[i]; t < d.lc_off[i + 1]; ++t) {
      const uint32_t var = d.lc_var[t];
      if (var >= nvar) return fail(ERR_ARG, where + ": variable id out of range");
      if (t > d.lc_off[i] && var <= d.lc_var[t - 1]) return fail(ERR_ARG, where + ": ids not strictly increasing");
      if (var >= wbase && side) {
        const uint32_t h = (var - wbase) / 3;
        if (h >= g) return fail(ERR_ARG, where + ": reads a wire of gate " + std::to_string(h));
        level[g] = std::max(level[g], level[h] + 1);
      }
      if (!hsc::from_canonical(P->lc_coef[t], d.lc_coef + 32 * t))
        return fail(ERR_NONCANONICAL, where + ": coefficient not below l");
      if (hsc::is_zero(P->lc_coef[t])) return fail(ERR_ARG, where + ": zero coefficient");
    }
  }
  if (hints) {
    const int rc = compile_hints(*hints, m_in, d.n_pub, n, d.n_aux, wire_hints, P->hints, err);
    if (rc != OK) return rc;
  }
  if (has_late_hints(*P)) {
    // a late hint's wires come from gates before every side it feeds, and the
    // levels count them: again over the gates in order, definitions and late hints
    const Hints& H = *P->hints;
    std::fill(level.begin(), level.end(), 0);
    for (uint32_t g = 0; g < n; ++g)
      for (uint32_t s = 0; s < 2; ++s) {
        const size_t i = 2 * (size_t)g + s;
        const uint32_t a = d.side_aux[i];
        if (a != SIDE_LC && !H.late[a]) continue;
        const uint32_t* var = a == SIDE_LC ? d.lc_var : H.lc_var.data();
        const size_t b = a == SIDE_LC ? d.lc_off[i] : H.lc_off[a], e = a == SIDE_LC ? d.lc_off[i + 1] : H.lc_off[a + 1];
        for (size_t t = b; t < e; ++t) {
          if (var[t] < wbase) continue;
          const uint32_t h = (var[t] - wbase) / 3;
          if (h >= g)
            return fail(ERR_ARG, "gate " + std::to_string(g) + (s ? " right" : " left") + ": its late hint " +
                                     std::to_string(a) + " reads a wire of gate " + std::to_string(h));
          level[g] = std::max(level[g], level[h] + 1);
        }
      }
  }
  C = perm::Circuit();
  C.k = 0;  // (no cards: nothing downstream of the witness reads k)
  C.n = n;
  C.n_p = 4;
  while (C.n_p < n) C.n_p *= 2;
  while ((1u << C.lg) < C.n_p) ++C.lg;
  C.Q = defined + A + 1;
  C.m = m_in + 1;
  C.nv = m_in;
  C.n_pub = d.n_pub;
  C.tiled = (d.flags & kTiled) != 0;
  if (!d.flags && !lds_fits(C.Q, C.n_p, n))
    return fail(ERR_LEN, "Q = " + std::to_string(C.Q) + ", n = " + std::to_string(n) +
                             " beyond the one-workgroup kernels' LDS (BPP_CIRCUIT_LARGE lifts this)");
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
  // late hints: a record per side, and their terms behind the description's T
  std::vector<uint32_t> late_var;
  std::vector<Sc> late_coef;
  if (has_late_hints(*P)) {
    const Hints& H = *P->hints;
    std::vector<uint32_t> at(d.n_aux, 0xFFFFFFFFu);  // where hint a's terms begin (one copy however many sides it feeds)
    P->dev_late = (uint32_t)dev.size();
    for (size_t i = 0; i < 2 * (size_t)n; ++i) {
      const uint32_t a = P->side_aux[i];
      uint32_t rec[3] = {kNoLateHint, 0, 0};
      if (a != SIDE_LC && H.late[a]) {
        if (at[a] == 0xFFFFFFFFu) {
          at[a] = (uint32_t)(T + late_var.size());
          late_var.insert(late_var.end(), H.lc_var.begin() + H.lc_off[a], H.lc_var.begin() + H.lc_off[a + 1]);
          late_coef.insert(late_coef.end(), H.lc_coef.begin() + H.lc_off[a], H.lc_coef.begin() + H.lc_off[a + 1]);
        }
        rec[0] = H.op[a], rec[1] = at[a], rec[2] = at[a] + (H.lc_off[a + 1] - H.lc_off[a]);
      }
      dev.insert(dev.end(), rec, rec + 3);
    }
  }
  P->dev_vars = (uint32_t)dev.size();
  for (size_t t = 0; t < T; ++t) dev.push_back(dev_term(P->lc_var[t], P->lc_coef[t]));
  for (size_t t = 0; t < late_var.size(); ++t) dev.push_back(dev_term(late_var[t], late_coef[t]));
  dev.resize((dev.size() + 7) & ~(size_t)7, 0);
  P->dev_coefs = (uint32_t)dev.size();
  for (size_t t = 0; t < T + late_var.size(); ++t) {
    uint32_t w[8];
    const Sc cR = hsc::to_mont(t < T ? P->lc_coef[t] : late_coef[t - T]);
    memcpy(w, cR.v, 32);
    dev.insert(dev.end(), w, w + 8);
  }
  C.program = P;
  return OK;
}

void eval(const Program& P, uint32_t n_p, const Sc* v, const Sc* aux, const Sc& x, std::vector<Sc>& aL,
          std::vector<Sc>& aR, std::vector<Sc>& aO, uint32_t* bad_assert, const Sc* pub) {
  const uint32_t m_in = P.m_in, n = P.n, wbase = 2 + m_in + P.n_pub;
  aL.assign(n_p, hsc::zero());
  aR.assign(n_p, hsc::zero());
  aO.assign(n_p, hsc::zero());
  std::vector<Sc>* const Wire[3] = {&aL, &aR, &aO};
  auto lc = [&](size_t i) {
    Sc acc = hsc::zero();
    for (size_t t = P.lc_off[i]; t < P.lc_off[i + 1]; ++t) {
      const uint32_t var = P.lc_var[t];
      const Sc val = var == 0           ? hsc::one()
                     : var <= m_in      ? v[var - 1]
                     : var == 1 + m_in  ? x
                     : var < wbase      ? pub[var - 2 - m_in]
                                        : (*Wire[(var - wbase) % 3])[(var - wbase) / 3];
      acc = hsc::add(acc, hsc::mul(P.lc_coef[t], val));
    }
    return acc;
  };
  for (uint32_t g = 0; g < n; ++g) {  // (a definition reads gates h < g only)
    for (uint32_t s = 0; s < 2; ++s) {
      const uint32_t a = P.side_aux[2 * g + s];
      (*Wire[s])[g] = a == SIDE_LC ? lc(2 * (size_t)g + s) : aux[a];
    }
    aO[g] = hsc::mul(aL[g], aR[g]);
  }
  *bad_assert = 0;
  for (uint32_t a = 0; a < P.A; ++a)
    if (!hsc::is_zero(lc(2 * (size_t)n + a))) {
      *bad_assert = a + 1;
      break;
    }
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

}  // namespace

void hint_eval(const Program& P, const Sc* v, const Sc* pub, Sc* aux) {
  const Hints& H = *P.hints;
  for (uint32_t t = 0; t < P.n_aux; ++t) {
    Sc w = hsc::zero();
    for (size_t e = H.lc_off[t]; e < H.lc_off[t + 1]; ++e) {
      const uint32_t var = H.lc_var[e];
      const Sc val = var == 0 ? hsc::one() : var <= P.m_in ? v[var - 1] : pub[var - 2 - P.m_in];
      w = hsc::add(w, hsc::mul(H.lc_coef[e], val));
    }
    aux[t] = hint_op(H.op[t], w);
    w = hsc::zero();
  }
}

void hint_eval_x(const Program& P, const Sc* v, const Sc* pub, const Sc& x, Sc* aux) {
  const Hints& H = *P.hints;
  const uint32_t m_in = P.m_in, n = P.n, wbase = 2 + m_in + P.n_pub;
  std::vector<Sc> wires(3 * (size_t)n, hsc::zero());  // l_h, r_h, o_h at 3h + {0, 1, 2}
  auto lc = [&](const std::vector<uint32_t>& off, const std::vector<uint32_t>& vars, const std::vector<Sc>& coef,
                size_t i) {
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
  };
  auto late = [&](uint32_t t) { return !H.late.empty() && H.late[t]; };
  for (uint32_t t = 0; t < P.n_aux; ++t)
    aux[t] = late(t) ? hsc::zero() : hint_op(H.op[t], lc(H.lc_off, H.lc_var, H.lc_coef, t));
  if (H.n_late)
    for (uint32_t g = 0; g < n; ++g) {
      for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t a = P.side_aux[2 * g + s];
        if (a != SIDE_LC && late(a)) aux[a] = hint_op(H.op[a], lc(H.lc_off, H.lc_var, H.lc_coef, a));
        wires[3 * (size_t)g + s] = a == SIDE_LC ? lc(P.lc_off, P.lc_var, P.lc_coef, 2 * (size_t)g + s) : aux[a];
      }
      wires[3 * (size_t)g + 2] = hsc::mul(wires[3 * (size_t)g], wires[3 * (size_t)g + 1]);
    }
  std::fill(wires.begin(), wires.end(), hsc::zero());
}

}  // namespace circuit
