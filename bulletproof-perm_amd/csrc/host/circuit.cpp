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

int compile(const Desc& d, perm::Circuit& C, std::string& err) {
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
  P->dev_vars = (uint32_t)dev.size();
  const Sc neg1 = hsc::neg(hsc::one());
  for (size_t t = 0; t < T; ++t) {
    const Sc& a = P->lc_coef[t];
    const Sc one = hsc::one();
    dev.push_back(P->lc_var[t] | (!memcmp(&a, &one, sizeof(Sc))    ? kTermOne
                                  : !memcmp(&a, &neg1, sizeof(Sc)) ? kTermNeg
                                                                   : 0u));
  }
  dev.resize((dev.size() + 7) & ~(size_t)7, 0);
  P->dev_coefs = (uint32_t)dev.size();
  for (size_t t = 0; t < T; ++t) {
    uint32_t w[8];
    const Sc cR = hsc::to_mont(P->lc_coef[t]);
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

}  // namespace circuit
