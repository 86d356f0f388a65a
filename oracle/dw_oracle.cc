/*
 * dw_oracle.cc -- CPU ORACLE: a plain C++ restatement of the reference's Gibbs
 * sweep hot path.
 *
 * TEST INFRASTRUCTURE, NOT PRODUCT (see dw_oracle.h).  Parity status: PINNED
 * against the real reference's outputs and known answers (tests/golden/).
 *
 * Every function cites the reference file:line it restates (paths relative to
 * /root/reference).  Nothing here is copied: the reference's AoS classes are
 * restated over flat std::vectors with the same arithmetic in the same order.
 */
#include "dw_oracle.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

thread_local std::string g_err;

// src/common.h:13-15
constexpr double kLog2 = 0.693147180559945;
constexpr double kMinusLogThreshold = -18.42;
constexpr double kLinearZero = 0.000001;

// src/common.h:35-48 FACTOR_FUNCTION_TYPE
enum Func {
  F_IMPLY_NATURAL = 0, F_OR = 1, F_AND = 2, F_EQUAL = 3, F_ISTRUE = 4,
  F_LINEAR = 7, F_RATIO = 8, F_LOGICAL = 9, F_AND_CATEGORICAL = 12, F_IMPLY_MLN = 13,
};

constexpr uint64_t kInvalid = (uint64_t)-1;

inline bool is_linear_zero(double x) { return x <= kLinearZero && x >= -kLinearZero; }

// src/common.h:118-132 logadd
inline double logadd(double a, double b) {
  if (a < b) std::swap(a, b);
  else if (a <= b && b <= a) return kLog2 + a;
  double nd = b - a;
  if (nd < kMinusLogThreshold) return a;
  return a + log1p(exp(nd));
}

// glibc erand48: X <- (0x5DEECE66D * X + 0xB) mod 2^48; returns X / 2^48.
// call sites src/gibbs_sampler.h:177,204,230
inline double erand48_step(uint16_t x[3]) {
  uint64_t X = (uint64_t)x[0] | ((uint64_t)x[1] << 16) | ((uint64_t)x[2] << 32);
  X = (X * 0x5DEECE66DULL + 0xBULL) & 0xFFFFFFFFFFFFULL;
  x[0] = (uint16_t)X; x[1] = (uint16_t)(X >> 16); x[2] = (uint16_t)(X >> 32);
  return (double)X * (1.0 / 281474976710656.0);
}

// Philox4x32-10 (Salmon et al., SC'11): the device RNG, restated independently.
inline void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c[4]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += W0; k1 += W1;
  }
}
inline void philox_uniforms(uint64_t seed, uint64_t vid, uint64_t sweep, double &A, double &B) {
  uint32_t c[4] = {(uint32_t)vid, (uint32_t)(vid >> 32), (uint32_t)sweep, (uint32_t)(sweep >> 32)};
  philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), c);
  uint64_t a = (uint64_t)c[0] | ((uint64_t)c[1] << 32);
  uint64_t b = (uint64_t)c[2] | ((uint64_t)c[3] << 32);
  A = (double)(a >> 11) * (1.0 / 9007199254740992.0);
  B = (double)(b >> 11) * (1.0 / 9007199254740992.0);
}

struct Var {          // src/variable.h:38-110 (fields that survive construct_index)
  uint8_t is_bool, is_evid;
  uint64_t cardinality, assignment_dense, var_val_base;
  double total_truthiness;
};
struct Value {        // src/variable.h:130-149 VariableToFactor
  uint64_t value; double truthiness; uint64_t index_base, index_len;
};
struct Factor {       // src/factor.h:19-26
  double feature_value; uint64_t weight_id; int func; uint64_t num_vars, vif_base;
};
struct Vif { uint64_t vid, dense_equal_to; };  // src/variable.h:154-167

struct Worker { uint64_t start, end; uint16_t seed[3]; };

}  // namespace

struct orc_sampler {
  orc_opts opts;
  uint64_t V, F, E, W, NVal;
  uint64_t Vg = 0;  // ghost variables (last Vg ids): hold assignments, never sampled
  std::vector<Var> vars;
  std::vector<Value> values;
  std::vector<Factor> factors;
  std::vector<Vif> vifs;
  std::vector<uint64_t> factor_index;
  // InferenceResult (src/inference_result.h:27-43)
  std::vector<uint64_t> tallies, nsamples, a_free, a_evid;
  std::vector<double> weight_values;
  std::vector<uint8_t> weights_isfixed;
  std::vector<Worker> workers;
  // exported columns
  std::vector<uint64_t> c_var_val_base, c_value_sparse, c_index_base, c_index_len, c_assign_dense;
  // schedule-mode accumulators
  std::vector<int64_t> GT;   // G[W], T[W], then H[W] (curvature bounds, schedule mode)
  // the same sums in 128 bits: the device's containers are int64, and an oracle that wrapped with them
  // would agree with a wrapped device bit for bit.  GT holds their image while every sum fits; a sum
  // that leaves int64 makes orc_sched_accumulate / orc_sched_apply fail (range_fault) instead.
  std::vector<__int128> GT128;
  bool range_fault = false;
  uint64_t vid_offset = 0;
  std::vector<uint8_t> fixed_mask;  // schedule mode: variables whose potentials the device sums in fixed point
  bool f32w = false;  // schedule mode: potentials use the weight rounded to f32 (device's sampling copy)

  // ---- src/factor.h:94-100 is_variable_satisfied ----
  inline bool sat(const Vif &vif, uint64_t vid, const uint64_t *assign, uint64_t proposal) const {
    return (vif.vid == vid ? proposal : assign[vif.vid]) == vif.dense_equal_to;
  }

  // ---- src/factor.h:59-86 Factor::potential and :112-299 sign functions ----
  double factor_potential(const Factor &f, const uint64_t *assign, uint64_t vid,
                          uint64_t proposal) const {
    const Vif *v = &vifs[f.vif_base];
    const uint64_t n = f.num_vars;
    double sign;
    switch (f.func) {
      case F_IMPLY_MLN: {                       // :186-206
        bool body = true;
        for (uint64_t i = 0; i + 1 < n; ++i) body &= sat(v[i], vid, assign, proposal);
        if (!body) sign = 1; else sign = sat(v[n - 1], vid, assign, proposal) ? 1 : 0;
        break;
      }
      case F_IMPLY_NATURAL: {                   // :221-241
        bool body = true;
        for (uint64_t i = 0; i + 1 < n; ++i) body &= sat(v[i], vid, assign, proposal);
        if (!body) sign = 0; else sign = sat(v[n - 1], vid, assign, proposal) ? 1 : -1;
        break;
      }
      case F_AND: case F_ISTRUE: {              // :138-146, alias :73
        sign = 1;
        for (uint64_t i = 0; i < n; ++i) if (!sat(v[i], vid, assign, proposal)) { sign = -1; break; }
        break;
      }
      case F_OR: {                              // :166-174
        sign = -1;
        for (uint64_t i = 0; i < n; ++i) if (sat(v[i], vid, assign, proposal)) { sign = 1; break; }
        break;
      }
      case F_EQUAL: {                           // :112-128
        bool first = sat(v[0], vid, assign, proposal);
        sign = 1;
        for (uint64_t i = 0; i < n; ++i) if (sat(v[i], vid, assign, proposal) != first) { sign = -1; break; }
        break;
      }
      case F_AND_CATEGORICAL: {                 // :148-158
        sign = 1;
        for (uint64_t i = 0; i < n; ++i) if (!sat(v[i], vid, assign, proposal)) { sign = 0; break; }
        break;
      }
      case F_LINEAR: {                          // :244-259
        double res = 0.0;
        bool head = sat(v[n - 1], vid, assign, proposal);
        for (uint64_t i = 0; i + 1 < n; ++i) res += ((1 - sat(v[i], vid, assign, proposal)) || head);
        sign = (n == 1) ? double(head) : res;
        break;
      }
      case F_RATIO: {                           // :262-275
        double res = 1.0;
        bool head = sat(v[n - 1], vid, assign, proposal);
        for (uint64_t i = 0; i + 1 < n; ++i) res += ((1 - sat(v[i], vid, assign, proposal)) || head);
        sign = (n == 1) ? log2(res + double(head)) : log2(res);
        break;
      }
      case F_LOGICAL: {                         // :278-296
        double res = 0.0;
        bool head = sat(v[n - 1], vid, assign, proposal);
        for (uint64_t i = 0; i + 1 < n; ++i) res += ((1 - sat(v[i], vid, assign, proposal)) || head);
        sign = (n == 1) ? double(head) : (res > 0.0 ? 1.0 : 0.0);
        break;
      }
      default:                                  // :80-84 (reference aborts)
        throw std::runtime_error("Unsupported FACTOR_FUNCTION_TYPE = " + std::to_string(f.func));
    }
    return sign * f.feature_value;
  }

  // ---- src/factor_graph.h:127-145 FactorGraph::potential ----
  double potential(const Var &var, uint64_t vid, uint64_t proposal, const uint64_t *assign,
                   const double *w) const {
    double pot = 0.0;
    const Value &vv = values[var.var_val_base + (var.is_bool ? 0 : proposal)];
    for (uint64_t i = 0; i < vv.index_len; ++i) {
      const Factor &f = factors[factor_index[vv.index_base + i]];
      const double wv = f32w ? (double)(float)w[f.weight_id] : w[f.weight_id];
      pot += wv * factor_potential(f, assign, vid, proposal);
    }
    return pot;
  }

  // Schedule mode, variables the device sums in fixed point (dwx_graph_get_fixed_point_mask:
  // boolean variables of an all-unary graph): pp - pn = 2^-32 * sum over the row of
  // round(2^32 * clamp(w * (term(1) - term(0)))) -- an integer sum, independent of the order of
  // the records (pot_fix in sampler_amd/csrc/factor_functions.h).
  double fixed_point_pot_diff(const Var &var, uint64_t vid, const uint64_t *assign, const double *w) const {
    long long acc = 0;
    const Value &vv = values[var.var_val_base];
    for (uint64_t i = 0; i < vv.index_len; ++i) {
      const Factor &f = factors[factor_index[vv.index_base + i]];
      const double wv = f32w ? (double)(float)w[f.weight_id] : w[f.weight_id];
      double p = wv * factor_potential(f, assign, vid, 1) - wv * factor_potential(f, assign, vid, 0);
      p = p < -524288.0 ? -524288.0 : (p > 524288.0 ? 524288.0 : p);
      acc += (long long)nearbyint(p * 4294967296.0);
    }
    return (double)acc * (1.0 / 4294967296.0);
  }

  // ---- src/gibbs_sampler.h:192-254 draw_sample, with the uniform r supplied ----
  template <class Rng>
  uint64_t draw_sample(uint64_t vid, const uint64_t *assign, const double *w, Rng &&next_r,
                       std::vector<double> &buf) const {
    const Var &var = vars[vid];
    if (var.is_bool) {                          // :198-215
      const bool fixed = !fixed_mask.empty() && fixed_mask[vid];
      double pp = fixed ? fixed_point_pot_diff(var, vid, assign, w) : potential(var, vid, 1, assign, w);
      double pn = fixed ? 0.0 : potential(var, vid, 0, assign, w);
      double r = next_r();
      return (r * (1.0 + exp(pn - pp)) < 1.0) ? 1 : 0;
    }
    // :217-246
    if (buf.size() < var.cardinality) buf.resize(var.cardinality);
    double sum = -100000.0;
    for (uint64_t i = 0; i < var.cardinality; ++i) {
      buf[i] = potential(var, vid, i, assign, w);
      sum = logadd(sum, buf[i]);
    }
    double r = next_r();
    for (uint64_t i = 0; i < var.cardinality; ++i) {
      r -= exp(buf[i] - sum);
      if (r <= 0) return i;
    }
    // the reference asserts here (:243); rounding can leave r a hair above 0
    return var.cardinality - 1;
  }

  bool has_truthiness(const Var &v) const { return !is_linear_zero(v.total_truthiness); }

  // ---- src/gibbs_sampler.h:171-190 sample_evid ----
  template <class Rng>
  uint64_t sample_evid(uint64_t vid, Rng &&next_r, std::vector<double> &buf) const {
    const Var &var = vars[vid];
    if (!opts.noise_aware && var.is_evid) return var.assignment_dense;
    if (opts.noise_aware && has_truthiness(var)) {
      double r = next_r();
      double sum = 0;
      for (uint64_t i = 0; i < var.cardinality; ++i) {
        sum += values[var.var_val_base + i].truthiness;
        if (sum >= r) return i;
      }
      return 0;
    }
    return draw_sample(vid, a_evid.data(), weight_values.data(), next_r, buf);
  }

  // ---- src/inference_result.h:66-85 update_weight ----
  void update_weight(uint64_t wid, double stepsize, double gradient) {
    double diff = stepsize * gradient;
    double weight = weight_values[wid];
    if (opts.regularization == 1) weight *= (1.0 / (1.0 + opts.reg_param * stepsize));
    else weight += opts.reg_param * (weight < 0);
    weight -= diff;
    weight_values[wid] = weight;
  }

  // ---- src/factor_graph.cc:243-260 sgd_on_factor ----
  template <class Upd>
  void sgd_on_factor(uint64_t fid, double stepsize, uint64_t vid, uint64_t evidence_value, Upd &&upd) {
    const Factor &f = factors[fid];
    if (weights_isfixed[f.weight_id]) return;
    double pot_evid = factor_potential(f, a_evid.data(), vid, evidence_value);
    double pot_free = factor_potential(f, a_free.data(), kInvalid, kInvalid);
    upd(f.weight_id, stepsize, pot_free - pot_evid);
  }

  // ---- src/factor_graph.cc:262-314 sgd_on_variable ----
  template <class Upd>
  void sgd_on_variable(uint64_t vid, double stepsize, Upd &&upd) {
    const Var &var = vars[vid];
    if (var.is_bool) {
      const Value &vv = values[var.var_val_base];
      for (uint64_t j = 0; j < vv.index_len; ++j)
        sgd_on_factor(factor_index[vv.index_base + j], stepsize, vid, var.assignment_dense, upd);
      return;
    }
    uint64_t proposal = a_free[vid];
    for (uint64_t val = 0; val < var.cardinality; ++val) {
      if (!opts.noise_aware && val != var.assignment_dense) continue;
      const Value &ev = values[var.var_val_base + val];
      if (opts.noise_aware && is_linear_zero(ev.truthiness)) continue;
      double truthiness = opts.noise_aware ? ev.truthiness : 1;
      for (uint64_t j = 0; j < ev.index_len; ++j)
        sgd_on_factor(factor_index[ev.index_base + j], stepsize * truthiness, vid, val, upd);
      if (val == proposal) continue;
      const Value &pv = values[var.var_val_base + proposal];
      for (uint64_t j = 0; j < pv.index_len; ++j)
        sgd_on_factor(factor_index[pv.index_base + j], stepsize * truthiness, vid, val, upd);
    }
  }

  // ---- schedule mode only: curvature bound of a variable's SGD updates, per factor ----
  // Restates the device's static table (sampler_amd/csrc/level_build.cc
  // for_each_record_bound): delta of a factor = how far it can move the variable's potential
  // between two of its values -- |sign(hit) - sign(miss)| |f| at arity 1 (the sign functions of
  // src/factor.h:112-299 with one satisfied bit), 2 |f| (arity - 1) beyond; a boolean variable
  // bounds factor r by 1/4 delta_r * (sum of its row's deltas), a categorical one by
  // 1/2 delta_r * (largest sum of deltas of one of its value rows).  Fixed weights: 0.
  static double unary_sign_of(int func, bool sat) {
    switch (func) {
      case F_AND: case F_ISTRUE: case F_OR: case F_IMPLY_NATURAL: return sat ? 1.0 : -1.0;
      case F_EQUAL: return 1.0;
      default: return sat ? 1.0 : 0.0;
    }
  }
  double factor_delta(const Factor &f, const Var &var) const {
    if (weights_isfixed[f.weight_id]) return 0.0;
    if (f.num_vars <= 1) {
      const uint64_t eq = vifs[f.vif_base].dense_equal_to;
      const double hit = unary_sign_of(f.func, !var.is_bool || eq == 1);
      const double miss = unary_sign_of(f.func, var.is_bool && eq == 0);
      return std::fabs(hit - miss) * std::fabs(f.feature_value);
    }
    return 2.0 * std::fabs(f.feature_value) * (double)(f.num_vars - 1);
  }
  template <class Fn>
  void curvature_bounds(uint64_t vid, Fn &&fn) const {
    const Var &var = vars[vid];
    const uint64_t rows = var.is_bool ? 1 : var.cardinality;
    double S = 0.0;
    for (uint64_t d = 0; d < rows; ++d) {
      const Value &vv = values[var.var_val_base + d];
      double sr = 0.0;
      for (uint64_t j = 0; j < vv.index_len; ++j) sr += factor_delta(factors[factor_index[vv.index_base + j]], var);
      S = var.is_bool ? S + sr : std::max(S, sr);
    }
    if (S == 0.0) return;
    const double kappa = var.is_bool ? 0.25 : 0.5;
    for (uint64_t d = 0; d < rows; ++d) {
      const Value &vv = values[var.var_val_base + d];
      for (uint64_t j = 0; j < vv.index_len; ++j) {
        const Factor &f = factors[factor_index[vv.index_base + j]];
        const double dl = factor_delta(f, var);
        if (dl != 0.0) fn(f.weight_id, kappa * dl * S);
      }
    }
  }

  bool sgd_triggers(const Var &var) const {  // src/gibbs_sampler.h:144-146 (negated)
    return opts.learn_non_evidence || ((!opts.noise_aware && var.is_evid) ||
                                       (opts.noise_aware && has_truthiness(var)));
  }

  // ---- src/gibbs_sampler.h:151-169 bookkeeping after an inference draw ----
  void record_sample(uint64_t vid, uint64_t proposal) {
    const Var &var = vars[vid];
    a_evid[vid] = proposal;
    ++nsamples[vid];
    if (!var.is_bool || proposal == 1) ++tallies[var.var_val_base + (var.is_bool ? 0 : proposal)];
  }
};

// ---------------------------------------------------------------------------
// construction: src/binary_format.cc:48-226 conversions + src/factor_graph.cc:90-199
// construct_index + src/inference_result.cc:24-42 init
// ---------------------------------------------------------------------------
extern "C" orc_sampler *orc_create(const orc_graph_desc *d, const orc_opts *opts) {
  try {
    auto *s = new orc_sampler();
    s->opts = *opts;
    s->V = d->num_variables; s->F = d->num_factors; s->E = d->num_edges; s->W = d->num_weights;
    s->Vg = d->num_ghost_variables;
    s->vars.resize(s->V);
    std::vector<std::unordered_map<uint64_t, std::pair<uint64_t, double>>> domain_map(0);
    std::vector<int64_t> dom_of(s->V, -1);
    // load_variables (src/binary_format.cc:64-126)
    for (uint64_t v = 0; v < s->V; ++v) {
      Var &x = s->vars[v];
      if (d->var_dtype[v] > 1) throw std::runtime_error("Only Boolean and Categorical variables are supported");
      x.is_bool = d->var_dtype[v] == 0;
      x.is_evid = d->var_role[v] >= 1;
      x.cardinality = d->var_cardinality[v];
      x.assignment_dense = x.is_evid ? d->var_init_value[v] : 0;
      x.total_truthiness = 0;
      x.var_val_base = kInvalid;
    }
    // load_domains (src/binary_format.cc:192-226)
    domain_map.resize(d->num_domains);
    for (uint64_t b = 0; b < d->num_domains; ++b) {
      uint64_t vid = d->dom_vid[b];
      if (vid >= s->V) throw std::runtime_error("domain block for unknown variable");
      Var &x = s->vars[vid];
      uint64_t lo = d->dom_offset[b], hi = d->dom_offset[b + 1];
      if (x.is_bool) throw std::runtime_error("domain block for boolean variable");
      if (x.cardinality != hi - lo) throw std::runtime_error("domain size != cardinality");
      auto &m = domain_map[b];
      for (uint64_t i = lo; i < hi; ++i) m[d->dom_value[i]] = {i - lo, d->dom_truthiness[i]};
      dom_of[vid] = (int64_t)b;
      if (x.assignment_dense) x.assignment_dense = m.at(x.assignment_dense).first;
    }
    auto domain_index = [&](uint64_t vid, uint64_t v) -> uint64_t {  // src/variable.h:124-126
      return dom_of[vid] >= 0 ? domain_map[dom_of[vid]].at(v).first : v;
    };
    // load_factors (src/binary_format.cc:128-190)
    s->factors.resize(s->F);
    s->vifs.resize(s->E);
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> adj(s->V);  // (value_dense, fid)
    for (uint64_t f = 0; f < s->F; ++f) {
      Factor &x = s->factors[f];
      x.func = d->fac_func[f];
      x.vif_base = d->fac_edge_offset[f];
      x.num_vars = d->fac_edge_offset[f + 1] - d->fac_edge_offset[f];
      x.weight_id = d->fac_weight_id[f];
      x.feature_value = d->fac_feature_value[f];
      if (x.weight_id >= s->W) throw std::runtime_error("factor references unknown weight");
      for (uint64_t e = x.vif_base; e < x.vif_base + x.num_vars; ++e) {
        uint64_t vid = d->edge_vid[e];
        if (vid >= s->V) throw std::runtime_error("factor references unknown variable");
        uint64_t dense = domain_index(vid, d->edge_equal_to[e]);
        s->vifs[e] = {vid, dense};
        adj[vid].push_back({s->vars[vid].is_bool ? 0 : dense, f});
      }
    }
    // construct_index (src/factor_graph.cc:90-199)
    uint64_t nval = 0;
    const uint64_t Vown = s->V - s->Vg;   // ghosts (ids >= Vown) get no rows and no back-refs
    for (uint64_t v = 0; v < Vown; ++v) nval += s->vars[v].is_bool ? 1 : s->vars[v].cardinality;
    s->NVal = nval;
    s->values.assign(nval, Value{kInvalid, 0, kInvalid, 0});
    s->factor_index.reserve(s->E);
    uint64_t vb = 0;
    for (uint64_t v = 0; v < s->V; ++v) {
      Var &x = s->vars[v];
      x.var_val_base = vb;
      if (v >= Vown) { std::vector<std::pair<uint64_t, uint64_t>>().swap(adj[v]); continue; }
      if (x.is_bool) {
        s->values[vb++] = Value{0, 0, 0, 0};
      } else if (dom_of[v] >= 0) {
        uint64_t b = dom_of[v], lo = d->dom_offset[b];
        // value_list[index] = value: with duplicate values in a block the map keeps the
        // LAST index for that value and the earlier slot stays INVALID (:151-160)
        std::vector<uint64_t> vl(x.cardinality, kInvalid);
        std::vector<double> tl(x.cardinality, 0);
        for (auto &it : domain_map[b]) {
          vl.at(it.second.first) = it.first;
          tl.at(it.second.first) = it.second.second;
          x.total_truthiness += it.second.second;
        }
        (void)lo;
        for (uint64_t j = 0; j < x.cardinality; ++j) s->values[vb++] = Value{vl[j], tl[j], 0, 0};
      } else {
        for (uint64_t j = 0; j < x.cardinality; ++j) s->values[vb++] = Value{j, 0, 0, 0};
      }
      auto &a = adj[v];
      std::sort(a.begin(), a.end());
      uint64_t cur_val = kInvalid, last_f = kInvalid;
      for (auto &it : a) {
        if (it.first != cur_val) {
          cur_val = it.first;
          if (cur_val >= x.cardinality) throw std::runtime_error("value_dense >= cardinality");
          s->values[x.var_val_base + cur_val].index_base = s->factor_index.size();
        } else if (it.second == last_f) {
          continue;
        }
        s->factor_index.push_back(it.second);
        ++s->values[x.var_val_base + cur_val].index_len;
        last_f = it.second;
      }
      std::vector<std::pair<uint64_t, uint64_t>>().swap(a);
    }
    // InferenceResult (src/inference_result.cc:24-42)
    s->weight_values.assign(d->w_initial_value, d->w_initial_value + s->W);
    s->weights_isfixed.assign(d->w_is_fixed, d->w_is_fixed + s->W);
    s->a_free.resize(s->V); s->a_evid.resize(s->V);
    for (uint64_t v = 0; v < s->V; ++v)
      s->a_free[v] = s->a_evid[v] = s->vars[v].is_evid ? s->vars[v].assignment_dense : 0;
    s->tallies.assign(nval, 0);
    s->nsamples.assign(s->V, 0);
    s->GT.assign(3 * s->W, 0);
    // exported columns
    s->c_var_val_base.resize(s->V); s->c_assign_dense.resize(s->V);
    for (uint64_t v = 0; v < s->V; ++v) {
      s->c_var_val_base[v] = s->vars[v].var_val_base;
      s->c_assign_dense[v] = s->vars[v].assignment_dense;
    }
    s->c_value_sparse.resize(nval); s->c_index_base.resize(nval); s->c_index_len.resize(nval);
    for (uint64_t i = 0; i < nval; ++i) {
      s->c_value_sparse[i] = s->values[i].value;
      s->c_index_base[i] = s->values[i].index_base;
      s->c_index_len[i] = s->values[i].index_len;
    }
    orc_ref_set_workers(s, 1);
    return s;
  } catch (const std::exception &e) {
    g_err = e.what();
    return nullptr;
  }
}

extern "C" void orc_destroy(orc_sampler *s) { delete s; }
extern "C" const char *orc_last_error(void) { return g_err.c_str(); }
extern "C" uint64_t orc_num_values(const orc_sampler *s) { return s->NVal; }
extern "C" uint64_t orc_num_index_entries(const orc_sampler *s) { return s->factor_index.size(); }
extern "C" double *orc_weights(orc_sampler *s) { return s->weight_values.data(); }
extern "C" uint64_t *orc_assignments(orc_sampler *s, int chain) {
  return chain == 0 ? s->a_free.data() : s->a_evid.data();
}
extern "C" uint64_t *orc_tallies(orc_sampler *s) { return s->tallies.data(); }
extern "C" uint64_t *orc_nsamples(orc_sampler *s) { return s->nsamples.data(); }
extern "C" const uint64_t *orc_var_val_base(const orc_sampler *s) { return s->c_var_val_base.data(); }
extern "C" const uint64_t *orc_value_sparse(const orc_sampler *s) { return s->c_value_sparse.data(); }
extern "C" const uint64_t *orc_value_index_base(const orc_sampler *s) { return s->c_index_base.data(); }
extern "C" const uint64_t *orc_value_index_len(const orc_sampler *s) { return s->c_index_len.data(); }
extern "C" const uint64_t *orc_factor_index(const orc_sampler *s) { return s->factor_index.data(); }
extern "C" const uint64_t *orc_var_assignment_dense(const orc_sampler *s) { return s->c_assign_dense.data(); }
// src/inference_result.cc:107-114
extern "C" void orc_clear_tallies(orc_sampler *s) {
  std::fill(s->tallies.begin(), s->tallies.end(), 0);
  std::fill(s->nsamples.begin(), s->nsamples.end(), 0);
}

// ---------------------------------------------------------------------------
// reference mode
// ---------------------------------------------------------------------------
// src/gibbs_sampler.cc:40-55 : shard ranges and rand()-derived seeds
extern "C" void orc_ref_set_workers(orc_sampler *s, uint32_t n) {
  if (n == 0) n = 1;
  s->workers.resize(n);
  // un-seeded rand() == glibc TYPE_3 additive feedback generator seeded with 1
  char statebuf[128];
  struct random_data rd;
  memset(&rd, 0, sizeof rd);
  memset(statebuf, 0, sizeof statebuf);
  initstate_r(1, statebuf, sizeof statebuf, &rd);
  for (uint32_t i = 0; i < n; ++i) {
    int32_t r[3];
    for (int k = 0; k < 3; ++k) random_r(&rd, &r[k]);
    Worker &w = s->workers[i];
    // g++ evaluates the arguments of set_random_seed(rand(), rand(), rand()) right to
    // left, so the FIRST rand() lands in seed[2] (pinned by the byte-exact goldens:
    // left-to-right gives weight 1.23412 instead of the reference's 0.71363).
    w.seed[0] = (uint16_t)r[2]; w.seed[1] = (uint16_t)r[1]; w.seed[2] = (uint16_t)r[0];
    uint64_t per = s->V / n + 1;
    w.start = per * i;
    w.end = std::min<uint64_t>(per * (i + 1), s->V);
    if (w.start > s->V) w.start = s->V;
  }
}
extern "C" void orc_ref_set_seed(orc_sampler *s, uint32_t w, uint16_t s0, uint16_t s1, uint16_t s2) {
  s->workers[w].seed[0] = s0; s->workers[w].seed[1] = s1; s->workers[w].seed[2] = s2;
}

namespace {
struct RefRng {
  uint16_t *seed;
  double operator()() { return erand48_step(seed); }
};
// src/gibbs_sampler.h:151-169
void ref_sample_one(orc_sampler *s, Worker &w, uint64_t vid, std::vector<double> &buf) {
  const Var &var = s->vars[vid];
  if (!var.is_evid || s->opts.sample_evidence) {
    uint64_t p = s->draw_sample(vid, s->a_evid.data(), s->weight_values.data(), RefRng{w.seed}, buf);
    s->record_sample(vid, p);
  }
}
// src/gibbs_sampler.h:127-149
void ref_sample_sgd_one(orc_sampler *s, Worker &w, uint64_t vid, double stepsize,
                        std::vector<double> &buf) {
  uint64_t p = s->draw_sample(vid, s->a_free.data(), s->weight_values.data(), RefRng{w.seed}, buf);
  s->a_free[vid] = p;
  s->a_evid[vid] = s->sample_evid(vid, RefRng{w.seed}, buf);
  if (!s->sgd_triggers(s->vars[vid])) return;
  s->sgd_on_variable(vid, stepsize,
                     [s](uint64_t wid, double st, double g) { s->update_weight(wid, st, g); });
}
template <class Fn>
void run_workers(orc_sampler *s, int threaded, Fn &&fn) {
  if (threaded && s->workers.size() > 1) {
    std::vector<std::thread> th;
    for (auto &w : s->workers) th.emplace_back([&fn, &w]() { fn(w); });
    for (auto &t : th) t.join();
  } else {
    for (auto &w : s->workers) fn(w);
  }
}
}  // namespace

extern "C" void orc_ref_sample_single_variable(orc_sampler *s, uint32_t w, uint64_t vid) {
  std::vector<double> buf;
  ref_sample_one(s, s->workers[w], vid, buf);
}
extern "C" void orc_ref_sample_sgd_single_variable(orc_sampler *s, uint32_t w, uint64_t vid,
                                                   double stepsize) {
  std::vector<double> buf;
  ref_sample_sgd_one(s, s->workers[w], vid, stepsize, buf);
}
extern "C" void orc_ref_sgd_on_variable(orc_sampler *s, uint64_t vid, double stepsize) {
  s->sgd_on_variable(vid, stepsize,
                     [s](uint64_t wid, double st, double g) { s->update_weight(wid, st, g); });
}
// src/gibbs_sampler.cc:20-25,65-69
extern "C" void orc_ref_sample(orc_sampler *s, int threaded) {
  run_workers(s, threaded, [s](Worker &w) {
    std::vector<double> buf;
    for (uint64_t v = w.start; v < w.end; ++v) ref_sample_one(s, w, v, buf);
  });
}
// src/gibbs_sampler.cc:27-33,71-75
extern "C" void orc_ref_sample_sgd(orc_sampler *s, double stepsize, int threaded) {
  run_workers(s, threaded, [s, stepsize](Worker &w) {
    std::vector<double> buf;
    for (uint64_t v = w.start; v < w.end; ++v) ref_sample_sgd_one(s, w, v, stepsize, buf);
  });
}
// src/dimmwitted.cc:162-207 (n_samplers_ == 1: update_weights only prints norms)
extern "C" void orc_ref_learn(orc_sampler *s, uint64_t n_epoch, double stepsize, double decay,
                              int threaded) {
  double cur = stepsize;
  for (uint64_t e = 0; e < n_epoch; ++e) {
    orc_ref_sample_sgd(s, cur, threaded);
    cur *= decay;
  }
}
// src/dimmwitted.cc:121-160
extern "C" void orc_ref_inference(orc_sampler *s, uint64_t n_epoch, int threaded) {
  orc_clear_tallies(s);
  for (uint64_t e = 0; e < n_epoch; ++e) orc_ref_sample(s, threaded);
}

extern "C" double orc_potential(orc_sampler *s, uint64_t vid, uint64_t proposal, int chain) {
  return s->potential(s->vars[vid], vid, proposal, chain == 0 ? s->a_free.data() : s->a_evid.data(),
                      s->weight_values.data());
}

// truth tables (test/factor_test.cc): evaluate one sign function on explicit
// satisfied-bits by building a throw-away one-factor graph where variable i has
// assignment sat[i] and every predicate is "== 1".
extern "C" double orc_factor_sign(int func, uint64_t arity, const uint8_t *satbits) {
  orc_sampler s;
  s.vifs.resize(arity);
  std::vector<uint64_t> assign(arity);
  for (uint64_t i = 0; i < arity; ++i) { s.vifs[i] = {i, 1}; assign[i] = satbits[i]; }
  Factor f{1.0, 0, func, arity, 0};
  try {
    return s.factor_potential(f, assign.data(), kInvalid, kInvalid);
  } catch (const std::exception &e) {
    g_err = e.what();
    return NAN;
  }
}
extern "C" double orc_logadd(double a, double b) { return logadd(a, b); }
extern "C" double orc_erand48(uint16_t x[3]) { return erand48_step(x); }
// raw block function, for the Random123 known-answer vectors (tests/test_philox_kat.py)
extern "C" void orc_philox4x32_10(const uint32_t key[2], uint32_t ctr[4]) { philox4x32_10(key[0], key[1], ctr); }
extern "C" void orc_philox_uniforms(uint64_t seed, uint64_t vid, uint64_t sweep, double out[2]) {
  philox_uniforms(seed, vid, sweep, out[0], out[1]);
}

// ---------------------------------------------------------------------------
// schedule mode (device semantics)
// ---------------------------------------------------------------------------
namespace {
constexpr double kFixScale = 1073741824.0;  // 2^30
constexpr double kHessScale = 1024.0;       // 2^10 (curvature bounds)
struct OneShot {   // hands out the pre-drawn uniform
  double r;
  double operator()() { return r; }
};
}  // namespace

extern "C" int orc_sched_check_independent(orc_sampler *s, const orc_schedule *sch) {
  std::vector<uint64_t> launch_of(s->V, kInvalid);
  for (uint64_t l = 0; l < sch->n_launches; ++l)
    for (uint64_t i = sch->launch_off[l]; i < sch->launch_off[l + 1]; ++i) launch_of[sch->order[i]] = l;
  // every owned variable must be scheduled; ghosts (the last Vg ids) must not be
  for (uint64_t v = 0; v < s->V; ++v) if ((launch_of[v] == kInvalid) != (v >= s->V - s->Vg)) return 0;
  // no launch holds two different variables of one factor (one pass per factor: a factor may have 65535 positions)
  std::vector<uint64_t> seen(sch->n_launches, kInvalid);   // launch -> the factor's variable met in it
  std::vector<uint64_t> touched;
  for (const Factor &f : s->factors) {
    bool ok = true;
    touched.clear();
    for (uint64_t i = 0; i < f.num_vars && ok; ++i) {
      const uint64_t a = s->vifs[f.vif_base + i].vid, l = launch_of[a];
      if (l == kInvalid) continue;
      if (seen[l] == kInvalid) { seen[l] = a; touched.push_back(l); }
      else ok = seen[l] == a;
    }
    for (uint64_t l : touched) seen[l] = kInvalid;
    if (!ok) return 0;
  }
  return 1;
}

extern "C" void orc_set_var_id_offset(orc_sampler *s, uint64_t off) { s->vid_offset = off; }
extern "C" void orc_set_sampling_weight_f32(orc_sampler *s, int on) { s->f32w = on != 0; }
extern "C" void orc_set_fixed_point_mask(orc_sampler *s, const uint8_t *mask) {
  if (mask) s->fixed_mask.assign(mask, mask + s->V); else s->fixed_mask.clear();
}
extern "C" int64_t *orc_grad(orc_sampler *s) { return s->GT.data(); }

extern "C" void orc_sched_sample(orc_sampler *s, const orc_schedule *sch, uint64_t seed, uint64_t sweep) {
  std::vector<double> buf;
  for (uint64_t i = 0; i < sch->n_order; ++i) {
    uint64_t vid = sch->order[i];
    const Var &var = s->vars[vid];
    if (var.is_evid && !s->opts.sample_evidence) continue;
    double A, B;
    philox_uniforms(seed, s->vid_offset + vid, sweep, A, B);
    uint64_t p = s->draw_sample(vid, s->a_evid.data(), s->weight_values.data(), OneShot{A}, buf);
    s->record_sample(vid, p);
  }
}

namespace {
// GT := GT128 where it fits; -> 0, or -1 with the text in orc_last_error (sticky until the next apply)
int publish_sums(orc_sampler *s) {
  const __int128 lo = INT64_MIN, hi = INT64_MAX;
  for (uint64_t i = 0; i < 3 * s->W; ++i) {
    const __int128 v = s->GT128[i];
    if (v < lo || v > hi) {
      if (!s->range_fault)
        g_err = std::string(i < s->W ? "gradient sum" : (i < 2 * s->W ? "update count" : "curvature bound")) +
                " of weight " + std::to_string(i % s->W) + " leaves int64 (about " + std::to_string((double)v) + ")";
      s->range_fault = true;
      s->GT[i] = v < lo ? INT64_MIN : INT64_MAX;
    } else {
      s->GT[i] = (int64_t)v;
    }
  }
  return s->range_fault ? -1 : 0;
}
}  // namespace

extern "C" int orc_sched_accumulate(orc_sampler *s, const orc_schedule *sch, uint64_t seed,
                                    uint64_t sweep) {
  std::vector<double> buf;
  if (s->GT128.size() != 3 * s->W) s->GT128.assign(3 * s->W, 0);
  __int128 *G = s->GT128.data(), *T = s->GT128.data() + s->W, *H = s->GT128.data() + 2 * s->W;
  for (uint64_t i = 0; i < sch->n_order; ++i) {
    uint64_t vid = sch->order[i];
    double A, B;
    philox_uniforms(seed, s->vid_offset + vid, sweep, A, B);
    uint64_t p = s->draw_sample(vid, s->a_free.data(), s->weight_values.data(), OneShot{A}, buf);
    s->a_free[vid] = p;
    s->a_evid[vid] = s->sample_evid(vid, OneShot{B}, buf);
    if (!s->sgd_triggers(s->vars[vid])) continue;
    // stepsize carries only the truthiness factor here (base step applied in apply)
    s->sgd_on_variable(vid, 1.0, [G, T](uint64_t wid, double t, double g) {
      G[wid] += llrint(kFixScale * (t * g));
      T[wid] += llrint(kFixScale * t);
    });
    s->curvature_bounds(vid, [H](uint64_t wid, double bound) { H[wid] += llrint(kHessScale * bound); });
  }
  return publish_sums(s);
}

// The device's batched update (apply_kernel, sampler_amd/csrc/sweep_kernels.h): the end point
// of the gradient flow the reference's T sequential updates of a weight follow over the batch,
// with the gradient linearised with slope h:  w -= s (G + reg T w),
// s = (1 - exp(-c stepsize)) / c, c = h + reg T  (-> the reference's own step for c stepsize
// << 1).  L1 (the reference adds reg_param per visit while the weight is
// negative, src/inference_result.h:76-78): the same flow with the push as a second field below
// zero, integrated piece by piece (l1_flow below restates apply_kernel's).
// hess != null: use these bounds instead of the accumulated ones (the device's fallback for
// plans without per-chunk tables applies every chunk with the WHOLE sweep's bounds)
extern "C" int orc_sched_apply_h(orc_sampler *s, double stepsize, const int64_t *hess);
extern "C" int orc_sched_apply(orc_sampler *s, double stepsize) { return orc_sched_apply_h(s, stepsize, nullptr); }
// out[W] = the curvature bounds of the SGD-triggering variables of the schedule (fixed point)
extern "C" int orc_sched_curvature(orc_sampler *s, const orc_schedule *sch, int64_t *out) {
  std::vector<__int128> acc(s->W, 0);
  for (uint64_t i = 0; i < sch->n_order; ++i) {
    const uint64_t vid = sch->order[i];
    if (!s->sgd_triggers(s->vars[vid])) continue;
    s->curvature_bounds(vid, [&acc](uint64_t wid, double bound) { acc[wid] += llrint(kHessScale * bound); });
  }
  int rc = 0;
  for (uint64_t w = 0; w < s->W; ++w) {
    if (acc[w] > (__int128)INT64_MAX) {
      g_err = "curvature bound of weight " + std::to_string(w) + " leaves int64";
      out[w] = INT64_MAX;
      rc = -1;
    } else {
      out[w] = (int64_t)acc[w];
    }
  }
  return rc;
}
namespace {
constexpr double kCurvMid = 0.5;   // DWX_CURV_MID of aux_kernels.h
// w < 0: dw/dtau = P - G - h (w - w0), P = reg T / stepsize;  w >= 0: dw/dtau = -G - h (w - w0);
// tau in [0, stepsize].  Fields pointing at each other across zero: the reference's weight
// rides the sawtooth w <- w - d + reg [w < 0] (values fill [-d, reg - d) evenly): end at its mean.
double l1_flow(double w0, double G, double h, double T, double stepsize, double reg) {
  if (!(stepsize > 0.0)) return w0;
  const double P = reg * T / stepsize, hm = kCurvMid * h;
  double w = w0, left = stepsize;
  for (int piece = 0; piece < 3; ++piece) {
    const double aP = -G - hm * (w - w0), aN = aP + P;
    double a;
    if (w < 0.0 || (w == 0.0 && aN <= 0.0)) a = aN;
    else if (w > 0.0 || aP > 0.0) a = aP;
    else return 0.5 * reg + aP * stepsize / T;
    double phi = hm > 0.0 ? -expm1(-hm * left) / hm : left;
    if (phi * h > 1.0) phi = 1.0 / h;
    const double end = w + a * phi;
    if (w == 0.0 || (w < 0.0) == (end <= 0.0)) return end;
    const double q = -w / a;
    left -= hm > 0.0 ? -log1p(-hm * q) / hm : q;
    w = 0.0;
    if (!(left > 0.0)) return 0.0;
  }
  return w;
}
// negligible curvature: the reference's own per-visit recurrence (src/inference_result.h:76-78) over
// the batch's T visits with the batch's mean gradient per visit, in closed form (l1_visits /
// l1_update of aux_kernels.h, restated)
double l1_visits(double w, double G, double T, double stepsize, double reg) {
  double n = T;
  const double d = stepsize * G / T, up = reg - d;
  if (w < 0.0) {
    if (!(up > 0.0)) return w + n * up;
    const double k = ceil(-w / up);
    if (k >= n) return w + n * up;
    w += k * up; n -= k;
  }
  if (!(d > 0.0)) return w - n * d;
  const double k = floor(w / d) + 1.0;
  if (k > n) return w - n * d;
  w -= k * d; n -= k;
  if (!(up > 0.0)) return w + n * up;
  if (n * d >= reg) return 0.5 * reg - d;
  double x = fmod(w + d - n * d, reg);
  if (x < 0.0) x += reg;
  return x - d;
}
double l1_update(double w0, double G, double h, double T, double stepsize, double reg) {
  return kCurvMid * h * stepsize <= 0.0625 ? l1_visits(w0, G, T, stepsize, reg) : l1_flow(w0, G, h, T, stepsize, reg);
}
}  // namespace
extern "C" int orc_sched_apply_h(orc_sampler *s, double stepsize, const int64_t *hess) {
  int64_t *G = s->GT.data(), *T = s->GT.data() + s->W, *H = s->GT.data() + 2 * s->W;
  // a sum that left int64 has no image in the device's containers: nothing is applied, the sums are dropped
  const bool fault = s->range_fault;
  s->range_fault = false;
  s->GT128.assign(3 * s->W, 0);
  if (fault) {
    for (uint64_t i = 0; i < 3 * s->W; ++i) s->GT[i] = 0;
    return -1;
  }
  // batch_step of aux_kernels.h: the flow with the middle of [0, h] as curvature, capped at 1 / (h + r)
  auto step = [stepsize](double h, double r) {
    const double c = kCurvMid * h + r, cb = h + r;
    const double st = c > 0.0 ? -expm1(-c * stepsize) / c : stepsize;
    return st * cb > 1.0 ? 1.0 / cb : st;
  };
  for (uint64_t w = 0; w < s->W; ++w) {
    const int64_t g = G[w], t = T[w], h = hess ? hess[w] : H[w];
    G[w] = 0; T[w] = 0; H[w] = 0;
    if (s->weights_isfixed[w] || t == 0) continue;
    const double Tt = (double)t / kFixScale, Gg = (double)g / kFixScale, hh = (double)h / kHessScale;
    double x = s->weight_values[w];
    if (s->opts.regularization == 1) {
      x -= step(hh, s->opts.reg_param * Tt) * (Gg + s->opts.reg_param * Tt * x);
    } else {
      x = l1_update(x, Gg, hh, Tt, stepsize, s->opts.reg_param);
    }
    s->weight_values[w] = x;
  }
  return 0;
}

extern "C" int orc_sched_sample_sgd(orc_sampler *s, const orc_schedule *sch, uint64_t seed,
                                    uint64_t sweep, double stepsize) {
  const int rc = orc_sched_accumulate(s, sch, seed, sweep);
  return orc_sched_apply(s, stepsize) ? -1 : rc;
}
