// level_build.cc -- see level_build.h: the host builders of a learning plan level.  Host-only; built with
// -ffp-contract=off (Makefile): the bounds and the curvature are the device's arithmetic term for term.
#include "level_build.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace dwx {

bool triggers_sgd(const dwx_options &o, uint32_t meta) {
  return o.learn_non_evidence || (!o.noise_aware && (meta & VM_EVIDENCE)) ||
         (o.noise_aware && (meta & VM_TRUTHINESS));
}

std::vector<uint32_t> cut_launch(const CompiledGraph &c, const std::vector<uint64_t> &sgd_work, uint64_t sgd_work_max_launch,
                                 size_t l, uint32_t nb) {
  const uint32_t t0 = c.launch_tile[l], t1 = c.launch_tile[l + 1];
  std::vector<uint32_t> cut{t0};
  if (t1 == t0) return cut;
  const uint64_t w0 = sgd_work[t0], total = sgd_work[t1] - w0;
  // nb pieces for the colour with the MOST work; a colour with less gets as many as keep its
  // pieces no bigger than that colour's (a greedy colouring leaves most of the work in the first
  // colours: cutting the small late colours nb-fold too only multiplies dependent launches --
  // 20 colours x 64 batches x 6 kernels on the power-law test graph)
  if (nb > 1 && sgd_work_max_launch > 0)
    nb = (uint32_t)std::max<uint64_t>(1, (total * nb + sgd_work_max_launch - 1) / sgd_work_max_launch);
  nb = std::max(1u, std::min(nb, t1 - t0));
  for (uint32_t b = 1; b < nb; ++b) {
    uint32_t t;
    if (total == 0) {
      t = t0 + (uint32_t)((uint64_t)(t1 - t0) * b / nb);
    } else {
      const uint64_t target = w0 + (total / nb) * b + (total % nb) * b / nb;
      t = (uint32_t)(std::lower_bound(sgd_work.begin() + t0, sgd_work.begin() + t1, target) - sgd_work.begin());
    }
    if (t > cut.back() && t < t1) cut.push_back(t);
  }
  cut.push_back(t1);
  return cut;
}

// How far one record can move its owner's potential between two of the owner's values, the
// building block of every curvature bound below: |sign(hit) - sign(miss)| * |f| for a unary
// factor (src/factor.h:112-299 at arity 1; boolean owner: hit = "1 satisfies the predicate",
// miss = "0 does"; categorical owner: the record sits in the row of the value that satisfies
// it), 2 |f| (arity - 1) for wider ones (a sign spans [-1, 1]; LINEAR counts up to arity - 1).
// Fixed weights do not move: 0.  The oracle restates this (orc_sched_accumulate).
static double host_unary_sign(uint32_t func, bool sat) {
  switch (func) {
    case FUNC_AND: case FUNC_ISTRUE: case FUNC_OR: case FUNC_IMPLY_NATURAL: return sat ? 1.0 : -1.0;
    case FUNC_EQUAL: return 1.0;
    default: return sat ? 1.0 : 0.0;
  }
}
static double record_delta(const CompiledGraph &c, uint32_t e, bool owner_is_cat) {
  const EdgeRec &r = c.edges[e];
  if (r.packed & EDGE_FIXED_FLAG) return 0.0;
  if (r.packed & EDGE_PRESIGNED) {
    float miss;
    std::memcpy(&miss, &r.aux, 4);
    return std::fabs((double)r.fval - (double)miss);
  }
  const double f = (r.packed & EDGE_F64_FLAG) ? c.edge_fval64[e] : (double)r.fval;
  const uint32_t ar = (r.packed & EDGE_INLINE2) ? 2u : ((r.packed >> EDGE_ARITY_SHIFT) & EDGE_ARITY_MASK);
  if (ar <= 1u) {
    const uint32_t fn = r.packed & EDGE_FUNC_MASK;
    const double hit = host_unary_sign(fn, owner_is_cat || r.aux == 1u);
    const double miss = host_unary_sign(fn, !owner_is_cat && r.aux == 0u);
    return std::fabs(hit - miss) * std::fabs(f);
  }
  return 2.0 * std::fabs(f) * (double)(ar - 1u);
}

// Gershgorin bound of one variable's share of the batch curvature, per record: the variable's
// SGD gradient over the weights has Jacobian kappa * d d^T for a boolean variable (logistic:
// kappa = p (1 - p) <= 1/4, d = the records' deltas) and J^T (diag(p) - p p^T) J for a
// categorical one (softmax over its value rows; absolute row sums of diag(p) - p p^T are
// 2 p (1 - p) <= 1/2).  Row sum of |H| for weight w: sum over w's records r of
//   1/4 * d_r * (sum of the row's deltas)              boolean
//   1/2 * d_r * (largest sum of deltas of a value row) categorical.
// fn(e, bound) is called for every record with a non-zero bound.
template <class Fn>
static void for_each_record_bound(const CompiledGraph &c, uint32_t p, Fn &&fn) {
  const uint32_t m = c.v_meta[p];
  const bool cat = m & VM_CATEGORICAL;
  double S = 0.0;
  for (uint32_t r = c.v_row[p]; r < c.v_row[p + 1]; ++r) {
    double sr = 0.0;
    for (uint32_t e = c.row_ptr[r]; e < c.row_ptr[r + 1]; ++e) sr += record_delta(c, e, cat);
    S = cat ? std::max(S, sr) : S + sr;
  }
  if (S == 0.0) return;
  const double kappa = cat ? 0.5 : 0.25;
  for (uint32_t e = c.row_ptr[c.v_row[p]]; e < c.row_ptr[c.v_row[p + 1]]; ++e) {
    const double d = record_delta(c, e, cat);
    if (d != 0.0) fn(e, kappa * d * S);
  }
}

// The domain of the learning sums.  A mini-batch adds, per weight, int64 sums in
// fixed point: G += llrint(2^30 t g) and T += llrint(2^30 t) per visited record (DWX_BUF_GRAD), and the
// static h = sum llrint(2^10 kappa d S) (for_each_record_bound).  Nothing on the sweep path saturates or
// checks them -- a wrapped sum is a gradient of the wrong sign, and the oracle's schedule mode, which
// restates the same containers, used to agree with it bit for bit -- so the domain is enforced here,
// where a plan's mini-batches are made.  Per group of variables that share an update (`groups`:
// device-order position ranges) and per weight, the WORST case of each sum over any assignment:
//   G: a record's |g| = |pot_free - pot_evid| is at most its delta (record_delta: the two signs of a
//      unary factor, 2 |f| (arity - 1) beyond); its visits carry a truthiness of 1 in all, or -- a
//      categorical variable under noise_aware -- of at most the variable's total truthiness (row d is
//      visited with t_d as the evidence row and with every other value's t as the proposal's row: up to one
//      visit per value row, each rounding its own term, so one unit per value row is added on top);
//   T: the same visits, 2^30 t each;   h: exactly the table's value.
// Every term is rounded UP to an integer, so the true sum of every prefix, in any order, stays inside
// the bound: the kernels' partial sums (LDS accumulators, block rows, per-record atomics) cannot wrap
// either.  Sums in uint64, saturating: a bound of exactly 2^63 - 1 passes, 2^63 does not.
// -> empty, or the text of the DWX_E_LIMIT error, naming the weight.
std::string learning_range_error(const CompiledGraph &c, const dwx_options &o,
                                 const std::vector<std::pair<uint32_t, uint32_t>> &groups) {
  if (!c.W || groups.empty()) return std::string();
  constexpr uint64_t kLimit = (uint64_t)INT64_MAX, kSat = UINT64_MAX;
  const uint32_t nth = host_threads();
  std::vector<uint64_t> acc(3 * c.W, 0);   // [G | T | h] bounds of the current group
  auto sat_add = [](uint64_t *a, uint64_t v) -> uint64_t {   // -> the value before
    uint64_t old = __atomic_load_n(a, __ATOMIC_RELAXED);
    for (;;) {
      const uint64_t next = old > kSat - v ? kSat : old + v;
      if (__atomic_compare_exchange_n(a, &old, next, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) return old;
    }
  };
  auto up = [](double x) -> uint64_t {   // ceil, saturating
    return x >= 18446744073709549568.0 ? kSat : (uint64_t)std::ceil(x);
  };
  for (size_t k = 0; k < groups.size(); ++k) {
    const uint32_t p0 = groups[k].first, p1 = groups[k].second;
    const uint32_t T = std::max(1u, std::min<uint32_t>(nth, (p1 - p0) / 4096u + 1u));
    std::vector<std::vector<uint32_t>> touched(T);
    parallel_parts(p1 - p0, T, [&](uint32_t t, uint64_t b, uint64_t e) {
      // a thread's adds go through a small direct-mapped cache: heavily tied weights (eight weights
      // on 10^7 records) would otherwise be one contended cache line
      struct Slot { uint32_t wid; uint64_t g, t, h; };
      constexpr uint32_t kSlots = 64;
      Slot cache[kSlots];
      for (auto &sl : cache) sl = Slot{0xFFFFFFFFu, 0, 0, 0};
      auto flush = [&](Slot &sl) {
        if (sl.wid == 0xFFFFFFFFu) return;
        const uint64_t before = sat_add(&acc[c.W + sl.wid], sl.t);
        sat_add(&acc[sl.wid], sl.g);
        sat_add(&acc[2 * c.W + sl.wid], sl.h);
        if (before == 0) touched[t].push_back(sl.wid);
        sl = Slot{0xFFFFFFFFu, 0, 0, 0};
      };
      auto slot_of = [&](uint32_t wid) -> Slot & {
        Slot &sl = cache[wid % kSlots];
        if (sl.wid != wid) { flush(sl); sl.wid = wid; }
        return sl;
      };
      auto add = [](uint64_t &a, uint64_t v) { a = a > kSat - v ? kSat : a + v; };
      for (uint32_t p = p0 + (uint32_t)b; p < p0 + (uint32_t)e; ++p) {
        const uint32_t m = c.v_meta[p];
        if (!triggers_sgd(o, m)) continue;
        const bool cat = m & VM_CATEGORICAL;
        double tt = 1.0;
        if (cat && o.noise_aware) {
          tt = 0.0;
          if (!c.row_truth.empty())
            for (uint32_t r = c.v_row[p]; r < c.v_row[p + 1]; ++r) tt += c.row_truth[r];
        }
        if (!(tt > 0.0)) continue;
        // (such a record is visited up to once per value row, each visit rounding its own term: half a unit each)
        const uint64_t visits_slack = cat && o.noise_aware ? c.v_row[p + 1] - c.v_row[p] : 0u;
        const uint64_t t_up = up(FIX_SCALE * tt) + visits_slack;
        for (uint32_t e2 = c.row_ptr[c.v_row[p]]; e2 < c.row_ptr[c.v_row[p + 1]]; ++e2) {
          if (c.edges[e2].packed & EDGE_FIXED_FLAG) continue;
          Slot &sl = slot_of(c.edges[e2].wid);
          add(sl.t, t_up);
          add(sl.g, up(FIX_SCALE * (tt * record_delta(c, e2, cat))));
          add(sl.g, visits_slack);
        }
        for_each_record_bound(c, p, [&](uint32_t e2, double bound) {
          add(slot_of(c.edges[e2].wid).h, up(H_SCALE * bound));
        });
      }
      for (auto &sl : cache) flush(sl);
    }, 4096);
    uint32_t bad = 0xFFFFFFFFu;
    for (const auto &list : touched)
      for (uint32_t w : list)
        if (acc[w] > kLimit || acc[c.W + w] > kLimit || acc[2 * c.W + w] > kLimit) bad = std::min(bad, w);
    if (bad != 0xFFFFFFFFu) {
      const uint64_t w = bad;
      char buf[512];
      const char *which = acc[bad] > kLimit ? "gradient sum (2^30 x sum of t |g|)"
                          : (acc[2 * c.W + bad] > kLimit ? "curvature bound (2^10 x sum of kappa d S)" : "update count (2^30 x sum of t)");
      const uint64_t v = acc[bad] > kLimit ? acc[bad] : (acc[2 * c.W + bad] > kLimit ? acc[2 * c.W + bad] : acc[c.W + bad]);
      snprintf(buf, sizeof buf,
               "the learning sums of weight %llu can leave int64 in mini-batch %zu of %zu: worst-case %s = %.17g%s, "
               "the limit is 2^63 - 1 (fewer or smaller feature values on this weight, or a finer plan: dwx_sgd_plan's force_batches)",
               (unsigned long long)w, k + 1, groups.size(), which, (double)v, v == kSat ? " or more" : "");
      return buf;
    }
    for (const auto &list : touched)
      for (uint32_t w : list) acc[w] = acc[c.W + w] = acc[2 * c.W + w] = 0;
  }
  return std::string();
}

namespace hostb {
void build_static_tables(const CompiledGraph &c, const dwx_options &o, const std::vector<TileGroup> &groups,
                         RawArray<long long> &ts, long long *t_max, long long *h_max) {
  const uint32_t nth = host_threads(), nc = (uint32_t)groups.size();
  ts.reset((size_t)nc * 2 * c.W);
  parallel_ranges((uint64_t)nc * 2 * c.W, nth, [&](uint64_t b, uint64_t e) { std::fill(ts.data() + b, ts.data() + e, 0LL); });
  const long long one = (long long)FIX_SCALE;
  // Few groups (the un-split level has ONE: a single thread used to walk all of config 5's 10^9
  // records here): the variables of a group are shared out over the threads instead, which add
  // into the group's rows atomically -- integer sums, the same tables in any order.
  auto group_rows = [&](uint64_t k, uint32_t pb, uint32_t pe, auto &&add) {
    long long *row = ts.data() + k * 2 * c.W, *hrow = row + c.W;
    for (uint32_t p = pb; p < pe; ++p) {
      const uint32_t m = c.v_meta[p];
      if (!triggers_sgd(o, m)) continue;
      for_each_record_bound(c, p, [&](uint32_t e, double bound) {
        add(&hrow[c.edges[e].wid], (long long)std::llrint(H_SCALE * bound));
      });
      if (m & VM_CATEGORICAL) continue;   // (their counts depend on the samples: dynamic)
      for (uint32_t e = c.row_ptr[c.v_row[p]]; e < c.row_ptr[c.v_row[p] + 1]; ++e)
        if (!c.w_fixed[c.edges[e].wid]) add(&row[c.edges[e].wid], one);
    }
  };
  if (nc >= nth || nth <= 1) {
    parallel_ranges(nc, std::min(nth, nc), [&](uint64_t kb, uint64_t ke) {
      for (uint64_t k = kb; k < ke; ++k)
        group_rows(k, c.tile_v[groups[k].t0], c.tile_v[groups[k].t1], [](long long *a, long long v) { *a += v; });
    }, 2);
  } else {
    for (uint64_t k = 0; k < nc; ++k) {
      const uint32_t p0 = c.tile_v[groups[k].t0], p1 = c.tile_v[groups[k].t1];
      parallel_ranges(p1 - p0, nth, [&](uint64_t b, uint64_t e) {
        group_rows(k, p0 + (uint32_t)b, p0 + (uint32_t)e,
                   [](long long *a, long long v) { __atomic_fetch_add(a, v, __ATOMIC_RELAXED); });
      });
    }
  }
  const uint32_t T = std::max(1u, std::min(nth, 16u));
  std::vector<long long> hm(T, 0), tm(T, 0);
  parallel_parts((uint64_t)nc * c.W, T, [&](uint32_t t, uint64_t b, uint64_t e) {
    long long h = 0, tt = 0;
    for (uint64_t i = b; i < e; ++i) {
      const uint64_t k = i / c.W, w = i % c.W;
      tt = std::max(tt, ts[k * 2 * c.W + w]);
      h = std::max(h, ts[(k * 2 + 1) * c.W + w]);
    }
    hm[t] = h; tm[t] = tt;
  }, 0);
  *t_max = *std::max_element(tm.begin(), tm.end());
  *h_max = *std::max_element(hm.begin(), hm.end());
}

void build_incidence(const CompiledGraph &c, const dwx_options &o, const std::vector<TileGroup> &groups,
                     uint64_t block_pull_min_w, uint64_t bp_tiles, bool allow_one_plane, Incidence &out) {
  const uint32_t nth = host_threads(), nc = (uint32_t)groups.size();
  std::vector<uint8_t> other_owner(nc, 0);   // per group: an entry's owner is not a boolean evidence variable
  std::vector<uint32_t> chunk_of(c.tiles.size(), 0);
  for (uint32_t k = 0; k < nc; ++k)
    for (uint32_t t = groups[k].t0; t < groups[k].t1; ++t) chunk_of[t] = k;
  struct Inc { uint32_t wid, slot; float d; uint32_t chunk; };
  RawArray<Inc> by_w, by_c;
  std::vector<uint64_t> w_start, c_start;
  parallel_group_by_key<Inc>(
      c.tiles.size(), nth, c.W, [](const Inc &r) { return (uint64_t)r.wid; },
      [&](uint64_t tb, uint64_t te, auto &&emit) {
        for (uint64_t ti = tb; ti < te; ++ti) {
          const TileDesc &td = c.tiles[ti];
          // (TILE_PULL_UNARY: only the tile's pre-signed records; not in a K = 12 build, whose
          // kernels walk such tiles generically)
          const bool unary_only = !(td.flags & TILE_PULL) && (td.flags & TILE_PULL_UNARY) && c.ecap <= 6 * BLOCK_THREADS;
          if (!(td.flags & TILE_PULL) && !unary_only) continue;
          if (td.flags & TILE_OUTSIDE) continue;   // giant_kernel / wide_kernel: atomics
          for (uint32_t l = 0; l < td.nv; ++l) {
            const uint32_t p = td.v0 + l, m = c.v_meta[p];
            // (the boolean pull tiles' own condition, NOT triggers_sgd: the two differ on purpose)
            if (!(o.learn_non_evidence || (!o.noise_aware && (m & VM_EVIDENCE)))) continue;
            for (uint32_t e = c.row_ptr[c.v_row[p]]; e < c.row_ptr[c.v_row[p] + 1]; ++e) {
              const EdgeRec &r = c.edges[e];
              if (r.packed & EDGE_FIXED_FLAG) continue;
              if (unary_only && !(r.packed & EDGE_PRESIGNED)) continue;
              float miss;
              std::memcpy(&miss, &r.aux, 4);
              const float dd = r.fval - miss;    // exact: |hit| == |miss| or one of them is 0
              if (dd == 0.0f) continue;
              if (((m & VM_CATEGORICAL) || !(m & VM_EVIDENCE)) && !other_owner[chunk_of[ti]]) other_owner[chunk_of[ti]] = 1;
              emit(Inc{r.wid, (uint32_t)(ti * BLOCK_THREADS + l), dd, chunk_of[ti]});
            }
          }
        }
      },
      by_w, w_start, 64);
  const uint64_t n_inc = by_w.size();
  if (n_inc + (uint64_t)nc * PULL_RUN >= 0xFFFFFFFFull)
    throw std::invalid_argument("incidence list exceeds 2^32-1 entries");
  // the groups' lists: by weight inside a group
  const RawArray<Inc> *src = &by_w;
  if (nc > 1) {
    parallel_group_by_key<Inc>(
        n_inc, nth, nc, [](const Inc &r) { return (uint64_t)r.chunk; },
        [&](uint64_t b, uint64_t e, auto &&emit) { for (uint64_t i = b; i < e; ++i) emit(by_w[i]); },
        by_c, c_start);
    by_w.clear();
    src = &by_c;
  } else {
    c_start = {0, n_inc};
  }
  // Block pull (graphs with many weights): per group, rows of BP_ROW * depth entries per
  // (variable block, weight) for pull_ell_kernel; an entry beyond its row stays on the list.
  RawArray<Inc> kept;                    // the lists of all groups after the tables took their entries
  std::vector<uint64_t> kept_start;
  {
    // the distinct record deltas (few: feature values repeat), as fixed-point steps
    std::vector<uint32_t> dvals;
    bool enabled = n_inc && c.W >= block_pull_min_w;
    if (enabled) {
      const uint32_t T = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nth, n_inc / 65536));
      std::vector<std::vector<uint32_t>> local(T);
      parallel_parts(n_inc, T, [&](uint32_t t, uint64_t b, uint64_t e) {
        std::vector<uint32_t> &v = local[t];
        uint32_t last = 0; bool have = false;
        for (uint64_t i = b; i < e && v.size() <= 4 * BP_MAX_DELTAS; ++i) {
          uint32_t bits; std::memcpy(&bits, &(*src)[i].d, 4);
          if (have && bits == last) continue;
          last = bits; have = true;
          v.push_back(bits);
          if (v.size() % 4096 == 0) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
        }
        std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end());
      }, 0);
      for (auto &v : local) dvals.insert(dvals.end(), v.begin(), v.end());
      std::sort(dvals.begin(), dvals.end()); dvals.erase(std::unique(dvals.begin(), dvals.end()), dvals.end());
      enabled = dvals.size() <= BP_MAX_DELTAS;
    }
    if (enabled) {
      const uint64_t Wp = (c.W + BP_THREADS - 1) / BP_THREADS * BP_THREADS;
      out.bp.resize(nc);
      uint64_t max_blocks = 0;
      std::vector<uint64_t> ov_count(nc, 0);
      std::vector<RawArray<Inc>> ov(nc);
      std::vector<uint8_t> has(c.tiles.size(), 0);
      std::vector<uint32_t> block_of(c.tiles.size(), 0);
      for (uint32_t k = 0; k < nc; ++k) {
        const Inc *ent = src->data() + c_start[k];
        const uint64_t n = c_start[k + 1] - c_start[k];
        if (!n) continue;
        // (1) blocks: runs of <= `tiles` consecutive tiles, started at tiles that own entries
        const bool one_plane = bp_one_plane(dvals.size(), o.learn_non_evidence != 0, o.noise_aware != 0, !other_owner[k], allow_one_plane);
        const uint64_t tiles = bp_block_tiles(one_plane, bp_tiles);
        std::fill(has.begin(), has.end(), 0);
        parallel_ranges(n, nth, [&](uint64_t b, uint64_t e) {
          for (uint64_t i = b; i < e; ++i) {   // (test first: the flags are shared by all threads)
            uint8_t &h = has[ent[i].slot / BLOCK_THREADS];
            if (!h) h = 1;
          }
        });
        std::vector<uint32_t> tile0;
        for (uint32_t ti = 0; ti < c.tiles.size(); ++ti) {
          if (!has[ti]) continue;
          if (tile0.empty() || ti >= tile0.back() + tiles) tile0.push_back(ti);
          block_of[ti] = (uint32_t)tile0.size() - 1;
        }
        const uint64_t nvb = tile0.size();
        const double lambda = (double)n / ((double)c.W * (double)nvb);
        if (lambda < 0.5) continue;   // nearly empty rows: this group keeps its list
        const bool packed = dvals.size() == 1;       // one delta: three 19-bit slots per 8-byte word
        const uint32_t depth = bp_row_depth(lambda, packed), cap = (packed ? BP_PK_ROW : BP_ROW) * depth;
        // (2) where each weight's entries start inside the group (they are sorted by weight)
        std::vector<uint64_t> w_at(c.W + 1, n);
        parallel_ranges(n, nth, [&](uint64_t b, uint64_t e) {
          for (uint64_t i = b; i < e; ++i) {
            const uint32_t w = ent[i].wid, prev = i ? ent[i - 1].wid + 1 : 0;
            if (!i || ent[i - 1].wid != w) for (uint32_t x = prev; x <= w; ++x) w_at[x] = i;
          }
        });
        // (3) the table; entries of one weight come in tile order: blocks ascending
        RawArray<unsigned long long> &ell8 = out.bp[k].ell;
        ell8.reset(nvb * depth * Wp * (packed ? 1 : 2));   // (8-byte words: U32x4 rows are two)
        U32x4 *ell = (U32x4 *)ell8.data();
        parallel_ranges(ell8.size(), nth, [&](uint64_t b, uint64_t e) { std::memset((void *)(ell8.data() + b), packed ? 0 : 0xFF, (e - b) * 8); });
        std::vector<uint64_t> &ovs = out.bp[k].ov_start;   // per weight: entries left on the list
        ovs.assign(c.W + 1, 0);
        parallel_ranges(c.W, nth, [&](uint64_t wb, uint64_t we) {
          for (uint64_t w = wb; w < we; ++w) {
            uint32_t cur = ~0u, kk = 0;
            uint64_t o = 0;
            for (uint64_t i = w_at[w]; i < w_at[w + 1]; ++i) {
              const Inc &r = ent[i];
              const uint32_t ti = r.slot / BLOCK_THREADS, vb = block_of[ti];
              if (vb != cur) {
                cur = vb; kk = 0;
                if (one_plane) {
                  // the block's row: its first `cap` entries, those that step by +q (v_init != 1) first
                  uint64_t e1 = i;
                  uint32_t n_plus = 0;
                  while (e1 < w_at[w + 1] && e1 - i < cap && block_of[ent[e1].slot / BLOCK_THREADS] == vb) ++e1;
                  auto plus = [&](const Inc &x) { return c.v_init[c.tiles[x.slot / BLOCK_THREADS].v0 + x.slot % BLOCK_THREADS] != 1u; };
                  for (uint64_t j = i; j < e1; ++j) n_plus += plus(ent[j]) ? 1u : 0u;
                  uint32_t at_plus = 0, at_minus = n_plus;
                  for (uint64_t j = i; j < e1; ++j) {
                    const Inc &x = ent[j];
                    const bool p = plus(x);
                    const uint32_t at = p ? at_plus++ : at_minus++;
                    unsigned long long &word = ell8[((uint64_t)vb * depth + at / BP_PK_ROW) * Wp + w];
                    word = bp1_pack_entry(word, at % BP_PK_ROW, (x.slot / BLOCK_THREADS - tile0[vb]) * BLOCK_THREADS + x.slot % BLOCK_THREADS, p);
                  }
                }
              }
              if (kk < cap && one_plane) {
                // (written with the block's first entry)
              } else if (kk < cap && packed) {
                unsigned long long &word = ell8[((uint64_t)vb * depth + kk / BP_PK_ROW) * Wp + w];
                word = bp_pack_entry(word, kk % BP_PK_ROW, (ti - tile0[vb]) * BLOCK_THREADS + r.slot % BLOCK_THREADS);
              } else if (kk < cap) {
                uint32_t bits; std::memcpy(&bits, &r.d, 4);
                const uint32_t di = (uint32_t)(std::lower_bound(dvals.begin(), dvals.end(), bits) - dvals.begin());
                ell[((uint64_t)vb * depth + kk / BP_ROW) * Wp + w].v[kk % BP_ROW] =
                    ((ti - tile0[vb]) * BLOCK_THREADS + r.slot % BLOCK_THREADS) | (di << BP_SLOT_BITS);
              } else {
                ++o;
              }
              ++kk;
            }
            ovs[w + 1] = o;
          }
        });
        for (uint64_t w = 0; w < c.W; ++w) ovs[w + 1] += ovs[w];
        ov_count[k] = ovs[c.W];
        // the entries the rows could not take, in list order (same walk, now copying)
        ov[k].reset(ov_count[k]);
        if (ov_count[k]) {
          Inc *dst = ov[k].data();
          parallel_ranges(c.W, nth, [&](uint64_t wb, uint64_t we) {
            for (uint64_t w = wb; w < we; ++w) {
              uint32_t cur = ~0u, kk = 0;
              uint64_t o = ovs[w];
              for (uint64_t i = w_at[w]; i < w_at[w + 1]; ++i) {
                const uint32_t vb = block_of[ent[i].slot / BLOCK_THREADS];
                if (vb != cur) { cur = vb; kk = 0; }
                if (kk >= cap) dst[o++] = ent[i];
                ++kk;
              }
            }
          });
        }
        Incidence::BlockTable &bt = out.bp[k];
        bt.tile0.swap(tile0);
        bt.blocks = (uint32_t)nvb; bt.depth = depth;
        bt.tiles = (uint32_t)tiles; bt.one_plane = one_plane;
        bt.total = n; bt.on_list = ov_count[k];
        max_blocks = std::max(max_blocks, nvb);
      }
      if (max_blocks) {
        // the lists shrink to what the tables left (same order: by weight inside a group)
        kept_start.assign(nc + 1, 0);
        for (uint32_t k = 0; k < nc; ++k)
          kept_start[k + 1] = kept_start[k] + (out.bp[k].blocks ? ov_count[k] : c_start[k + 1] - c_start[k]);
        kept.reset(kept_start[nc]);
        for (uint32_t k = 0; k < nc; ++k) {
          const Inc *ent = src->data() + c_start[k];
          const uint64_t n = c_start[k + 1] - c_start[k];
          Inc *dst = kept.data() + kept_start[k];
          if (!out.bp[k].blocks) std::copy(ent, ent + n, dst);
          else std::copy(ov[k].data(), ov[k].data() + ov[k].size(), dst);
        }
        out.dvals.swap(dvals);
        out.max_blocks = max_blocks; out.wp = Wp;
        by_w.clear(); by_c.clear();
        src = &kept;
        c_start = kept_start;
      } else {
        out.bp.clear();
      }
    }
  }
  // columns; every chunk padded to whole runs with neutral entries (its last weight, zero
  // contribution), so the kernel's 16-byte loads never leave the chunk
  std::vector<uint64_t> off(nc + 1, 0);
  for (uint32_t k = 0; k < nc; ++k)
    off[k + 1] = off[k] + (c_start[k + 1] - c_start[k] + PULL_RUN - 1) / PULL_RUN * PULL_RUN;
  const uint64_t padded = off[nc];
  out.inc_begin.resize(nc); out.inc_end.resize(nc);
  if (padded) {
    RawArray<uint32_t> &iw = out.inc_wid, &is = out.inc_slot;
    RawArray<float> &id = out.inc_d;
    iw.reset(padded); is.reset(padded); id.reset(padded);
    for (uint32_t k = 0; k < nc; ++k) {
      out.inc_begin[k] = (uint32_t)off[k]; out.inc_end[k] = (uint32_t)off[k + 1];
      const uint64_t n = c_start[k + 1] - c_start[k], base = c_start[k];
      parallel_ranges(off[k + 1] - off[k], nth, [&](uint64_t b, uint64_t e) {
        for (uint64_t i = b; i < e; ++i) {
          const Inc &r = (*src)[base + std::min(i, n - 1)];
          iw[off[k] + i] = r.wid; is[off[k] + i] = r.slot; id[off[k] + i] = i < n ? r.d : 0.0f;
        }
      });
    }
  }
}

// A variable v that triggers SGD contributes kappa_v d_v d_v^T to the batch Hessian bound, d_v[w] = sum
// of |d_r| over its non-fixed records with weight w, d_r = the change of the record's potential between
// proposals (record_delta), kappa = 1/4 (logistic) for boolean, 1/2 for categorical variables.  The
// largest eigenvalue of that matrix is estimated by two power iterations from the all-ones vector (the
// matrix is entrywise non-negative: the iteration converges from below to its Perron value) combined
// with the largest diagonal entry (exact for a batch dominated by one heavily tied weight).
double batch_curvature(const CompiledGraph &c, const dwx_options &o, uint32_t p0, uint32_t p1, CurvatureScratch &sc) {
  sc.x.resize(c.W); sc.y.resize(c.W); sc.diag.resize(c.W); sc.seen.resize(c.W);   // (all zero between calls)
  std::vector<double> &x = sc.x, &y = sc.y, &diag = sc.diag;
  std::vector<uint8_t> &seen = sc.seen;
  std::vector<uint32_t> &touched = sc.touched;
  // y = H x, three times: x0 = 1 (y = row sums), then two normalised power steps
  double lam = 0.0, dmax = 0.0;
  if (batch_is_dense(c, p0, p1)) {
    // a batch that touches a good part of the weight table: variable ranges in parallel on ALL host
    // threads, ONE shared y (and diagonal) in 64-bit FIXED POINT -- integer atomic adds: the sums
    // do not depend on the order, lambda is reproducible -- and dense passes over the table.
    // (Round 4: this was one private f64 vector per thread, hence 16 threads at most and a merge
    // pass over 16 W doubles per iteration: 6 s of config 5's sampler create at W = 10 M.)
    const uint32_t T = host_threads();
    // bound of one term kappa d dot (x <= 1 entrywise: dot <= the variable's sum of deltas) and of
    // a weight's number of terms, for the scale
    std::vector<double> umax(T, 0.0), dmx(T, 0.0);
    std::vector<uint64_t> nrec(T, 0);
    parallel_parts(p1 - p0, T, [&](uint32_t t, uint64_t b, uint64_t e) {
      double u = 0.0, dm = 0.0;
      uint64_t n = 0;
      for (uint32_t p = p0 + (uint32_t)b; p < p0 + (uint32_t)e; ++p) {
        const uint32_t m = c.v_meta[p];
        if (!triggers_sgd(o, m)) continue;
        const bool cat = (m & VM_CATEGORICAL) != 0;
        const uint32_t e0 = c.row_ptr[c.v_row[p]], e1 = c.row_ptr[c.v_row[p + 1]];
        double S = 0.0, dv = 0.0;
        for (uint32_t k = e0; k < e1; ++k) { const double d = record_delta(c, k, cat); S += d; dv = std::max(dv, d); }
        u = std::max(u, (cat ? 0.5 : 0.25) * dv * S);
        dm = std::max(dm, (cat ? 0.5 : 0.25) * dv * dv);
        n += e1 - e0;
      }
      umax[t] = u; dmx[t] = dm; nrec[t] = n;
    }, 0);
    double U = 0.0, D2 = 0.0;
    uint64_t R = 0;
    for (uint32_t t = 0; t < T; ++t) { U = std::max(U, umax[t]); D2 = std::max(D2, dmx[t]); R += nrec[t]; }
    if (U > 0.0 && R > 0) {
      const double scale = std::ldexp(1.0, 62) / ((double)R * U), dscale = std::ldexp(1.0, 62) / ((double)R * D2);
      RawArray<long long> yfix(c.W), dfix(c.W);
      parallel_ranges(c.W, T, [&](uint64_t b, uint64_t e) { for (uint64_t w = b; w < e; ++w) { yfix[w] = 0; dfix[w] = 0; } });
      std::fill(x.begin(), x.end(), 1.0);
      for (int iter = 0; iter < 3; ++iter) {
        parallel_parts(p1 - p0, T, [&](uint32_t, uint64_t b, uint64_t e) {
          for (uint32_t p = p0 + (uint32_t)b; p < p0 + (uint32_t)e; ++p) {
            const uint32_t m = c.v_meta[p];
            if (!triggers_sgd(o, m)) continue;
            const uint32_t e0 = c.row_ptr[c.v_row[p]], e1 = c.row_ptr[c.v_row[p + 1]];
            const bool cat = (m & VM_CATEGORICAL) != 0;
            const double kappa = cat ? 0.5 : 0.25;
            double dot = 0.0;
            for (uint32_t k = e0; k < e1; ++k) dot += record_delta(c, k, cat) * x[c.edges[k].wid];
            for (uint32_t k = e0; k < e1; ++k) {
              const double d = record_delta(c, k, cat);
              if (d == 0.0) continue;
              __atomic_fetch_add(&yfix[c.edges[k].wid], (long long)std::llrint(scale * (kappa * d * dot)), __ATOMIC_RELAXED);
              if (iter == 0) __atomic_fetch_add(&dfix[c.edges[k].wid], (long long)std::llrint(dscale * (kappa * d * d)), __ATOMIC_RELAXED);
            }
          }
        }, 0);
        std::vector<double> part(3 * T, 0.0);
        parallel_parts(c.W, T, [&](uint32_t t, uint64_t b, uint64_t e) {
          double xy = 0.0, xx = 0.0, yy = 0.0;
          for (uint64_t w = b; w < e; ++w) {
            const double yw = (double)yfix[w] / scale;
            y[w] = yw;
            xy += x[w] * yw; xx += x[w] * x[w]; yy += yw * yw;
          }
          part[3 * t] = xy; part[3 * t + 1] = xx; part[3 * t + 2] = yy;
        }, 0);
        double xy = 0.0, xx = 0.0, yy = 0.0;
        for (uint32_t t = 0; t < T; ++t) { xy += part[3 * t]; xx += part[3 * t + 1]; yy += part[3 * t + 2]; }
        if (xx > 0) lam = std::max(lam, xy / xx);
        const double norm = yy > 0 ? 1.0 / std::sqrt(yy) : 0.0;
        parallel_ranges(c.W, T, [&](uint64_t b, uint64_t e) { for (uint64_t w = b; w < e; ++w) { x[w] = y[w] * norm; y[w] = 0.0; yfix[w] = 0; } });
      }
      std::vector<double> dpart(T, 0.0);
      parallel_parts(c.W, T, [&](uint32_t t, uint64_t b, uint64_t e) {
        long long mx = 0;
        for (uint64_t w = b; w < e; ++w) { mx = std::max(mx, dfix[w]); x[w] = 0.0; }
        dpart[t] = (double)mx / dscale;
      }, 0);
      for (uint32_t t = 0; t < T; ++t) dmax = std::max(dmax, dpart[t]);
    } else {
      std::fill(x.begin(), x.end(), 0.0);
    }
  } else {
    for (int iter = 0; iter < 3; ++iter) {
      for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t m = c.v_meta[p];
        if (!triggers_sgd(o, m)) continue;
        const uint32_t e0 = c.row_ptr[c.v_row[p]], e1 = c.row_ptr[c.v_row[p + 1]];
        const double kappa = (m & VM_CATEGORICAL) ? 0.5 : 0.25;
        double dot = 0.0;
        for (uint32_t e = e0; e < e1; ++e) {
          const double d = record_delta(c, e, (m & VM_CATEGORICAL) != 0);
          if (d == 0.0) continue;
          const uint32_t w = c.edges[e].wid;
          if (!seen[w]) { seen[w] = 1; touched.push_back(w); x[w] = 1.0; }
          dot += d * x[w];
        }
        for (uint32_t e = e0; e < e1; ++e) {
          const double d = record_delta(c, e, (m & VM_CATEGORICAL) != 0);
          if (d == 0.0) continue;
          y[c.edges[e].wid] += kappa * d * dot;
          if (iter == 0) diag[c.edges[e].wid] += kappa * d * d;   // (lower bound of H_ww)
        }
      }
      double xy = 0.0, xx = 0.0, yy = 0.0;
      for (uint32_t w : touched) { xy += x[w] * y[w]; xx += x[w] * x[w]; yy += y[w] * y[w]; }
      if (xx > 0) lam = std::max(lam, xy / xx);
      const double norm = yy > 0 ? 1.0 / std::sqrt(yy) : 0.0;
      for (uint32_t w : touched) { x[w] = y[w] * norm; y[w] = 0.0; }
    }
    for (uint32_t w : touched) { dmax = std::max(dmax, diag[w]); diag[w] = 0.0; seen[w] = 0; x[w] = 0.0; }
    touched.clear();
  }
  return std::max(lam, dmax);
}

}  // namespace hostb
}  // namespace dwx
