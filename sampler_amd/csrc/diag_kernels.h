// diag_kernels.h -- split-R-hat and effective sample size of every value row, computed from the sample trace's
// ring where it lies (dwx_trace_diagnostics; include/dwx.h states the definition, DESIGN.md 3.1g the layout).
// NOTE: tests/hipemu/Makefile names its prerequisite headers and does not name this one: after an edit of
// this header ALONE, run `make clean` in tests/hipemu before `make`, or the emulated libraries stay stale.
//
// NO reference counterpart: the reference only counts the drawn values (src/gibbs_sampler.h:160-167).
//
// A row's 0/1 series is walked in chunks of 64 entries, oldest first, bit i of a chunk = entry e0 + i.  Both
// plane widths build such chunks (BITS = 1: a 64 x 64 bit transpose by ballots; BITS = 8: byte == value from an
// LDS tile) and feed the SAME two device functions: diag_accumulate (integer statistics: popcounts of the
// series ANDed with itself shifted) and diag_finish (the fixed f64 formulas over them), so that the two widths
// cannot drift apart.  Everything a launch geometry could reorder is an integer sum.
#ifndef DWX_DIAG_KERNELS_H_
#define DWX_DIAG_KERNELS_H_

#include "device_intrinsics.h"

namespace dwx {

constexpr uint32_t DIAG_MAX_LAG = 64;
constexpr uint32_t DIAG_BIT_THREADS = 1024;   // BITS = 1: 16 waves on 16 adjacent word columns = 128 bytes of every plane
constexpr uint32_t DIAG_BYTE_THREADS = 256;   // BITS = 8: a row per lane
constexpr uint32_t DIAG_NO_ROW = 0xFFFFFFFFu;
constexpr uint32_t DIAG_FLAG_CONSTANT = 1u, DIAG_FLAG_TRUNCATED = 2u;

// integer statistics of one row's series
struct DiagStats {
  uint32_t c[DIAG_MAX_LAG + 1];      // c[t] = sum_{i < n - t} x_i x_{i+t}
  uint32_t k, k1, k2;                // ones; ones among the first h = n / 2 entries; among the last h
  unsigned long long first, last;    // entries 0 .. 63 (bit i = entry i); entries n - 64 .. n - 1 (bit 63 = entry n - 1)
  unsigned long long prev;           // the chunk before the current one
};

// a workgroup's candidates for the summary's extremes (device row numbering; DIAG_NO_ROW: none)
struct DiagPartial {
  double max_rhat, min_ess;
  uint32_t max_row, min_row;
};

DWX_DEV unsigned long long diag_below(uint32_t x) {   // bits [0, x), x in 0 .. 64
  return x >= 64u ? ~0ull : (1ull << x) - 1ull;
}
// bits of the chunk at entries [e0, e0 + 64) that lie in the entry range [a, b)
DWX_DEV unsigned long long diag_range(uint32_t e0, uint32_t a, uint32_t b) {
  const uint32_t lo = a > e0 ? (a - e0 > 64u ? 64u : a - e0) : 0u;
  const uint32_t hi = b > e0 ? (b - e0 > 64u ? 64u : b - e0) : 0u;
  return diag_below(hi) & ~diag_below(lo);
}

DWX_DEV void diag_init(DiagStats &st) {
#pragma unroll
  for (uint32_t t = 0; t <= DIAG_MAX_LAG; ++t) st.c[t] = 0;
  st.k = st.k1 = st.k2 = 0;
  st.first = st.last = st.prev = 0;
}

// the chunk `cur` of entries [e0, e0 + 64) (bits at entries >= n are zero), chunks in order
DWX_DEV void diag_accumulate(DiagStats &st, unsigned long long cur, uint32_t e0, uint32_t n) {
  const unsigned long long prev = st.prev;
  const uint32_t h = n / 2u;
  st.c[0] += (uint32_t)__builtin_popcountll(cur);          // (x * x = x)
#pragma unroll
  for (uint32_t t = 1; t < 64u; ++t)
    st.c[t] += (uint32_t)__builtin_popcountll(cur & ((cur << t) | (prev >> (64u - t))));
  st.c[64] += (uint32_t)__builtin_popcountll(cur & prev);   // (a shift by 64 is undefined: its own expression)
  st.k += (uint32_t)__builtin_popcountll(cur);
  st.k1 += (uint32_t)__builtin_popcountll(cur & diag_range(e0, 0u, h));
  st.k2 += (uint32_t)__builtin_popcountll(cur & diag_range(e0, n - h, n));
  if (e0 == 0u) st.first = cur;
  if (e0 + 64u >= n) {                                      // the last chunk: nb of its bits are entries
    const uint32_t nb = n - e0;
    st.last = nb >= 64u ? cur : (cur << (64u - nb)) | (prev >> nb);
  }
  st.prev = cur;
}

// rho_t of include/dwx.h; T a compile-time lag, so that c[] stays in registers
template <uint32_t T>
DWX_DEV double diag_rho(const DiagStats &st, double nd, double m, double W, double var_plus) {
  const uint32_t tail = T == 0u ? 0u : (uint32_t)__builtin_popcountll(st.last >> (64u - (T == 0u ? 1u : T)));
  const uint32_t head = T == 0u ? 0u : (uint32_t)__builtin_popcountll(st.first & diag_below(T));
  const double H = (double)(st.k - tail), Tt = (double)(st.k - head);
  const double a = ((double)st.c[T] - m * (H + Tt) + (nd - (double)T) * (m * m)) / nd;
  return 1.0 - (W - a) / var_plus;
}

// Geyer's pairs from lag T on, while the sum goes on (include/dwx.h: the loop of diagnostics.ess, cut at max_lag)
template <uint32_t T>
struct DiagPairs {
  static DWX_DEV void run(const DiagStats &st, uint32_t n, uint32_t max_lag, double nd, double m, double W,
                          double var_plus, double &s, uint32_t &t_end, bool &truncated) {
    if (T + 1u >= n) return;
    if (T + 1u > max_lag) { truncated = true; return; }
    const double pair = diag_rho<T>(st, nd, m, W, var_plus) + diag_rho<T + 1u>(st, nd, m, W, var_plus);
    if (!(pair > 0.0)) return;
    s += pair;
    t_end = T + 2u;
    DiagPairs<T + 2u>::run(st, n, max_lag, nd, m, W, var_plus, s, t_end, truncated);
  }
};
template <>
struct DiagPairs<DIAG_MAX_LAG> {   // (lag 65 is beyond every max_lag)
  static DWX_DEV void run(const DiagStats &, uint32_t n, uint32_t, double, double, double, double, double &, uint32_t &,
                          bool &truncated) {
    if (DIAG_MAX_LAG + 1u < n) truncated = true;
  }
};

// The formulas of include/dwx.h over a row's statistics, in f64 as written there (-ffp-contract=off).
DWX_DEV void diag_finish(const DiagStats &st, uint32_t n, uint32_t max_lag, double &rhat, double &ess, uint32_t &flags) {
  const double nd = (double)n, hd = (double)(n / 2u);
  const double k = (double)st.k, k1 = (double)st.k1, k2 = (double)st.k2;
  // split-R-hat: IEEE arithmetic decides 0 / 0 = nan (constant, equal halves) and B / 0 = inf (constant, different)
  const double var1 = (k1 - k1 * k1 / hd) / (hd - 1.0), var2 = (k2 - k2 * k2 / hd) / (hd - 1.0);
  const double Ws = (var1 + var2) / 2.0;
  const double dm = k1 / hd - k2 / hd;
  const double B = dm * dm / 2.0;
  rhat = sqrt(((hd - 1.0) / hd * Ws + B) / Ws);
  flags = 0;
  if (st.k == 0u || st.k == n) {
    flags = DIAG_FLAG_CONSTANT;
    ess = __builtin_nan("");
    return;
  }
  const double m = k / nd;
  const double W = (k - k * k / nd) / (nd - 1.0), var_plus = (k - k * k / nd) / nd;
  double s = 0.0;
  uint32_t t_end = 0;
  bool truncated = false;
  DiagPairs<0>::run(st, n, max_lag, nd, m, W, var_plus, s, t_end, truncated);
  const double tau = t_end ? 1.0 + 2.0 * (s - diag_rho<0>(st, nd, m, W, var_plus)) : 1.0;
  ess = nd / tau;
  if (truncated) flags |= DIAG_FLAG_TRUNCATED;
}

// a is a better candidate than b for the maximum (MAX) / minimum; rows DIAG_NO_ROW hold no value
template <bool MAX>
DWX_DEV bool diag_better(double a, uint32_t ra, double b, uint32_t rb) {
  if (ra == DIAG_NO_ROW) return false;
  if (rb == DIAG_NO_ROW) return true;
  return MAX ? a > b : a < b;
}

// A row's results out (device row order; each array may be null) and into the summary: counts[0 .. 3] =
// finite, constant, truncated, above the threshold -- integer atomics, one per wave and count; the extremes
// through an LDS tree into partials[blockIdx.x].  Every thread of the workgroup calls it (has: the lane holds a row).
template <uint32_t THREADS>
DWX_DEV void diag_emit(bool has, uint32_t row, double rhat, double ess, uint32_t flags, double rhat_threshold,
                       double *out_rhat, double *out_ess, unsigned char *out_flags, unsigned long long *counts,
                       DiagPartial *partials) {
  __shared__ double s_max[THREADS], s_min[THREADS];
  __shared__ uint32_t s_maxr[THREADS], s_minr[THREADS];
  const uint32_t t = threadIdx.x;
  if (has) {
    if (out_rhat) out_rhat[row] = rhat;
    if (out_ess) out_ess[row] = ess;
    if (out_flags) out_flags[row] = (unsigned char)flags;
  }
  const bool rnan = rhat != rhat, enan = ess != ess;
  const bool preds[4] = {has && !rnan && rhat - rhat == 0.0, has && (flags & DIAG_FLAG_CONSTANT) != 0u,
                         has && (flags & DIAG_FLAG_TRUNCATED) != 0u, has && rhat > rhat_threshold};
#pragma unroll
  for (uint32_t i = 0; i < 4u; ++i) {
    const unsigned long long m = DWX_BALLOT(preds[i]);
    if ((t & 63u) == 0u && m) atomicAdd(&counts[i], (unsigned long long)__builtin_popcountll(m));
  }
  s_max[t] = rhat; s_maxr[t] = has && !rnan ? row : DIAG_NO_ROW;
  s_min[t] = ess; s_minr[t] = has && !enan ? row : DIAG_NO_ROW;
  __syncthreads();
  for (uint32_t half = THREADS / 2u; half >= 1u; half >>= 1) {
    if (t < half) {
      if (diag_better<true>(s_max[t + half], s_maxr[t + half], s_max[t], s_maxr[t])) {
        s_max[t] = s_max[t + half]; s_maxr[t] = s_maxr[t + half];
      }
      if (diag_better<false>(s_min[t + half], s_minr[t + half], s_min[t], s_minr[t])) {
        s_min[t] = s_min[t + half]; s_minr[t] = s_minr[t + half];
      }
    }
    __syncthreads();
  }
  if (t == 0u) {
    DiagPartial p;
    p.max_rhat = s_max[0]; p.max_row = s_maxr[0];
    p.min_ess = s_min[0]; p.min_row = s_minr[0];
    partials[blockIdx.x] = p;
  }
}

// BITS = 1 (all-boolean graph: position p is bit p & 63 of word p >> 6 of a plane, one value row per position).
// Workgroup b, wave w owns word column b * 16 + w -- the 16 waves of a workgroup consume 128 adjacent bytes of
// every plane together: one 128-byte line where slot * words is a multiple of 16, else parts of two lines (a plane's
// stride is words * 8 bytes, unpadded), whose other parts the neighbouring workgroup reads -- and walks the entries
// 64 at a time: lane l loads the column's word of
// entry e0 + l, 64 ballots of (word >> j) & 1 hand lane j the 64-entry chunk of position column * 64 + j.
// (Geyer's pairs reach lag 63 at the most -- the pair (64, 65) is beyond max_lag -- so c[64] is summed, not read.)
// Chronological entry e lives in plane (slot0 + e) mod cap.  Grid: ceil(words / 16) workgroups of DIAG_BIT_THREADS.
// BITS = 8 (a byte per position): a lane per value ROW, workgroup b the rows [b * 256, b * 256 + 256), whose
// positions are consecutive; a tile of 64 entries x those positions is staged in LDS with coalesced loads and
// lane builds its row's chunk as the (byte == d) bits, d = 1 for a boolean variable's one row.
// Grid: ceil(R / 256) workgroups of DIAG_BYTE_THREADS.
template <int BITS>
__global__ void __launch_bounds__(BITS == 1 ? DIAG_BIT_THREADS : DIAG_BYTE_THREADS)
trace_diag_kernel(const unsigned long long *ring, uint32_t words, uint32_t cap, uint32_t slot0, uint32_t n,
                  uint32_t n_pos, uint32_t n_rows, const uint32_t *v_row, const uint32_t *v_meta, uint32_t max_lag,
                  double rhat_threshold, double *out_rhat, double *out_ess, unsigned char *out_flags,
                  unsigned long long *counts, DiagPartial *partials) {
  DiagStats st;
  diag_init(st);
  bool has;
  uint32_t row = 0;
  if constexpr (BITS == 1) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t col = blockIdx.x * (DIAG_BIT_THREADS / 64u) + (threadIdx.x >> 6);
    const uint32_t p = col * 64u + lane;
    const bool col_ok = col < words;
    has = col_ok && p < n_pos;
    if (has) row = v_row[p];
    for (uint32_t e0 = 0; e0 < n; e0 += 64u) {   // (n is the same for every thread: whole workgroups ballot together)
      unsigned long long w = 0;
      if (col_ok && e0 + lane < n) {
        uint32_t slot = slot0 + e0 + lane;       // (slot0 < cap, e0 + lane < n <= cap: one wrap at the most)
        if (slot >= cap) slot -= cap;
        w = ring[(size_t)slot * words + col];
      }
      unsigned long long cur = 0;
#pragma unroll
      for (uint32_t j = 0; j < 64u; ++j) {
        const unsigned long long m = DWX_BALLOT(((w >> j) & 1ull) != 0ull);
        if (lane == j) cur = m;
      }
      diag_accumulate(st, cur, e0, n);
    }
  } else {
    __shared__ unsigned char tile[64u * DIAG_BYTE_THREADS];
    __shared__ uint32_t s_pos[2];
    const uint32_t t = threadIdx.x;
    const uint32_t r = blockIdx.x * DIAG_BYTE_THREADS + t;
    has = r < n_rows;
    row = r;
    // the row's position: the last p with v_row[p] <= r
    uint32_t p = 0, target = 0;
    if (has) {
      uint32_t lo = 0, hi = n_pos;               // v_row[lo] <= r < v_row[hi]
      while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (v_row[mid] <= r) lo = mid; else hi = mid;
      }
      p = lo;
      target = (v_meta[p] & VM_CATEGORICAL) ? r - v_row[p] : 1u;
    }
    const uint32_t last_row = (n_rows - blockIdx.x * DIAG_BYTE_THREADS < DIAG_BYTE_THREADS ? n_rows - blockIdx.x * DIAG_BYTE_THREADS
                                                                                            : DIAG_BYTE_THREADS) - 1u;
    if (t == 0u) s_pos[0] = p;
    if (t == last_row) s_pos[1] = p;
    __syncthreads();
    const uint32_t p_first = s_pos[0], width = s_pos[1] - s_pos[0] + 1u;   // width <= 256: every position has a row
    for (uint32_t e0 = 0; e0 < n; e0 += 64u) {
      const uint32_t ne = n - e0 < 64u ? n - e0 : 64u;
      __syncthreads();                            // (the tile's last readers)
      for (uint32_t i = t; i < ne * width; i += DIAG_BYTE_THREADS) {
        const uint32_t e = i / width, x = i - e * width;
        uint32_t slot = slot0 + e0 + e;
        if (slot >= cap) slot -= cap;
        tile[e * DIAG_BYTE_THREADS + x] = ((const unsigned char *)(ring + (size_t)slot * words))[p_first + x];
      }
      __syncthreads();
      unsigned long long cur = 0;
      if (has)
        for (uint32_t e = 0; e < ne; ++e)
          cur |= (unsigned long long)(tile[e * DIAG_BYTE_THREADS + (p - p_first)] == target) << e;
      diag_accumulate(st, cur, e0, n);
    }
  }
  double rhat = 0.0, ess = 0.0;
  uint32_t flags = 0;
  diag_finish(st, n, max_lag, rhat, ess, flags);
  diag_emit<BITS == 1 ? DIAG_BIT_THREADS : DIAG_BYTE_THREADS>(has, row, rhat, ess, flags, rhat_threshold, out_rhat,
                                                              out_ess, out_flags, counts, partials);
}

// the workgroups' candidates folded into partials[0]: ONE workgroup of BLOCK_THREADS
__global__ void __launch_bounds__(BLOCK_THREADS)
trace_diag_fold_kernel(DiagPartial *partials, uint32_t n_partials) {
  __shared__ DiagPartial s_p[BLOCK_THREADS];
  const uint32_t t = threadIdx.x;
  DiagPartial best;
  best.max_rhat = best.min_ess = 0.0;
  best.max_row = best.min_row = DIAG_NO_ROW;
  for (uint32_t i = t; i < n_partials; i += BLOCK_THREADS) {
    const DiagPartial q = partials[i];
    if (diag_better<true>(q.max_rhat, q.max_row, best.max_rhat, best.max_row)) { best.max_rhat = q.max_rhat; best.max_row = q.max_row; }
    if (diag_better<false>(q.min_ess, q.min_row, best.min_ess, best.min_row)) { best.min_ess = q.min_ess; best.min_row = q.min_row; }
  }
  s_p[t] = best;
  __syncthreads();
  for (uint32_t half = BLOCK_THREADS / 2u; half >= 1u; half >>= 1) {
    if (t < half) {
      const DiagPartial q = s_p[t + half];
      if (diag_better<true>(q.max_rhat, q.max_row, s_p[t].max_rhat, s_p[t].max_row)) { s_p[t].max_rhat = q.max_rhat; s_p[t].max_row = q.max_row; }
      if (diag_better<false>(q.min_ess, q.min_row, s_p[t].min_ess, s_p[t].min_row)) { s_p[t].min_ess = q.min_ess; s_p[t].min_row = q.min_row; }
    }
    __syncthreads();
  }
  if (t == 0u) partials[0] = s_p[0];
}

}  // namespace dwx
#endif  // DWX_DIAG_KERNELS_H_
