// aux_kernels.h -- the kernels around the sweep: pull gradient (list and block form), apply
// (update_weight), terms tables, weight refresh / averaging, halo pack / unpack, test hooks.
// Part of sweep_kernels.h.
#ifndef DWX_AUX_KERNELS_H_
#define DWX_AUX_KERNELS_H_

#include "../../include/dwx.h"   // (DWX_WAVE_OP_*: the test hook's op codes)
#include "tile_walk.h"

namespace dwx {

// Pull-based weight gradient for TILE_PULL tiles (replaces their gradient atomics).
// inc_* is the incidence list of every (triggering boolean variable, non-fixed record)
// pair, SORTED BY WEIGHT: inc_wid[i], inc_slot[i] = tile * 256 + lane of the owning
// variable, inc_d[i] = sign(hit)*f - sign(miss)*f of the record (f32-exact).  The
// record's gradient is delta(owner) * inc_d, delta in {-1, 0, +1} read from the ballot
// bit-planes the sweep wrote (2 bits per variable: L2-resident).  A workgroup stages
// 256 * PULL_RUN entries' contributions in LDS (coalesced loads), then every lane sums its
// PULL_RUN consecutive entries and flushes one atomic per weight run -- neighbouring
// lanes hit neighbouring weights.  Integer sums: the result is independent of the order
// and identical to what the per-record atomics would have produced.
struct alignas(16) DeltaPair { unsigned long long nz, ng; };
struct alignas(16) F32x4 { float v[4]; };

// One lane owns PULL_RUN consecutive entries (a multiple of 4: 16-byte loads straight
// from HBM; a wave covers one contiguous 4 KiB span per array, every line is consumed
// fully across the lane's loads), gathers their owners' bits (one 16-byte L2 hit each,
// all in flight), sums per weight run in registers and flushes one atomic per run.
// No LDS, no barrier.
// SEG: weights own long stretches of the list (host: entries per weight >= 8) -- the lanes' last
// runs are summed per weight across the wave before the atomic; else every lane flushes its own.
template <bool SEG>
__global__ void __launch_bounds__(BLOCK_THREADS)
pull_grad_kernel(const uint32_t *inc_wid, const uint32_t *inc_slot, const float *inc_d,
                 uint32_t n, const unsigned long long *delta, long long *grad) {
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t n_runs = (n + PULL_RUN - 1) / PULL_RUN;   // arrays are padded to a full run
  const uint32_t lane = threadIdx.x & 63u;
  // (whole waves stay in the loop: the lanes meet in a wave-wide sum at its end)
  for (uint32_t r0 = (blockIdx.x * blockDim.x + threadIdx.x) - lane; r0 < n_runs; r0 += stride) {
    const bool valid = r0 + lane < n_runs;
    const uint32_t i0 = (valid ? r0 + lane : n_runs - 1) * PULL_RUN;
    uint32_t key[PULL_RUN], slot[PULL_RUN];
    float dd[PULL_RUN];
#pragma unroll
    for (uint32_t k = 0; k < PULL_RUN / 4; ++k) {
      const U32x4 a = ((const U32x4 *)(inc_wid + i0))[k];
      const U32x4 b = ((const U32x4 *)(inc_slot + i0))[k];
      const F32x4 c = ((const F32x4 *)(inc_d + i0))[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) { key[4 * k + j] = a.v[j]; slot[4 * k + j] = b.v[j]; dd[4 * k + j] = c.v[j]; }
    }
    DeltaPair dp[PULL_RUN];
#pragma unroll
    for (uint32_t k = 0; k < PULL_RUN; ++k) dp[k] = ((const DeltaPair *)delta)[slot[k] >> 6];
    uint32_t cur = key[0];
    long long acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < PULL_RUN; ++k) {
      const unsigned long long bit = 1ull << (slot[k] & 63u);
      long long v = 0;
      if (dp[k].nz & bit) {
        const long long q = llrint(FIX_SCALE * (double)dd[k]);
        v = (dp[k].ng & bit) ? -q : q;
      }
      if (key[k] != cur) {
        if (acc && valid) atomicAdd((unsigned long long *)&grad[cur], (unsigned long long)acc);
        cur = key[k];
        acc = v;
      } else {
        acc += v;
      }
    }
    // The lane's last weight run usually continues in the next lanes (a heavily tied weight
    // spans hundreds of lanes): one atomic per weight and WAVE instead of one per lane -- with
    // 10^3-10^4 weights the per-lane atomics queued up on a few thousand addresses.
    if (SEG) {
      bool head;
      const long long total = DWX_WAVE_SEG_SUM_I64(valid ? cur : 0xFFFFFFFFu, valid ? acc : 0ll, head);
      if (head && total) atomicAdd((unsigned long long *)&grad[cur], (unsigned long long)total);
    } else if (acc && valid) {
      atomicAdd((unsigned long long *)&grad[cur], (unsigned long long)acc);
    }
  }
}

// Block pull: the same sums as pull_grad_kernel without its random L2 gathers and with no
// atomics at all.  The owners of the incidence entries are cut into blocks of <= BP_TILES
// consecutive tiles whose ballot pairs (128 KiB) fit LDS; ell holds, per block and weight,
// BP_ROW * DEPTH entries (host: build_level; what does not fit a row stays on the list for
// fold_partials_kernel).  Workgroup (block b, part p) copies b's ballots into LDS once, then
// streams its share of b's rows -- coalesced 16-byte loads, independent iterations, no
// barrier -- and stores one partial sum per weight; fold_partials_kernel adds the blocks'
// partials into grad.  Integer sums: the result equals pull_grad_kernel's.

// UNIFORM: every record delta of the graph is the same (one feature value, one factor
// function -- the usual case): its step comes in as an argument instead of an LDS table.
// PACKED (with UNIFORM; the builders' form of such tables): a row is DEPTH planes of 8-byte words of three
// 19-bit slots and a count (device_types.h: bp_pack_entry) -- 8 bytes per three entries instead of 16 per four.
template <int DEPTH, bool UNIFORM, bool PACKED = false>
__global__ void __launch_bounds__(BP_THREADS)
pull_ell_kernel(const U32x4 *__restrict__ ell, const uint32_t *block_tile0, uint32_t parts, const long long *qtab,
                uint32_t n_deltas, uint32_t Wp, const unsigned long long *delta, long long *__restrict__ partial) {
  DWX_DYN_LDS(dyn_lds);
  DeltaPair *s_delta = (DeltaPair *)dyn_lds;
  constexpr uint32_t PAIRS = BP_TILES * 4;                 // ballot pairs per block
  // the deltas' fixed-point steps live in LDS too (a dependent global load inside the loop
  // would wait for every load issued before it: vmcnt retires in order)
  long long *s_q = (long long *)(dyn_lds + PAIRS * sizeof(DeltaPair));
  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x / parts, part = blockIdx.x % parts;
  const DeltaPair *src = (const DeltaPair *)delta + (size_t)block_tile0[b] * 4;   // (padded allocation)
  for (uint32_t i = tid; i < PAIRS; i += BP_THREADS) s_delta[i] = src[i];
  if (!UNIFORM)
    for (uint32_t i = tid; i < BP_DELTA_SLOTS; i += BP_THREADS) s_q[i] = i < n_deltas ? qtab[i] : 0;
  const long long q0 = qtab[0];
  const uint32_t *s_words = (const uint32_t *)s_delta;
  __syncthreads();
  // this part's weights: whole groups of BP_THREADS
  const uint32_t groups = Wp / BP_THREADS, per = (groups + parts - 1) / parts;
  const uint32_t g0 = part * per, g1 = g0 + per < groups ? g0 + per : groups;
  const U32x4 *__restrict__ rows = ell + (size_t)b * DEPTH * Wp;
  long long *__restrict__ out = partial + (size_t)b * Wp;
  // UNIFORM: one BYTE per (block, weight) -- the count of +1 / -1 steps; fold_partials_kernel multiplies
  // (an eighth of the partial sums' traffic: 160 MB written and read again per sweep on config 3)
  signed char *__restrict__ out8 = (signed char *)partial + (size_t)b * Wp;
  // BP_UNROLL groups per step: all their row loads are issued before the first is used (the
  // compiler does not hoist them over the stores on its own); past the end the last group is
  // loaded again and not stored
  if constexpr (PACKED) {
    static_assert(UNIFORM, "packed rows carry no delta index");
    const unsigned long long *__restrict__ rows8 = (const unsigned long long *)ell + (size_t)b * DEPTH * Wp;
    for (uint32_t g = g0; g < g1; g += BP_UNROLL) {
      unsigned long long row[BP_UNROLL][DEPTH];
#pragma unroll
      for (uint32_t u = 0; u < BP_UNROLL; ++u) {
        const uint32_t w = umin(g + u, g1 - 1) * BP_THREADS + tid;
#pragma unroll
        for (int dd = 0; dd < DEPTH; ++dd) row[u][dd] = DWX_NT_LOAD(&rows8[(size_t)dd * Wp + w]);
      }
#pragma unroll
      for (uint32_t u = 0; u < BP_UNROLL; ++u) {
        int cnt = 0;   // (at most BP_PK_ROW * DEPTH entries: a byte)
#pragma unroll
        for (int dd = 0; dd < DEPTH; ++dd) {
          const unsigned long long e = row[u][dd];
          const uint32_t n = (uint32_t)(e >> BP_PK_COUNT_SHIFT) & 3u;
#pragma unroll
          for (uint32_t k = 0; k < BP_PK_ROW; ++k) {
            // branch-free, as below: an unused slot reads the bits of slot 0 and adds zero
            const uint32_t slot = (uint32_t)(e >> (BP_SLOT_BITS * k)) & BP_SLOT_MASK;
            const uint32_t word = (slot >> 6) * 4u + ((slot >> 5) & 1u);
            const uint32_t nzw = s_words[word], ngw = s_words[word + 2u];
            const uint32_t nz = (nzw >> (slot & 31u)) & (k < n ? 1u : 0u), ng = (ngw >> (slot & 31u)) & 1u;
            cnt += nz ? (ng ? -1 : 1) : 0;
          }
        }
        if (g + u < g1) DWX_NT_STORE((signed char)cnt, &out8[(g + u) * BP_THREADS + tid]);
      }
    }
    return;
  }
  for (uint32_t g = g0; g < g1; g += BP_UNROLL) {
    U32x4 row[BP_UNROLL][DEPTH];
#pragma unroll
    for (uint32_t u = 0; u < BP_UNROLL; ++u) {
      const uint32_t w = umin(g + u, g1 - 1) * BP_THREADS + tid;
#pragma unroll
      for (int dd = 0; dd < DEPTH; ++dd) row[u][dd] = DWX_LOAD_ROW_NT(&rows[(size_t)dd * Wp + w]);
    }
#pragma unroll
    for (uint32_t u = 0; u < BP_UNROLL; ++u) {
      long long acc = 0;
      int cnt = 0;   // UNIFORM: the sum in units of the one step (at most BP_ROW * DEPTH entries: a byte)
#pragma unroll
      for (int dd = 0; dd < DEPTH; ++dd) {
#pragma unroll
        for (uint32_t k = 0; k < BP_ROW; ++k) {
          // branch-free: an empty entry decodes to the block's last slot and adds zero.
          // Only the two 32-bit words that hold the owner's bits are read (a ballot pair is
          // {nz lo, nz hi, ng lo, ng hi}), and no step table when all deltas are equal.
          const uint32_t e = row[u][dd].v[k];
          const uint32_t slot = e & BP_SLOT_MASK;
          const uint32_t word = (slot >> 6) * 4u + ((slot >> 5) & 1u);
          const uint32_t nzw = s_words[word], ngw = s_words[word + 2u];
          const long long q = UNIFORM ? q0 : s_q[(e >> BP_SLOT_BITS) & (BP_DELTA_SLOTS - 1)];
          const uint32_t nz = (nzw >> (slot & 31u)) & (e != BP_EMPTY ? 1u : 0u), ng = (ngw >> (slot & 31u)) & 1u;
          if (UNIFORM) {
            cnt += nz ? (ng ? -1 : 1) : 0;
          } else {
            const long long t = ng ? -q : q;
            acc += nz ? t : 0;
          }
        }
      }
      if (g + u < g1) {
        if (UNIFORM) DWX_NT_STORE((signed char)cnt, &out8[(g + u) * BP_THREADS + tid]);
        else DWX_NT_STORE(acc, &out[(g + u) * BP_THREADS + tid]);
      }
    }
  }
}

// One-plane packed rows (device_types.h: bp1_pack_entry; the builders' form of a one-delta table whose owners
// are all boolean evidence variables): an entry's sign is in its row, so only the nz words of the block's ballot
// pairs go to LDS -- as 8-byte words, pair i of the block at s_nz[i]; the pairs lie 16 bytes apart in `delta` --
// and a slot costs one 32-bit LDS read.  A block holds up to BP1_TILES tiles (`tiles`: the table's block size;
// the allocation of `delta` is padded by one full block).  The byte partials are those of
// pull_ell_kernel<DEPTH, true, true>: fold_partials_kernel<true> consumes them alike.
template <int DEPTH>
__global__ void __launch_bounds__(BP_THREADS)
pull_ell1_kernel(const unsigned long long *__restrict__ ell, const uint32_t *block_tile0, uint32_t parts, uint32_t tiles,
                 uint32_t Wp, const unsigned long long *delta, signed char *__restrict__ partial) {
  DWX_DYN_LDS(dyn_lds);
  unsigned long long *s_nz = (unsigned long long *)dyn_lds;
  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x / parts, part = blockIdx.x % parts;
  const DeltaPair *src = (const DeltaPair *)delta + (size_t)block_tile0[b] * 4;   // (padded allocation)
  const uint32_t pairs = umin(tiles, BP1_TILES) * 4u;
  for (uint32_t i = tid; i < pairs; i += BP_THREADS) s_nz[i] = src[i].nz;
  const uint32_t *s_words = (const uint32_t *)s_nz;
  __syncthreads();
  // A lane owns TWO consecutive weights: one 16-byte load per plane takes both words (the planes are [Wp], Wp a
  // multiple of BP_THREADS: 16-byte aligned at an even weight), and their two byte counts leave as one 16-bit
  // store.  This part's weights: whole groups of 2 * BP_THREADS; the last group of the table may be half a one.
  static_assert(BP_UNROLL % 2 == 0, "two weights per lane");
  constexpr uint32_t U2 = BP_UNROLL / 2, GROUP = 2 * BP_THREADS;
  const uint32_t groups = (Wp + GROUP - 1) / GROUP, per = (groups + parts - 1) / parts;
  const uint32_t g0 = part * per, g1 = g0 + per < groups ? g0 + per : groups;
  const unsigned long long *__restrict__ rows8 = ell + (size_t)b * DEPTH * Wp;
  signed char *__restrict__ out8 = partial + (size_t)b * Wp;
  for (uint32_t g = g0; g < g1; g += U2) {
    U32x4 row[U2][DEPTH];
#pragma unroll
    for (uint32_t u = 0; u < U2; ++u) {
      const uint32_t w = umin(umin(g + u, g1 - 1) * GROUP + 2u * tid, Wp - 2u);   // (past the end: loaded again, not stored)
#pragma unroll
      for (int dd = 0; dd < DEPTH; ++dd) row[u][dd] = DWX_LOAD_ROW_NT((const U32x4 *)&rows8[(size_t)dd * Wp + w]);
    }
#pragma unroll
    for (uint32_t u = 0; u < U2; ++u) {
      int cnt[2] = {0, 0};   // (at most BP_PK_ROW * DEPTH entries each: a byte)
#pragma unroll
      for (int dd = 0; dd < DEPTH; ++dd) {
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          const uint32_t lo = row[u][dd].v[2 * h], hi = row[u][dd].v[2 * h + 1];
          const unsigned long long e = ((unsigned long long)hi << 32) | lo;
          const uint32_t n = (hi >> (BP1_COUNT_SHIFT - 32)) & 3u, npos = hi >> (BP1_NPOS_SHIFT - 32);
#pragma unroll
          for (uint32_t k = 0; k < BP_PK_ROW; ++k) {
            // branch-free: an unused slot reads the bit of slot 0 and adds zero
            const uint32_t slot = (uint32_t)(e >> (BP1_SLOT_BITS * k)) & BP1_SLOT_MASK;
            const int bit = (int)((s_words[slot >> 5] >> (slot & 31u)) & 1u);
            cnt[h] += k < n ? (k < npos ? bit : -bit) : 0;
          }
        }
      }
      const uint32_t w = (g + u) * GROUP + 2u * tid;
      if (g + u < g1 && w < Wp)
        DWX_NT_STORE((unsigned short)(((uint32_t)cnt[0] & 255u) | (((uint32_t)cnt[1] & 255u) << 8)), (unsigned short *)&out8[w]);
    }
  }
}

// grad[w] += sum over blocks of partial[block][w]  (UNIFORM: byte counts of the one step q0), plus the
// entries that did not fit the blocks' rows: they stay on the weight-sorted list, weight w's at
// [ov_start[w], ov_start[w + 1]) of inc_slot / inc_d (ov_start == nullptr: none), and the lane that owns
// the weight adds them -- the owner's bits from the global ballot planes, the same step as
// pull_grad_kernel -- so no atomic and no launch of its own is spent on them.  A lane owns FOLD_W
// consecutive weights: the byte partials come as one 32-bit load per block, the lane's leftovers are
// one contiguous stretch of the list, walked FOLD_W entries at a time with their gathers in flight together.
// Integer sums: the result equals pull_grad_kernel's.
template <bool UNIFORM>
__global__ void __launch_bounds__(BLOCK_THREADS)
fold_partials_kernel(const long long *partial, uint32_t n_blocks, uint32_t Wp, uint32_t W, long long *grad,
                     const long long *qtab, const uint32_t *ov_start, const uint32_t *inc_slot, const float *inc_d,
                     const unsigned long long *delta) {
  static_assert(FOLD_W == 4, "the byte partials of a lane's weights are one 32-bit word");
  const uint32_t stride = gridDim.x * blockDim.x * FOLD_W;
  const long long q0 = qtab[0];
  for (uint32_t w0 = (blockIdx.x * blockDim.x + threadIdx.x) * FOLD_W; w0 < W; w0 += stride) {
    long long acc[FOLD_W];
    if (UNIFORM) {
      int cnt[FOLD_W] = {0, 0, 0, 0};
      for (uint32_t b = 0; b < n_blocks; ++b) {   // (w0 + 3 < Wp, a multiple of BP_THREADS: the word is inside the row)
        const uint32_t x = *(const uint32_t *)((const signed char *)partial + (size_t)b * Wp + w0);
#pragma unroll
        for (uint32_t j = 0; j < FOLD_W; ++j) cnt[j] += (int)(signed char)(x >> (8u * j));
      }
#pragma unroll
      for (uint32_t j = 0; j < FOLD_W; ++j) acc[j] = (long long)cnt[j] * q0;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < FOLD_W; ++j) acc[j] = 0;
      for (uint32_t b = 0; b < n_blocks; ++b) {
#pragma unroll
        for (uint32_t j = 0; j < FOLD_W; ++j) acc[j] += partial[(size_t)b * Wp + w0 + j];
      }
    }
    if (ov_start) {
      uint32_t at[FOLD_W + 1];   // (ov_start has W + 1 entries; weights past W own nothing)
#pragma unroll
      for (uint32_t j = 0; j <= FOLD_W; ++j) at[j] = ov_start[umin(w0 + j, W)];
      for (uint32_t i0 = at[0]; i0 < at[FOLD_W]; i0 += FOLD_W) {
        uint32_t slot[FOLD_W];
        float dd[FOLD_W];
        DeltaPair dp[FOLD_W];
#pragma unroll
        for (uint32_t k = 0; k < FOLD_W; ++k) {
          const uint32_t i = umin(i0 + k, at[FOLD_W] - 1);
          slot[k] = inc_slot[i];
          dd[k] = UNIFORM ? 0.0f : inc_d[i];
        }
#pragma unroll
        for (uint32_t k = 0; k < FOLD_W; ++k) dp[k] = ((const DeltaPair *)delta)[slot[k] >> 6];
#pragma unroll
        for (uint32_t k = 0; k < FOLD_W; ++k) {
          const uint32_t i = i0 + k;
          const unsigned long long bit = 1ull << (slot[k] & 63u);
          long long v = 0;
          if (i < at[FOLD_W] && (dp[k].nz & bit)) {
            const long long q = UNIFORM ? q0 : llrint(FIX_SCALE * (double)dd[k]);
            v = (dp[k].ng & bit) ? -q : q;
          }
#pragma unroll
          for (uint32_t j = 0; j < FOLD_W; ++j) acc[j] += (i >= at[j] && i < at[j + 1]) ? v : 0;
        }
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < FOLD_W; ++j)
      if (w0 + j < W && acc[j]) grad[w0 + j] += acc[j];
  }
}

// Batched InferenceResult::update_weight (src/inference_result.h:66-85): apply one
// mini-batch's accumulated gradient to every non-fixed weight that received updates, then
// clear the accumulators.  T = dynamic counts (atomics) + static counts (boolean variables,
// precomputed per chunk; null when the plan counts dynamically).
//
// The reference applies its T updates of a weight one after the other, each seeing the
// samples the previous ones already moved: over one batch the weight follows the flow
//   dw/dtau = -(G(w) + reg * T * w),  tau in [0, stepsize]
// and therefore never overshoots, however many factors share the weight.  One plain step
// w -= stepsize * (G + reg T w) does (it diverges once stepsize * curvature > 2).  So the
// batch is integrated instead: with G linearised around the current weight with slope h[w]
// (t_hess: the batch's Gershgorin curvature bound of this weight), the flow's
// end point is
//   w - s * (G + reg T w),   s = (1 - exp(-c stepsize)) / c,   c = h[w] + reg T.
// s -> stepsize for c stepsize << 1 (weights with few factors: the reference's own step, to
// first order w / (1 + reg stepsize)^T - stepsize G), s -> 1 / c for heavily tied weights
// (the flow has converged within the batch).
// Also refreshes the f32 sampling copy of each weight it changes.
DWX_DEV double saturating_step(double c, double stepsize) {
  return c > 0.0 ? -expm1(-c * stepsize) / c : stepsize;
}
// h is an upper BOUND of the batch's curvature; the reference's visits feel the true one,
// somewhere in [0, h].  While no step can overshoot anyway (s (h + r) <= 1: monotone approach
// whatever the truth) the flow is integrated with the middle of that interval, CURV_MID h --
// half the worst-case lag behind the reference in a transient -- and the step is capped at
// 1 / (h + r), the converged flow under the bound.  r = the exact part (L2 pull, reg T).
#ifndef DWX_CURV_MID
#define DWX_CURV_MID 0.5
#endif
DWX_DEV double batch_step(double h, double r, double stepsize) {
  const double s = saturating_step(DWX_CURV_MID * h + r, stepsize), cb = h + r;
  return s * cb > 1.0 ? 1.0 / cb : s;
}
// L1 (src/inference_result.h:76-78): every visit adds reg_param -- NOT scaled by the step --
// while the weight is negative, then takes the gradient step.  Over a batch of T visits that is
// the flow of a piecewise-linear field,
//   w < 0:   dw/dtau = P - G - h (w - w0),   P = reg_param T / stepsize
//   w >= 0:  dw/dtau =     - G - h (w - w0),                     tau in [0, stepsize]
// integrated piece by piece: the push STOPS at the zero crossing.  Where the two fields point
// at each other across zero (the gradient wants the weight negative, the push is stronger) the
// reference's weight rides a sawtooth around zero -- w <- w - d + reg_param [w < 0] with
// d = stepsize G(0) / T per visit, a rotation whose values fill [-d, reg_param - d) evenly; a
// batch that ends there ends at that sawtooth's mean, reg_param / 2 - d.
DWX_DEV double l1_flow(double w0, double G, double h, double T, double stepsize, double reg_param) {
  if (!(stepsize > 0.0)) return w0;
  const double P = reg_param * T / stepsize, hm = DWX_CURV_MID * h;
  double w = w0, left = stepsize;
  for (int piece = 0; piece < 3; ++piece) {
    const double aP = -G - hm * (w - w0), aN = aP + P;  // the two fields at w
    double a;
    if (w < 0.0 || (w == 0.0 && aN <= 0.0)) a = aN;
    else if (w > 0.0 || aP > 0.0) a = aP;
    else return 0.5 * reg_param + aP * stepsize / T;    // sliding: aN > 0 >= aP, d = -aP stepsize / T
    double phi = hm > 0.0 ? -expm1(-hm * left) / hm : left;
    if (phi * h > 1.0) phi = 1.0 / h;                   // as batch_step: never past the bound's fixed point
    const double end = w + a * phi;                     // dw/dtau = a - hm (w(tau) - w)
    if (w == 0.0 || (w < 0.0) == (end <= 0.0)) return end;   // no crossing: monotone towards its fixed point
    const double q = -w / a;                            // phi(tau_c): the flow reaches zero
    left -= hm > 0.0 ? -log1p(-hm * q) / hm : q;
    w = 0.0;
    if (!(left > 0.0)) return 0.0;
  }
  return w;
}
// Where the batch's curvature is negligible (h stepsize small: weights with few visits per batch --
// the untied weights of a DeepDive graph) the flow's "the push stops at zero" is NOT what the
// reference does: a visit's push is a jump of the whole reg_param (w = -0.001, one visit, no
// gradient: the reference lands on 0.009 and stays).  There the reference's own recurrence
//   w += reg_param [w < 0];  w -= stepsize g          (src/inference_result.h:76-78)
// is followed exactly over the batch's n = T visits with the batch's mean gradient per visit, in
// closed form: rise by reg - d per visit while negative, fall by d per visit while not, and once
// both have happened w <- w - d + reg [w < 0] is a rotation of x = w + d on [0, reg).  A batch that
// spans a whole period of that rotation ends at its mean (the visits' own noise decides the phase),
// a shorter one at the rotation's exact end point.  (T is real: truthiness-weighted.)
DWX_DEV double l1_visits(double w, double G, double T, double stepsize, double reg_param) {
  double n = T;
  const double d = stepsize * G / T, up = reg_param - d;
  if (w < 0.0) {
    if (!(up > 0.0)) return w + n * up;          // the gradient outweighs the push: it keeps falling
    const double k = ceil(-w / up);              // visits until it is >= 0
    if (k >= n) return w + n * up;
    w += k * up; n -= k;                         // in [0, up)
  }
  if (!(d > 0.0)) return w - n * d;              // nothing pulls it below zero again: no more pushes
  const double k = floor(w / d) + 1.0;           // visits until it is negative
  if (k > n) return w - n * d;
  w -= k * d; n -= k;                            // in [-d, 0)
  if (!(up > 0.0)) return w + n * up;
  if (n * d >= reg_param) return 0.5 * reg_param - d;
  double x = fmod(w + d - n * d, reg_param);
  if (x < 0.0) x += reg_param;
  return x - d;
}
// (curvature "negligible": the flow's step differs from the plain one by less than 1/32 of itself)
DWX_DEV double l1_update(double w0, double G, double h, double T, double stepsize, double reg_param) {
  return DWX_CURV_MID * h * stepsize <= 0.0625 ? l1_visits(w0, G, T, stepsize, reg_param)
                                               : l1_flow(w0, G, h, T, stepsize, reg_param);
}
// InferenceResult::update_weight (src/inference_result.h:66-85) for one weight over one batch:
// G, Td = the batch's fixed-point gradient sum and dynamic update count; returns the new value
// (x itself for a fixed weight or one nobody visited).
DWX_DEV double apply_value(double x, bool fixed, const long long *t_static, const long long *t_hess, uint32_t i,
                           long long G, long long Td, double stepsize, double reg_param, int l2) {
  const long long Tn = Td + (t_static ? t_static[i] : 0);
  if (fixed || Tn == 0) return x;
  const double Tt = (double)Tn / FIX_SCALE, Gg = (double)G / FIX_SCALE;
  const double h = t_hess ? (double)t_hess[i] / H_SCALE : 0.0;
  if (l2) return x - batch_step(h, reg_param * Tt, stepsize) * (Gg + reg_param * Tt * x);
  return l1_update(x, Gg, h, Tt, stepsize, reg_param);
}
DWX_DEV void apply_one(double *weights, float *w32, const uint8_t *w_fixed, const long long *t_static,
                       const long long *t_hess, uint32_t i, long long G, long long Td, double stepsize,
                       double reg_param, int l2) {
  const long long Tn = Td + (t_static ? t_static[i] : 0);
  if (w_fixed[i] || Tn == 0) return;
  const double x = apply_value(weights[i], false, t_static, t_hess, i, G, Td, stepsize, reg_param, l2);
  weights[i] = x;
  w32[i] = (float)x;
}
// w_in (the last update of a sweep whose mini-batches ran as merged launches, persist_kernels.h): the
// weights before this update live in another buffer -- every weight is written, touched or not;
// also_zero: a second gradient buffer to clear (the one the last merged launch read).
// w32_prev (the update after a sweep that deferred draws): every weight's f32 value as that sweep
// read it is saved there before the new one is written -- all W of them, touched or not.
__global__ void __launch_bounds__(BLOCK_THREADS)
apply_kernel(double *weights, float *w32, const uint8_t *w_fixed, long long *grad,
             const long long *t_static, const long long *t_hess, uint32_t W, double stepsize,
             double reg_param, int l2, const double *w_in = nullptr, long long *also_zero = nullptr,
             float *w32_prev = nullptr) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += stride) {
    if (w32_prev) w32_prev[i] = w32[i];
    const long long G = grad[i], Td = grad[W + i];
    if (G != 0 || Td != 0) { grad[i] = 0; grad[W + i] = 0; }
    if (also_zero) { also_zero[i] = 0; also_zero[W + i] = 0; }
    if (w_in) {
      const double x = apply_value(w_in[i], w_fixed[i] != 0, t_static, t_hess, i, G, Td, stepsize, reg_param, l2);
      weights[i] = x;
      w32[i] = (float)x;
    } else {
      apply_one(weights, w32, w_fixed, t_static, t_hess, i, G, Td, stepsize, reg_param, l2);
    }
  }
}

// Inference with unchanged weights repeats the same products sweep after sweep: tabulate
// them once.  For every pre-signed (unary) record, exactly the two terms the staging pass of
// sweep_kernel computes -- f64 products of two f32 values, exact -- in a stream with the
// records' own 16-byte stride; other records get zeros (their tiles never read the table).
// Inference sweeps then stream the table and touch no weight: the 50 M random L2 requests
// per sweep that bound config 3's inference are gone.
__global__ void __launch_bounds__(BLOCK_THREADS)
build_terms_kernel(const TileDesc *tiles, uint32_t n_tiles, const EdgeRec *edges, const float *w32,
                   EdgeTerms *terms) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const TileDesc d = tiles[tile];
    const bool simple = d.flags & TILE_SIMPLE, inline2 = d.flags & TILE_INLINE2;
    if (!simple && !inline2) continue;        // such tiles never read the table
    for (uint32_t i = threadIdx.x; i < d.nedges; i += BLOCK_THREADS) {
      const EdgeRec r = edges[d.e0 + i];
      const double wv = (double)w32[r.wid];
      if (simple) {
        EdgeTerms tt;
        tt.t1 = wv * (double)r.fval;
        tt.t0 = wv * (double)bits_to_float(r.aux);
        terms[d.e0 + i] = tt;
      } else {
        TabRec2 tr;
        if (r.packed & EDGE_PRESIGNED) {
          // hit / miss values are s * f with s in {-1, 0, +1}: one product, two small codes
          const float hit = r.fval, miss = bits_to_float(r.aux);
          const float ref = hit != 0.0f ? hit : miss;
          tr.wf = wv * (double)ref;
          const uint32_t c0 = miss == 0.0f ? 1u : (miss == ref ? 2u : 0u);
          tr.bits = (r.packed & EDGE_FUNC_MASK) | TAB2_UNARY | (hit != 0.0f ? TAB2_C1 : 0u) | (c0 << TAB2_C0_SHIFT);
          tr.other = d.v0 + edge_owner_lane(r);
        } else {
          tr.wf = wv * (double)r.fval;
          tr.bits = r.packed & (EDGE_FUNC_MASK | (EDGE_ARITY_MASK << EDGE_ARITY_SHIFT));
          tr.other = r.aux;
        }
        ((TabRec2 *)terms)[d.e0 + i] = tr;
      }
    }
  }
}

// The terms table of an all-unary graph (compact records): 8 bytes per record, the exact
// product w * f (f64 of two f32) with sign(hit) + 1 and sign(miss) + 1 in its four lowest
// mantissa bits -- zero in every such product, so nothing is lost.
__global__ void __launch_bounds__(BLOCK_THREADS)
build_terms8_kernel(const EdgeRec8 *edges8, uint64_t n, const float *w32, unsigned long long *terms) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const EdgeRec8 c = edges8[i];
    const double wf = (double)w32[c.key & REC8_WID_MASK] * (double)c.f;
    unsigned long long u;
    __builtin_memcpy(&u, &wf, 8);
    terms[i] = u | ((c.key >> REC8_HIT_SHIFT) & 15u);   // hit code in bits 0-1, miss code in bits 2-3
  }
}

// Multi-GPU, all-boolean all-unary graphs: every contribution to a gradient sum is a multiple of
// 2^shift (dwx_graph_info.grad_shift), so the sums travel through the all-reduce as 32-bit counts
// -- half the bytes -- and come back shifted.  `bad` is raised if a sum is not such a multiple or
// does not fit (it never is by construction; dwx_wait reports it).
__global__ void __launch_bounds__(BLOCK_THREADS)
grad_pack32_kernel(const long long *grad, int *out, uint32_t W, uint32_t shift, uint32_t *bad) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += stride) {
    const long long g = grad[i], v = g >> shift;
    // (inside (-2^31, 2^31), symmetric like the 16-bit form: -2^31 fits an int but not its own negation or a sum)
    if ((long long)((unsigned long long)v << shift) != g || v <= -2147483648ll || v >= 2147483648ll) atomicAdd(bad, 1u);
    out[i] = (int)v;
  }
}
__global__ void __launch_bounds__(BLOCK_THREADS)
grad_unpack32_kernel(const int *in, long long *grad, uint32_t W, uint32_t shift) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += stride)
    grad[i] = (long long)((unsigned long long)(long long)in[i] << shift);
}

// The same as 16-bit counts, two per 32-bit word (RCCL has no 16-bit integer type): word i =
// c[2i] + 65536 * c[2i + 1] as ARITHMETIC (a negative low count borrows from the high one), so that
// the all-reduce's plain 32-bit sums of the words ARE the packed sums of the counts as long as every
// summed count stays inside (-2^15, 2^15) -- what the ranks agreed on before choosing this form
// (sum over ranks of max_records_per_weight x grad_unit_max < 2^15).  A quarter of the int64 bytes.
__global__ void __launch_bounds__(BLOCK_THREADS)
grad_pack16_kernel(const long long *grad, int *out, uint32_t W, uint32_t shift, uint32_t *bad) {
  const uint32_t stride = gridDim.x * blockDim.x, words = (W + 1u) / 2u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const long long g0 = grad[2 * i], g1 = 2 * i + 1 < W ? grad[2 * i + 1] : 0;
    const long long v0 = g0 >> shift, v1 = g1 >> shift;
    if ((long long)((unsigned long long)v0 << shift) != g0 || (long long)((unsigned long long)v1 << shift) != g1 ||
        v0 <= -32768 || v0 >= 32768 || v1 <= -32768 || v1 >= 32768)
      atomicAdd(bad, 1u);
    out[i] = (int)(v0 + v1 * 65536);
  }
}
__global__ void __launch_bounds__(BLOCK_THREADS)
grad_unpack16_kernel(const int *in, long long *grad, uint32_t W, uint32_t shift) {
  const uint32_t stride = gridDim.x * blockDim.x, words = (W + 1u) / 2u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const int x = in[i];
    const int lo = (int)(short)(x & 0xFFFF);        // the low count, sign-extended
    const int hi = (x - lo) >> 16;                  // exact: x - lo is a multiple of 65536
    grad[2 * i] = (long long)((unsigned long long)(long long)lo << shift);
    if (2 * i + 1 < W) grad[2 * i + 1] = (long long)((unsigned long long)(long long)hi << shift);
  }
}

// f64 master weights -> f32 sampling copy (after dwx_set_weights)
__global__ void __launch_bounds__(BLOCK_THREADS)
refresh_w32_kernel(const double *weights, float *w32, uint32_t W) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += stride)
    w32[i] = (float)weights[i];
}

// Replica averaging (InferenceResult::average_weights + copy_weights_to,
// src/inference_result.cc:75-86): the caller summed the replicas' weights in place; divide
// by their number.  Fixed weights are put back verbatim (copy_weights_to skips them; a sum
// of n equal values divided by n need not round back for n = 3, 5, 6, 7).
__global__ void __launch_bounds__(BLOCK_THREADS)
average_weights_kernel(double *weights, float *w32, const uint8_t *w_fixed, const double *w_init,
                       uint32_t W, double n_replicas) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += stride) {
    const double w = w_fixed[i] ? w_init[i] : weights[i] / n_replicas;
    weights[i] = w;
    w32[i] = (float)w;
  }
}

// Halo exchange (multi-GPU, cross-shard factors): gather the listed variables' assignments of
// the selected chains into a contiguous buffer [chain][i] (what a peer receives), and the
// reverse for the ghosts.  pos = device positions; chains = bit 0 free, bit 1 evidence chain;
// the buffer holds the selected chains back to back.
// BITS per value: 32, 8 (every listed cardinality <= 256) or 1 (every listed variable boolean:
// a wave's 64 values are one ballot); block = 8-byte words per chain block.
template <int BITS>
__global__ void __launch_bounds__(BLOCK_THREADS)
halo_pack_kernel(const uint32_t *pos, uint32_t n, const uint32_t *assign_free, const uint32_t *assign_evid,
                 uint32_t chains, unsigned long long *buf, uint32_t block) {
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t n_round = (n + blockDim.x - 1) / blockDim.x * blockDim.x;   // (whole workgroups ballot together)
  unsigned long long *second = buf + ((chains & 1u) ? block : 0u);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += stride) {
    const uint32_t p = pos[i < n ? i : n - 1];
    const uint32_t vf = (chains & 1u) ? assign_free[p] : 0u, ve = (chains & 2u) ? assign_evid[p] : 0u;
    if (BITS == 1) {
      const unsigned long long mf = DWX_BALLOT(i < n && (vf & 1u)), me = DWX_BALLOT(i < n && (ve & 1u));
      if ((threadIdx.x & 63u) == 0 && i < n) {
        if (chains & 1u) buf[i >> 6] = mf;
        if (chains & 2u) second[i >> 6] = me;
      }
    } else if (i < n) {
      if (BITS == 8) {
        if (chains & 1u) ((unsigned char *)buf)[i] = (unsigned char)vf;
        if (chains & 2u) ((unsigned char *)second)[i] = (unsigned char)ve;
      } else {
        if (chains & 1u) ((uint32_t *)buf)[i] = vf;
        if (chains & 2u) ((uint32_t *)second)[i] = ve;
      }
    }
  }
}
template <int BITS>
__global__ void __launch_bounds__(BLOCK_THREADS)
halo_unpack_kernel(const uint32_t *pos, uint32_t n, uint32_t *assign_free, uint32_t *assign_evid,
                   uint32_t chains, const unsigned long long *buf, uint32_t block) {
  const uint32_t stride = gridDim.x * blockDim.x;
  const unsigned long long *second = buf + ((chains & 1u) ? block : 0u);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t p = pos[i];
    uint32_t vf = 0, ve = 0;
    if (BITS == 1) {
      if (chains & 1u) vf = (uint32_t)(buf[i >> 6] >> (i & 63u)) & 1u;
      if (chains & 2u) ve = (uint32_t)(second[i >> 6] >> (i & 63u)) & 1u;
    } else if (BITS == 8) {
      if (chains & 1u) vf = ((const unsigned char *)buf)[i];
      if (chains & 2u) ve = ((const unsigned char *)second)[i];
    } else {
      if (chains & 1u) vf = ((const uint32_t *)buf)[i];
      if (chains & 2u) ve = ((const uint32_t *)second)[i];
    }
    if (chains & 1u) assign_free[p] = vf;
    if (chains & 2u) assign_evid[p] = ve;
  }
}

// Sample trace (dwx_trace_enable; NO reference counterpart: the reference only counts the drawn values,
// src/gibbs_sampler.h:160-167, and overwrites every assignment with the next).  The ring holds `cap` planes of
// `words` 8-byte words; a plane is the inference chain's assignment of owned positions [0, n) in device order,
// BITS = 1: bit (p & 63) of word p >> 6 (all-boolean graph: lane <-> position, a wave's 64 values are one
// ballot, one 8-byte store per wave), BITS = 8: byte p (four values per 32-bit store).
// trace_pack_kernel writes the CURRENT assign_evid into planes slot0, slot0 + 1, ... (mod cap), n_planes of
// them: one plane after every single inference sweep, whatever kernels the sweep took.  unsampled_only: the
// positions an inference sweep draws (not evidence, or OPT_SAMPLE_EVIDENCE) are written as 0 -- the planes a
// one-launch run of sweeps (sweep8_kernel<MULTI, TRACE>) is about to fill: its draws are ADDED as disjoint bits
// (BITS = 1) or stored over the zero bytes (BITS = 8), the unsampled positions hold their value in every plane.
template <int BITS>
__global__ void __launch_bounds__(BLOCK_THREADS)
trace_pack_kernel(const uint32_t *assign_evid, const uint32_t *v_meta, uint32_t n, uint32_t unsampled_only,
                  uint32_t sample_evidence, unsigned long long *ring, uint32_t words, uint32_t cap, uint32_t slot0,
                  uint32_t n_planes) {
  const uint32_t stride = gridDim.x * blockDim.x;
  auto keep = [&](uint32_t p) {
    return !unsampled_only || (!sample_evidence && (v_meta[p] & VM_EVIDENCE));
  };
  if (BITS == 1) {
    const uint32_t n_round = (n + blockDim.x - 1) / blockDim.x * blockDim.x;   // (whole workgroups ballot together)
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_round; p += stride) {
      const bool one = p < n && keep(p) && assign_evid[p] != 0;
      const unsigned long long m = DWX_BALLOT(one);
      if ((threadIdx.x & 63u) == 0 && p < n) {   // (p: the wave's first position, a multiple of 64)
        uint32_t slot = slot0;
        for (uint32_t j = 0; j < n_planes; ++j) {
          ring[(size_t)slot * words + (p >> 6)] = m;
          if (++slot == cap) slot = 0;
        }
      }
    }
  } else {
    const uint32_t n4 = (n + 3u) / 4u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      uint32_t packed = 0;
#pragma unroll
      for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t p = 4u * i + b;
        if (p < n && keep(p)) packed |= (assign_evid[p] & 255u) << (8u * b);
      }
      uint32_t slot = slot0;
      for (uint32_t j = 0; j < n_planes; ++j) {
        ((uint32_t *)(ring + (size_t)slot * words))[i] = packed;
        if (++slot == cap) slot = 0;
      }
    }
  }
}

// dwx_trace_read: out[e * n_pos + i] = the value of position pos[i] in entry e of the ring, entry 0 at plane
// slot0 (the oldest entry asked for), one byte each.  pos was translated once per call on the host
// (CompiledGraph::pos, as dwx_graph_get_positions); only the selection crosses to the host.
template <int BITS>
__global__ void __launch_bounds__(BLOCK_THREADS)
trace_gather_kernel(const unsigned long long *ring, uint32_t words, uint32_t cap, uint32_t slot0, uint32_t n_entries,
                    const uint32_t *pos, uint64_t n_pos, unsigned char *out) {
  const uint64_t total = (uint64_t)n_entries * n_pos, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
    const uint64_t e = j / n_pos, i = j - e * n_pos;
    const uint32_t slot = (uint32_t)(((uint64_t)slot0 + e) % cap), p = pos[i];
    const unsigned long long *plane = ring + (size_t)slot * words;
    out[j] = BITS == 1 ? (unsigned char)((plane[p >> 6] >> (p & 63u)) & 1ull) : ((const unsigned char *)plane)[p];
  }
}

// dwx_trace_cooccurrence: joint counts of pairs of value rows over n_entries entries of the ring, entry 0 at plane
// slot0 (NO reference counterpart: the reference keeps counts only, src/gibbs_sampler.h:160-167).  Pair i is the
// positions pos_a[i], pos_b[i] and, BITS = 8, the dense values val_a[i], val_b[i] its two rows are the indicators of
// (a boolean variable's row: 1); BITS = 1 ignores the values (every row is "the bit is set").  The host translated
// the rows once per call.  out[i], out[n_pairs + i], out[2 n_pairs + i] = the entries where both indicators are 1,
// where a's is, where b's is.
// A LANE OWNS A PAIR and keeps its three counts in registers; pairs are walked grid-stride and, within a pass, every
// lane of the grid walks the entries in the same order, oldest first -- the waves resident together read the same
// few planes, which stay in the XCD's L2 while they are needed (a plane of 10 M booleans is 1.25 MB).  The entry
// loop is unrolled COOC_UNROLL times: 2 x COOC_UNROLL independent gathers in flight per lane.  One writer per pair:
// plain coalesced stores, no atomics, no ballots (so no whole-workgroup convergence under the emulation either).
// Counts are 32-bit: n_entries <= the ring's capacity < 2^32.
constexpr uint32_t COOC_UNROLL = 8;
constexpr uint32_t COOC_MAX_BLOCKS = 512;   // the grid's cap: two workgroups per CU, 16 gathers in flight per lane
template <int BITS>
DWX_DEV uint32_t trace_cooc_bit(const unsigned long long *plane, uint32_t p, uint32_t d) {
  if (BITS == 1) return (uint32_t)(plane[p >> 6] >> (p & 63u)) & 1u;
  return ((const unsigned char *)plane)[p] == d ? 1u : 0u;
}
template <int BITS>
__global__ void __launch_bounds__(BLOCK_THREADS)
trace_cooc_kernel(const unsigned long long *ring, uint32_t words, uint32_t cap, uint32_t slot0, uint32_t n_entries,
                  const uint32_t *pos_a, const uint32_t *pos_b, const unsigned char *val_a, const unsigned char *val_b,
                  uint64_t n_pairs, unsigned long long *out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += stride) {
    const uint32_t pa = pos_a[i], pb = pos_b[i];
    const uint32_t da = BITS == 8 ? val_a[i] : 1u, db = BITS == 8 ? val_b[i] : 1u;
    uint32_t n_ab = 0, n_a = 0, n_b = 0;
    uint32_t slot = slot0, e = 0;                  // slot = (slot0 + e) mod cap, slot0 < cap
    for (; e + COOC_UNROLL <= n_entries; e += COOC_UNROLL) {
      uint32_t xa[COOC_UNROLL], xb[COOC_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < COOC_UNROLL; ++u) {
        uint32_t su = slot + u;                    // (u < COOC_UNROLL <= n_entries <= cap: one wrap at the most)
        if (su >= cap) su -= cap;
        const unsigned long long *plane = ring + (size_t)su * words;
        xa[u] = trace_cooc_bit<BITS>(plane, pa, da);
        xb[u] = trace_cooc_bit<BITS>(plane, pb, db);
      }
#pragma unroll
      for (uint32_t u = 0; u < COOC_UNROLL; ++u) { n_ab += xa[u] & xb[u]; n_a += xa[u]; n_b += xb[u]; }
      slot += COOC_UNROLL;
      if (slot >= cap) slot -= cap;
    }
    for (; e < n_entries; ++e) {
      const unsigned long long *plane = ring + (size_t)slot * words;
      const uint32_t x = trace_cooc_bit<BITS>(plane, pa, da), y = trace_cooc_bit<BITS>(plane, pb, db);
      n_ab += x & y; n_a += x; n_b += y;
      if (++slot == cap) slot = 0;
    }
    out[i] = n_ab;
    out[n_pairs + i] = n_a;
    out[2 * n_pairs + i] = n_b;
  }
}

// dwx_score / dwx_trace_score: the joint log-score of a state, sum over ALL factors of w * (sign * fval), from the
// factor-major table (CompiledGraph::frecs; include/dwx.h states the definition, DESIGN.md 3.1j the layout).  The
// reference has the per-variable sum only (FactorGraph::potential, src/factor_graph.h:127-145).
//
// Every one of the ten functions (src/factor.h:112-299) is a function of the arity, the number nb of satisfied BODY
// positions (all but the last) and whether the head (the last) is satisfied -- what a lane can keep per entry while
// it walks a factor's positions once for several entries.  Agrees with factor_sign for every function and arity
// (arity 0, which factor_sign never meets: the functions on no predicates, head false).
DWX_DEV double sign_from_counts(uint32_t func, uint32_t arity, uint32_t nb, bool head) {
  if (arity == 1u) return unary_sign(func, head);
  const uint32_t body = arity ? arity - 1u : 0u;
  switch (func) {
    case FUNC_AND: case FUNC_ISTRUE: return (nb == body && (head || !arity)) ? 1.0 : -1.0;
    case FUNC_AND_CATEGORICAL: return (nb == body && (head || !arity)) ? 1.0 : 0.0;
    case FUNC_OR: return (nb > 0u || head) ? 1.0 : -1.0;
    case FUNC_EQUAL: { const uint32_t k = nb + (head ? 1u : 0u); return (k == 0u || k == arity) ? 1.0 : -1.0; }
    case FUNC_IMPLY_MLN: return (nb != body || head) ? 1.0 : 0.0;
    case FUNC_IMPLY_NATURAL: return nb != body ? 0.0 : (head ? 1.0 : -1.0);
    default: {  // LINEAR, RATIO, LOGICAL: the body positions b with !b || head
      const uint32_t count = head ? body : body - nb;
      if (func == FUNC_LINEAR) return (double)count;
      if (func == FUNC_RATIO) return log2(1.0 + (double)count);
      return count > 0u ? 1.0 : 0.0;
    }
  }
}

// One term into a lane's exact sum: q = llrint(2^32 t) (the scaling is exact, the rounding to nearest-even), its
// arithmetic high part into hi, its low 32 bits into lo -- fewer than 2^32 terms: neither can overflow.
constexpr double SCORE_SCALE = 4294967296.0, SCORE_TERM_LIMIT = 1073741824.0;   // 2^32; |t| < 2^30
DWX_DEV void score_term(double t, long long &hi, unsigned long long &lo, bool &bad) {
  if (!(fabs(t) < SCORE_TERM_LIMIT)) { bad = true; return; }   // (NaN fails the comparison too)
  const long long q = llrint(t * SCORE_SCALE);
  hi += q >> 32;
  lo += (unsigned long long)(uint32_t)q;
}

// Where a position's value comes from.  MODE 0: a live chain, assign[p] (EB = 1).  MODE 1 / 8: the trace ring at a
// bit / a byte per position; a pass covers EB consecutive entries, entry u in plane (slot0 + u) mod cap; entries
// u >= ne (the last pass of a call) read plane slot0 again and are dropped at the end.
#ifndef DWX_SCORE_EB
#define DWX_SCORE_EB 8
#endif
constexpr int SCORE_EB = DWX_SCORE_EB;
#ifndef DWX_SCORE_MAX_BLOCKS
#define DWX_SCORE_MAX_BLOCKS 1024
#endif
constexpr uint32_t SCORE_MAX_BLOCKS = DWX_SCORE_MAX_BLOCKS;   // the grid's cap: four workgroups per CU walk the same few planes
template <int MODE, int EB>
struct ScoreReader {
  const unsigned char *plane[EB];
  DWX_DEV ScoreReader(const void *src, uint32_t words, uint32_t cap, uint32_t slot0, uint32_t ne) {
#pragma unroll
    for (int u = 0; u < EB; ++u) {
      uint32_t su = slot0;
      if (MODE != 0 && (uint32_t)u < ne) {        // (slot0 < cap, u < ne <= cap: one wrap at the most)
        su = slot0 + (uint32_t)u;
        if (su >= cap) su -= cap;
      }
      plane[u] = (const unsigned char *)src + (MODE == 0 ? (size_t)0 : (size_t)su * words * 8u);
    }
  }
  // the EB gathers of one position, issued together
  DWX_DEV void sat(const VifRec vf, bool (&s)[EB]) const {
    uint32_t x[EB];
#pragma unroll
    for (int u = 0; u < EB; ++u) {
      if (MODE == 0) x[u] = ((const uint32_t *)plane[u])[vf.vid];
      else if (MODE == 1) x[u] = (((const uint32_t *)plane[u])[vf.vid >> 5] >> (vf.vid & 31u)) & 1u;   // (little-endian: bit p of the plane)
      else x[u] = plane[u][vf.vid];
    }
#pragma unroll
    for (int u = 0; u < EB; ++u) s[u] = x[u] == vf.equal_to;
  }
};

// The lanes' sums of a workgroup into acc[2u], acc[2u + 1] (hi, lo of entry u < ne): per wave with the segmented
// sum over one run (all 64 lanes reach it), across waves through LDS, then ONE atomic pair per workgroup and entry.
// Integer sums: the result does not depend on the grid or on the order of the atomics.
template <int EB>
DWX_DEV void score_reduce(const long long (&hi)[EB], const unsigned long long (&lo)[EB], bool bad, uint32_t ne,
                          unsigned long long *acc, unsigned *flag) {
  __shared__ unsigned long long s_part[BLOCK_THREADS / 64u][2 * EB];
  const uint32_t t = threadIdx.x, wave = t >> 6;
#pragma unroll
  for (int u = 0; u < EB; ++u) {
    bool head = false;
    const long long h = DWX_WAVE_SEG_SUM_I64(0u, hi[u], head);
    const long long l = DWX_WAVE_SEG_SUM_I64(0u, (long long)lo[u], head);
    if ((t & 63u) == 0u) { s_part[wave][2 * u] = (unsigned long long)h; s_part[wave][2 * u + 1] = (unsigned long long)l; }
  }
  if (bad) atomicAdd(flag, 1u);
  __syncthreads();
  if (t < 2u * ne) {
    unsigned long long sum = 0;
    for (uint32_t w = 0; w < BLOCK_THREADS / 64u; ++w) sum += s_part[w][t];
    if (sum) atomicAdd(&acc[t], sum);
  }
}

// A LANE OWNS A FACTOR, grid-stride over the table: the 16-byte records are one coalesced stream, a factor's entries
// 8-byte loads at consecutive addresses from lane to lane where arities agree, and every position's value EB
// independent gathers (trace_cooc_kernel's pattern: the waves resident together read the same few planes, which
// stay in L2 meanwhile).  Factors wider than SCORE_WAVE_ARITY are score_wide_kernel's.  No wave operation inside
// the loop: lanes may leave it at different times.
template <int MODE, int EB>
__global__ void __launch_bounds__(BLOCK_THREADS)
score_kernel(const FactorRec *recs, const double *fval64, const VifRec *vifs, uint32_t n_factors, const double *weights,
             const void *src, uint32_t words, uint32_t cap, uint32_t slot0, uint32_t ne, unsigned long long *acc,
             unsigned *flag) {
  const ScoreReader<MODE, EB> rd(src, words, cap, slot0, ne);
  long long hi[EB];
  unsigned long long lo[EB];
#pragma unroll
  for (int u = 0; u < EB; ++u) { hi[u] = 0; lo[u] = 0; }
  bool bad = false;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_factors; f += stride) {
    const FactorRec r = recs[f];
    const uint32_t func = r.packed & FREC_FUNC_MASK, field = r.packed >> FREC_ARITY_SHIFT;
    const uint32_t arity = (r.packed & FREC_UNARY) ? 1u : field;
    if (arity > SCORE_WAVE_ARITY) continue;
    uint32_t nb[EB];
    bool head[EB], s[EB];
#pragma unroll
    for (int u = 0; u < EB; ++u) { nb[u] = 0; head[u] = false; }
    if (r.packed & FREC_UNARY) {
      rd.sat(VifRec{r.aux, field}, head);
    } else {
      const VifRec *v = vifs + r.aux;
      for (uint32_t i = 0; i + 1u < arity; ++i) {
        rd.sat(v[i], s);
#pragma unroll
        for (int u = 0; u < EB; ++u) nb[u] += s[u] ? 1u : 0u;
      }
      if (arity) rd.sat(v[arity - 1u], head);
    }
    const double fv = (r.packed & FREC_F64_FLAG) ? fval64[f] : (double)r.fval;
    const double w = weights[r.wid];
#pragma unroll
    for (int u = 0; u < EB; ++u) score_term(w * (sign_from_counts(func, arity, nb[u], head[u]) * fv), hi[u], lo[u], bad);
  }
  score_reduce<EB>(hi, lo, bad, ne, acc, flag);
}

// A WAVE OWNS A WIDE FACTOR (arity > SCORE_WAVE_ARITY; wide[] lists them): lanes take its positions strided and
// count their satisfied body positions, one segmented sum per entry yields nb and the head (packed: head << 32 |
// nb), lane 0 evaluates the function and keeps the term.  The waves' loop over the list has the same trip count in
// all 64 lanes; no ballot (arities differ from wave to wave).
template <int MODE, int EB>
__global__ void __launch_bounds__(BLOCK_THREADS)
score_wide_kernel(const FactorRec *recs, const double *fval64, const VifRec *vifs, const uint32_t *wide, uint32_t n_wide,
                  const double *weights, const void *src, uint32_t words, uint32_t cap, uint32_t slot0, uint32_t ne,
                  unsigned long long *acc, unsigned *flag) {
  const ScoreReader<MODE, EB> rd(src, words, cap, slot0, ne);
  long long hi[EB];
  unsigned long long lo[EB];
#pragma unroll
  for (int u = 0; u < EB; ++u) { hi[u] = 0; lo[u] = 0; }
  bool bad = false;
  const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (BLOCK_THREADS / 64u);
  for (uint32_t i = blockIdx.x * (BLOCK_THREADS / 64u) + (threadIdx.x >> 6); i < n_wide; i += waves) {
    const uint32_t f = wide[i];
    const FactorRec r = recs[f];
    const uint32_t func = r.packed & FREC_FUNC_MASK, arity = r.packed >> FREC_ARITY_SHIFT;
    const VifRec *v = vifs + r.aux;
    long long cnt[EB];
    bool s[EB];
#pragma unroll
    for (int u = 0; u < EB; ++u) cnt[u] = 0;
    for (uint32_t j = lane; j < arity; j += 64u) {
      rd.sat(v[j], s);
      const long long one = j + 1u == arity ? (1ll << 32) : 1ll;
#pragma unroll
      for (int u = 0; u < EB; ++u) cnt[u] += s[u] ? one : 0ll;
    }
    const double fv = (r.packed & FREC_F64_FLAG) ? fval64[f] : (double)r.fval;
    const double w = weights[r.wid];
#pragma unroll
    for (int u = 0; u < EB; ++u) {
      bool first = false;
      const long long c = DWX_WAVE_SEG_SUM_I64(0u, cnt[u], first);
      if (lane == 0u)
        score_term(w * (sign_from_counts(func, arity, (uint32_t)c, (c >> 32) != 0) * fv), hi[u], lo[u], bad);
    }
  }
  score_reduce<EB>(hi, lo, bad, ne, acc, flag);
}

// dwx_weight_stats / dwx_trace_weight_stats: per weight w the exact sum of u_f = sign_f * fval_f over the factors on
// w and over the entries [0, n) of the call (include/dwx.h states the definition, DESIGN.md 3.1k the choices): the
// score's reads without the weights' values, and a scatter onto W hi / lo pairs acc[2w], acc[2w + 1] instead of
// one pair per entry.  Terms are combined in three steps before any atomic: over the entries inside the lane (the
// loop over groups of EB entries below: a factor's record, its feature value and wid are read once per call),
// over neighbouring lanes of equal wid with the keyed segmented sum, and only run heads issue the atomic pair.
// Integer sums: the result does not depend on the grid, on which lanes combined or on the order of the atomics.
#ifndef DWX_WSTATS_EB
#define DWX_WSTATS_EB 8
#endif
constexpr int WSTATS_EB = DWX_WSTATS_EB;
#ifndef DWX_WSTATS_MAX_BLOCKS
#define DWX_WSTATS_MAX_BLOCKS 2048
#endif
constexpr uint32_t WSTATS_MAX_BLOCKS = DWX_WSTATS_MAX_BLOCKS;   // the grid's cap: eight workgroups per CU
constexpr uint32_t WSTATS_NO_KEY = 0xFFFFFFFFu;                  // an idle lane's key (no weight has this id: W < 2^32)

// the plane of the g-th group of EB entries of a call whose first entry lies in plane slot0 (g * EB < n <= cap)
DWX_DEV uint32_t wstats_group_slot(uint32_t slot0, uint32_t e0, uint32_t cap) {
  const uint64_t s = (uint64_t)slot0 + e0;          // (slot0 < cap or a live chain's 0 == cap; e0 < n <= cap: one wrap at the most)
  return (uint32_t)(s >= cap ? s - cap : s);
}

// The run of equal keys a lane belongs to, numbered along the wave.  The segmented sum wants equal keys in ONE run
// of neighbouring lanes (pull_grad_kernel's are sorted); weight ids in factor order are not -- w, x, w would add
// lane 2 into lane 0 -- so the sums below are keyed by the run's number instead.  A lane learns its right
// neighbour's key from the pair swap (even lanes) or from a two-lane segmented sum over the pairs (1, 2), (3, 4), ...
// (odd lanes); the ballot of "my run ends here" counts the runs before a lane.  Every lane of the workgroup calls.
DWX_DEV uint32_t wstats_run_id(uint32_t key, uint32_t lane) {
  const uint32_t partner = DWX_PAIR_SWAP_U32(key);
  bool unused = false;
  const long long two = DWX_WAVE_SEG_SUM_I64((lane + 1u) >> 1, (long long)key, unused);
  const bool cont = (lane & 1u) ? (lane < 63u && (uint32_t)(two - (long long)key) == key) : partner == key;
  const unsigned long long ends = DWX_BALLOT(!cont);
  return (uint32_t)__builtin_popcountll(ends & ((1ull << lane) - 1ull));
}

// A LANE OWNS A FACTOR, grid-stride over the table by whole workgroups: the trip count is the same in all lanes
// (wave operations close every trip); lanes past the table, and lanes whose factor is the wide kernel's, carry a
// zero term -- the former under the sentinel key, the latter under their own wid, so that they do not cut a run.
template <int MODE, int EB>
__global__ void __launch_bounds__(BLOCK_THREADS)
weight_stats_kernel(const FactorRec *recs, const double *fval64, const VifRec *vifs, uint32_t n_factors, const void *src,
                    uint32_t words, uint32_t cap, uint32_t slot0, uint32_t n, unsigned long long *acc, unsigned *flag) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t f0 = (uint64_t)blockIdx.x * blockDim.x; f0 < n_factors; f0 += stride) {
    const uint64_t f = f0 + threadIdx.x;
    const bool valid = f < n_factors;
    FactorRec r{0u, 0u, 0u, 0.0f};
    if (valid) r = recs[f];
    const uint32_t func = r.packed & FREC_FUNC_MASK, field = r.packed >> FREC_ARITY_SHIFT;
    const uint32_t arity = (r.packed & FREC_UNARY) ? 1u : field;
    const bool mine = valid && arity <= SCORE_WAVE_ARITY;
    long long hi = 0;
    unsigned long long lo = 0;
    if (mine) {
      const double fv = (r.packed & FREC_F64_FLAG) ? fval64[f] : (double)r.fval;
      for (uint32_t e0 = 0; e0 < n; e0 += (uint32_t)EB) {
        const uint32_t ne = n - e0 < (uint32_t)EB ? n - e0 : (uint32_t)EB;
        const ScoreReader<MODE, EB> rd(src, words, cap, wstats_group_slot(slot0, e0, cap), ne);
        uint32_t nb[EB];
        bool head[EB], s[EB];
#pragma unroll
        for (int u = 0; u < EB; ++u) { nb[u] = 0; head[u] = false; }
        if (r.packed & FREC_UNARY) {
          rd.sat(VifRec{r.aux, field}, head);
        } else {
          const VifRec *v = vifs + r.aux;
          for (uint32_t i = 0; i + 1u < arity; ++i) {
            rd.sat(v[i], s);
#pragma unroll
            for (int u = 0; u < EB; ++u) nb[u] += s[u] ? 1u : 0u;
          }
          if (arity) rd.sat(v[arity - 1u], head);
        }
#pragma unroll
        for (int u = 0; u < EB; ++u)
          if ((uint32_t)u < ne) score_term(sign_from_counts(func, arity, nb[u], head[u]) * fv, hi, lo, bad);
      }
    }
    const uint32_t key = valid ? r.wid : WSTATS_NO_KEY;
    const uint32_t run = wstats_run_id(key, lane);
    bool first = false;
    const long long h = DWX_WAVE_SEG_SUM_I64(run, hi, first);
    const long long l = DWX_WAVE_SEG_SUM_I64(run, (long long)lo, first);   // (two's complement: the unsigned sum mod 2^64, which it is below)
    if (first && valid) {
      if (h) atomicAdd(&acc[2 * (size_t)key], (unsigned long long)h);
      if (l) atomicAdd(&acc[2 * (size_t)key + 1], (unsigned long long)l);
    }
  }
  if (bad) atomicAdd(flag, 1u);
}

// A WAVE OWNS A WIDE FACTOR, as in score_wide_kernel; lane 0 keeps the terms.  Consecutive factors of a wave's walk
// that share a weight are combined in lane 0 before the atomic pair (wide[] ascends: factors of one rule are
// usually neighbours).
template <int MODE, int EB>
__global__ void __launch_bounds__(BLOCK_THREADS)
weight_stats_wide_kernel(const FactorRec *recs, const double *fval64, const VifRec *vifs, const uint32_t *wide, uint32_t n_wide,
                         const void *src, uint32_t words, uint32_t cap, uint32_t slot0, uint32_t n, unsigned long long *acc,
                         unsigned *flag) {
  const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (BLOCK_THREADS / 64u);
  bool bad = false;
  uint32_t cur = WSTATS_NO_KEY;
  long long hi = 0;
  unsigned long long lo = 0;
  for (uint32_t i = blockIdx.x * (BLOCK_THREADS / 64u) + (threadIdx.x >> 6); i < n_wide; i += waves) {
    const uint32_t f = wide[i];
    const FactorRec r = recs[f];
    const uint32_t func = r.packed & FREC_FUNC_MASK, arity = r.packed >> FREC_ARITY_SHIFT;
    const VifRec *v = vifs + r.aux;
    const double fv = (r.packed & FREC_F64_FLAG) ? fval64[f] : (double)r.fval;
    if (lane == 0u && r.wid != cur) {
      if (hi) atomicAdd(&acc[2 * (size_t)cur], (unsigned long long)hi);
      if (lo) atomicAdd(&acc[2 * (size_t)cur + 1], lo);
      cur = r.wid; hi = 0; lo = 0;
    }
    for (uint32_t e0 = 0; e0 < n; e0 += (uint32_t)EB) {
      const uint32_t ne = n - e0 < (uint32_t)EB ? n - e0 : (uint32_t)EB;
      const ScoreReader<MODE, EB> rd(src, words, cap, wstats_group_slot(slot0, e0, cap), ne);
      long long cnt[EB];
      bool s[EB];
#pragma unroll
      for (int u = 0; u < EB; ++u) cnt[u] = 0;
      for (uint32_t j = lane; j < arity; j += 64u) {
        rd.sat(v[j], s);
        const long long one = j + 1u == arity ? (1ll << 32) : 1ll;
#pragma unroll
        for (int u = 0; u < EB; ++u) cnt[u] += s[u] ? one : 0ll;
      }
#pragma unroll
      for (int u = 0; u < EB; ++u) {
        bool first = false;
        const long long c = DWX_WAVE_SEG_SUM_I64(0u, cnt[u], first);
        if (lane == 0u && (uint32_t)u < ne)
          score_term(sign_from_counts(func, arity, (uint32_t)c, (c >> 32) != 0) * fv, hi, lo, bad);
      }
    }
  }
  if (lane == 0u && cur != WSTATS_NO_KEY) {
    if (hi) atomicAdd(&acc[2 * (size_t)cur], (unsigned long long)hi);
    if (lo) atomicAdd(&acc[2 * (size_t)cur + 1], lo);
  }
  if (bad) atomicAdd(flag, 1u);
}

// test hook: the raw Philox4x32-10 block function and the two uniforms drawn from it, on the
// device (Random123 known-answer vectors; tests/test_philox_kat.py)
__global__ void test_philox_kernel(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                   uint32_t *out, double *uni) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    philox4x32_10(k0, k1, c0, c1, c2, c3);
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    // the same block through the sampler's own entry point: seed = key, counter = (vid, sweep)
    philox_uniforms((uint64_t)k0 | ((uint64_t)k1 << 32), (uint64_t)out[4] | ((uint64_t)out[5] << 32),
                    (uint64_t)out[6] | ((uint64_t)out[7] << 32), uni[0], uni[1]);
  }
}

// test hook: one factor function evaluated on the device (test/factor_test.cc)
__global__ void test_sign_kernel(uint32_t func, uint32_t arity, const VifRec *vifs,
                                 const uint32_t *assign, double *out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (arity == 1) out[0] = factor_sign(func, 1, 1u, vifs, assign, 0u, assign[0]);
    else out[0] = factor_sign(func, arity, 0u, vifs, assign, kNoVar, 0u);
  }
}

// test hook: the wave-level primitives behind device_intrinsics.h, one workgroup of BLOCK_THREADS lanes on the
// caller's per-lane inputs (include/dwx.h: dwx_test_wave_ops; tests/test_wave_ops.py).  `op` is uniform: every lane
// of the workgroup reaches the same primitive together.
constexpr int WAVE_OP_LOAD_K = (int)STAGE_UNROLL, WAVE_OP_SORT_K = 4;
__global__ void __launch_bounds__(BLOCK_THREADS)
test_wave_ops_kernel(uint32_t op, const unsigned long long *in, const void *recs, uint32_t n_rec, uint32_t first,
                     unsigned long long *out) {
  const uint32_t t = threadIdx.x;
  if (op == DWX_WAVE_OP_SEG_SUM) {
    bool head = false;
    const long long s = DWX_WAVE_SEG_SUM_I64((uint32_t)in[t], (long long)in[BLOCK_THREADS + t], head);
    out[t] = (unsigned long long)s;
    out[BLOCK_THREADS + t] = head ? 1ull : 0ull;
  } else if (op == DWX_WAVE_OP_SUM_F64) {
    double v;
    const unsigned long long bits = in[t];
    __builtin_memcpy(&v, &bits, 8);
    const double s = DWX_WAVE_SUM_F64(v);
    unsigned long long r;
    __builtin_memcpy(&r, &s, 8);
    out[t] = r;
  } else if (op == DWX_WAVE_OP_BALLOT) {
    out[t] = DWX_BALLOT(in[t] != 0ull);
  } else if (op == DWX_WAVE_OP_PAIR_SWAP) {
    out[t] = DWX_PAIR_SWAP_U32((uint32_t)in[t]);
  } else if (op == DWX_WAVE_OP_LOAD16) {
    EdgeRec rec[WAVE_OP_LOAD_K];
    DWX_LOAD_TILE_RECORDS(WAVE_OP_LOAD_K, (const EdgeRec *)recs, n_rec, t, rec);
#pragma unroll
    for (int k = 0; k < WAVE_OP_LOAD_K; ++k) {
      uint32_t fw;
      __builtin_memcpy(&fw, &rec[k].fval, 4);
      out[(k * BLOCK_THREADS + t) * 2u] = (unsigned long long)rec[k].wid | ((unsigned long long)rec[k].aux << 32);
      out[(k * BLOCK_THREADS + t) * 2u + 1u] = (unsigned long long)rec[k].packed | ((unsigned long long)fw << 32);
    }
  } else if (op == DWX_WAVE_OP_LOAD8) {
    EdgeRec8 rec[WAVE_OP_LOAD_K];
    DWX_LOAD_TILE_RECORDS8(WAVE_OP_LOAD_K, (const EdgeRec8 *)recs, n_rec, t, rec);
#pragma unroll
    for (int k = 0; k < WAVE_OP_LOAD_K; ++k) {
      uint32_t fw;
      __builtin_memcpy(&fw, &rec[k].f, 4);
      out[k * BLOCK_THREADS + t] = (unsigned long long)rec[k].key | ((unsigned long long)fw << 32);
    }
  } else if (op == DWX_WAVE_OP_LOAD_SORTED) {
    SortRec8 rec[WAVE_OP_SORT_K];
    DWX_LOAD_SORTED_RECORDS(WAVE_OP_SORT_K, (const SortRec8 *)recs, n_rec, first, t, rec);
#pragma unroll
    for (int k = 0; k < WAVE_OP_SORT_K; ++k)
      out[k * BLOCK_THREADS + t] = (unsigned long long)rec[k].wid | ((unsigned long long)rec[k].od << 32);
  }
}

}  // namespace dwx
#endif  // DWX_AUX_KERNELS_H_
