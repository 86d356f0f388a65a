// dwx_api.cc -- implementation of the C ABI in include/dwx.h.
//
// Compiled as HIP for gfx950 into libdwx.so (Makefile).  The runtime layer is
// rt_hip.h; when DWX_EMU is defined (tests/hipemu only) the same file is compiled by
// g++ against a host emulation of that layer so the kernels run under sanitizers.
#include "../../include/dwx.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_build.h"
#include "graph_compile.h"
#include "host_parallel.h"
#include "level_build.h"
#if defined(DWX_EMU) && !defined(DWX_EMU_LEVEL_BUILD_UNIT)
#include "level_build.cc"   // (a host harness recipe that does not compile that unit itself: the suite of a revision before it)
#endif

#include "sweep_kernels.h"   // (device_intrinsics.h: the HIP runtime shim rt_hip.h comes with it)
#include "diag_kernels.h"    // (dwx_trace_diagnostics)

// a finer cut must lower the batches' curvature estimate to this fraction, else the plan stops
// (dwx_sgd_plan; multi-GPU drivers apply the same rule to the global estimate)
constexpr double PLAN_MIN_GAIN = 0.8;

#ifndef DWX_PULL_GRID
#define DWX_PULL_GRID 16u   // pull_grad_kernel workgroups per CU (grid-stride beyond)
#endif

using namespace dwx;

namespace {
thread_local std::string g_err;

// the heavy build phases run on the sampler's device where the library can (device_build.hip);
// DWX_HOST_BUILD=1: the host builders, which are also their checker (level_build.cc, graph_compile.cc)
bool build_on_device() { return devb::available() && !getenv("DWX_HOST_BUILD"); }

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

struct RangeError : std::runtime_error {   // -> DWX_E_LIMIT
  using std::runtime_error::runtime_error;
};

template <class Fn>
int guarded(Fn &&fn) {
  try {
    fn();
    return DWX_OK;
  } catch (const std::bad_alloc &) {
    return fail(DWX_E_NOMEM, "out of host memory");
  } catch (const RangeError &e) {
    return fail(DWX_E_LIMIT, e.what());
  } catch (const std::invalid_argument &e) {
    return fail(DWX_E_INVALID, e.what());
  } catch (const std::exception &e) {
    return fail(DWX_E_DEVICE, e.what());
  }
}

// `pad` extra zeroed elements behind the data (the kernels' clamped, branch-free loads
// may touch one element past an empty tile)
template <class T>
T *upload(const std::vector<T> &v, rt::stream_t s, size_t pad = 0) {
  T *d = (T *)rt::dmalloc((v.size() + pad) * sizeof(T));
  rt::h2d(d, v.data(), v.size() * sizeof(T), s);
  if (pad) rt::dmemset(d + v.size(), 0, pad * sizeof(T), s);
  return d;
}

template <class T>
T *upload(const RawArray<T> &v, rt::stream_t s, size_t pad = 0) {
  T *d = (T *)rt::dmalloc((v.size() + pad) * sizeof(T));
  rt::h2d(d, v.data(), v.size() * sizeof(T), s);
  if (pad) rt::dmemset(d + v.size(), 0, pad * sizeof(T), s);
  return d;
}

// an optional device buffer: nullptr instead of an exception when the device is out of memory (the emulation's
// runtime layer has the throwing allocator only: host memory)
void *optional_dmalloc(size_t n) {
#ifdef DWX_EMU
  return rt::dmalloc(n);
#else
  return rt::try_dmalloc(n);
#endif
}

template <class T>
T *upload_raw(const T *h, size_t n, rt::stream_t s) {
  T *d = (T *)rt::dmalloc(n * sizeof(T));
  rt::h2d(d, h, n * sizeof(T), s);
  return d;
}

struct TimedSpan {
  rt::event_t a, b, c;   // a..b: sweep kernels of all colours; b..c: pull_grad_kernel (learning)
  int kind;
  uint32_t launches;
  bool has_pull;
  bool new_sweep;   // the span opens a sweep (inference: always; learning: its first chunk)
  uint32_t n_sweeps = 1;   // ... or several (dwx_sample_n_async on an all-unary graph)
};

// One build of a sweep-family kernel as this sampler runs it.  dwx_sampler_create resolves every role's build
// once (resolve_builds) and the launch sites go through launch(): a launch cannot name a build, an LDS size or
// a grid bound other than the one create set up.
template <class... A>
struct Variant {
  void (*fn)(A...) = nullptr;   // nullptr: the graph never runs this role
  size_t lds = 0;               // dynamic LDS of every launch
  unsigned cap = 1;             // workgroups resident on the whole chip: the bound of a persistent grid
  bool allowed = false;         // the dynamic-LDS allowance of `lds` is set
  void allow() {
    if (!allowed) { rt::allow_dynamic_lds(fn, lds); allowed = true; }
  }
  // allowance and occupancy at create: the plain builds
  static Variant eager(void (*f)(A...), size_t bytes) {
    Variant v;
    v.fn = f; v.lds = bytes;
    v.allow();
    v.cap = rt::resident_blocks(f, BLOCK_THREADS, bytes);
    return v;
  }
  // Another build of this role (RB, TRACE, several sweeps per launch), set up by its first launch, not at
  // create: a sampler that never runs it pays nothing.  Its persistent grid is the one sized from this build's
  // occupancy: a build that keeps fewer workgroups resident runs the surplus ones after the first leave --
  // correct, the tiles are strided.
  Variant lazy(void (*f)(A...)) const {
    Variant v = *this;
    v.fn = f; v.allowed = false;
    return v;
  }
  template <class... B>
  void launch(unsigned grid, unsigned block, rt::stream_t st, B... args) {
    if (!fn) throw std::logic_error("a sweep kernel build that dwx_sampler_create did not resolve for this graph");
    allow();
    rt::launch(fn, grid, block, lds, st, args...);
  }
};
using SweepVariant = Variant<KernelParams>;
using SortedVariant = Variant<KernelParams, const SuperTile *, uint32_t, const SortRec8 *, const double *, uint32_t>;
struct SweepVariants {
  SweepVariant infer[2];            // the lane tiles' inference sweep, [RB]
  SweepVariant learn, learn_pull;   // ... learning sweep; the same build staging 16-byte terms only (all_pull)
  SweepVariant tab[2];              // inference on the 8-byte terms table, [RB]
  SweepVariant multi[2][2];         // several inference sweeps per launch, [RB][TRACE]
  Variant<KernelParams, MergeArgs> merged[2];   // a mini-batch with the last one's update as prologue; [1]: a workgroup per tile
  Variant<KernelParams, PersistArgs> persist;   // a split learning sweep as one launch
  SortedVariant sorted_infer[2][2], sorted_learn[2];   // weight-sorted super-tiles, [UNI][RB] and [UNI]
};
}  // namespace

struct dwx_graph {
  std::shared_ptr<CompiledGraph> cg;
};

struct dwx_sampler {
  std::shared_ptr<CompiledGraph> cg;
  dwx_options opts;
  int device = 0;
  rt::stream_t stream = nullptr;
  // The three degree bins of a launch are independent sets of one colour: the wave-per-variable and
  // workgroup-per-variable kernels run beside the tiles' sweep kernel on two side streams, forked
  // from and joined into `stream` with events (a hub graph's chunk: 180 -> 85 us).
  rt::stream_t side[2] = {nullptr, nullptr};
  rt::event_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  // device buffers
  uint32_t *d_v_meta = nullptr, *d_v_orig = nullptr, *d_v_row = nullptr, *d_v_init = nullptr;
  uint32_t *d_row_ptr = nullptr;
  TileDesc *d_tiles = nullptr;
  uint32_t *d_giant = nullptr, *d_wide = nullptr;
  // oversized variables: categorical ones -> giant_kernel (one workgroup each, d_giant);
  // boolean ones -> pieces of GIANT_PIECE records over several workgroups (giant_pot_kernel,
  // giant_decide_kernel, giant_grad_kernel)
  std::vector<uint32_t> cgiant_tiles, bgiant_tiles, bgiant_piece_off;
  uint32_t *d_bgiant = nullptr, *d_bgiant_piece_off = nullptr, *d_bgiant_decision = nullptr;
  GiantPiece *d_bgiant_pieces = nullptr;
  double *d_bgiant_partial = nullptr;
  int stage_k = 12;
  // learning-sweep plan (dwx_sgd_plan)
  struct Chunk { uint32_t launch, t0, t1; };
  std::vector<Chunk> plan_chunks;
  uint32_t plan_batches = 1;
  double plan_eta = 0.0;
  bool plan_valid = false;
  std::map<uint32_t, double> row_sum_cache;   // batches -> R
  std::vector<uint64_t> sgd_work;             // [tiles + 1] prefix sums of SGD-visited records
  uint64_t sgd_work_max_launch = 0;           // ... of the colour launch with the most
  bool wide_learn = false;   // the graph has TILE_TERMS2 tiles: 32-byte staged records when learning
  bool tv_pair = false;      // every lane tile is pre-signed unary and / or inline arity-2: sweep_kernel<.., TV_PAIR>
  SweepVariants kv;                     // the sweep kernels' builds for this graph, resolved at create
  bool rec8 = false;                    // the graph streams 8-byte records (CompiledGraph::edges8)
  bool rp_cat = false;                  // ... with every row pointer of a categorical tile prefetched (K = 6 builds)
  // every tile that fits is TILE_PULL: a learning sweep with the pull gradient stages 16-byte
  // terms only (no f32 weight array behind the records) -- smaller LDS, one more workgroup per CU
  bool all_pull = false;
  EdgeRec8 *d_edges8 = nullptr;
  // weight-sorted super-tiles (sorted_sweep_kernel)
  SortRec8 *d_sorted = nullptr;
  SuperTile *d_supers = nullptr;
  double *d_sort_dvals = nullptr;
  uint32_t n_sort_dvals = 0;
  bool sorted_learn = false;            // ... also in learning sweeps (the super-tiles' tiles pull their gradient)
  bool no_sort_uni = false;             // DWX_NO_SORT_UNI: never the single-d build of sorted_sweep_kernel (A/B)
  bool sorted_fallback_said = false;    // the "more than 8 runs: tile sweep instead" note was printed
  double *d_row_truth = nullptr, *d_edge_fval64 = nullptr;
  EdgeRec *d_edges = nullptr;
  VifRec *d_vifs = nullptr;
  uint32_t *d_assign_free = nullptr, *d_assign_evid = nullptr, *d_tally = nullptr;
  double *d_weights = nullptr;
  float *d_w32 = nullptr;
  double *d_w_init = nullptr;   // initial weights, uploaded on the first replica averaging
  // tabulated potential terms of the pre-signed records (inference with unchanged weights)
  EdgeTerms *d_terms = nullptr;
  int terms_state = 0;          // 0 weights changed since / 1 one inference sweep ran on them / 2 table valid
  // potential cache: on an all-unary graph a variable's pp - pn depends on the weights
  // only, so the learning sweep that follows an inference sweep on the same weights takes the query
  // variables' sums the inference sweep summed instead of streaming their records again
  // Rao-Blackwellised marginals (dwx_rb_enable; tile_walk.h rb_*): [R] 32.32 fixed-point sums, device order
  unsigned long long *d_rb = nullptr;   // allocated by the first enable
  bool rb_on = false;                   // inference sweeps run the RB builds of their kernels and accumulate
  // Sample trace (dwx_trace_enable): a ring of the last trace_cap inference sweeps' assignments of
  // the inference chain, packed (aux_kernels.h: trace_pack_kernel), in device order
  unsigned long long *d_trace = nullptr;   // [trace_cap][trace_words], allocated by the first enable
  uint32_t trace_cap = 0, trace_words = 0, trace_bits = 0;   // planes; 8-byte words per plane; 1 or 8 bits per position
  uint32_t trace_next = 0, trace_count = 0;                  // the plane the next sweep writes; entries held
  bool trace_on = false;                   // inference sweeps record
  std::vector<uint64_t> trace_ids;         // [trace_cap] by plane: the sweep counter its entry was drawn at
  // Joint log-score (dwx_score, dwx_trace_score): the device copy of the graph's factor-major table,
  // uploaded by the first call
  FactorRec *d_frecs = nullptr;
  VifRec *d_fvifs = nullptr;
  double *d_ffval64 = nullptr;
  uint32_t *d_fwide = nullptr;
  bool score_ready = false;
  // Per-weight feature sums (dwx_weight_stats, dwx_trace_weight_stats): the factors on the
  // most-used weight, counted once from the table by the first call (the term-count guard of the two-limb sums)
  bool wstats_ready = false;
  uint64_t wstats_max_count = 0, wstats_max_wid = 0;
  long long *d_pot = nullptr;       // [V] fixed-point sums by device position (allocated on first use)
  int pot_alloc = 0;                // 0 not tried yet, 1 d_pot allocated, -1 no cache (not eligible, DWX_NO_POT_CACHE, no memory)
  std::vector<uint8_t> pot_valid;   // [launches] one sweep stored every query tile's sum, no weight changed since
  bool pot_wanted = false;          // a learning sweep has followed an inference sweep: inference sweeps store
  bool last_infer = false;          // the last sweep enqueued was an inference sweep
  bool pot_query_first = false;     // DWX_POT_QUERY_FIRST: a learning launch runs its cached super-tiles first (A/B)
  uint64_t pot_supers = 0, pot_sweeps = 0;   // super-tiles / learning sweeps served from the cache
  // Deferred draws: an un-split learning sweep of an all-unary graph launches over its
  // evidence tiles only; the draws of its query tiles are owed until somebody reads the chains
  // (flush_pending) or a later sweep overwrites them unread (drop_pending / enqueue_inference).
  struct Pending {
    bool owed = false;            // the free chain of every query variable is still that of an earlier sweep
    bool evid_owed = false;       // ... and so is the evidence chain (no inference sweep has run since)
    uint64_t sweep = 0;           // the sweep counter the owed draws are drawn with
    bool snap = false;            // d_w32 has changed since that sweep: its weights are in d_w32_prev (else still in d_w32)
    std::vector<uint8_t> cached;  // [launches] the potential cache still holds that launch's sums under the sweep's weights
  } pending;
  bool defer_ok = false;          // the graph and the options allow it, and no assignment buffer was handed out
  float *d_w32_prev = nullptr;    // [W + 1] d_w32 as the last deferring sweep read it, once pending.snap says so: written
                                  // by whoever overwrites d_w32 first (apply_kernel; keep_snapshot for the host's writers)
  uint64_t deferred_sweeps = 0, flushes = 0;
  bool has_simple_tiles = false;
  // pull-based gradient (TILE_PULL tiles)
  unsigned long long *d_delta = nullptr;
  // One incidence list + static update counts per plan level (number of batches): sorted by
  // (chunk, weight), every chunk padded to whole runs; t_static holds one row of W counts per
  // chunk (rows >= chunks: a multi-GPU driver sizes it for the slowest rank).  Level 1 (the
  // un-split sweep) is built at create, the others when a plan first needs them.
  struct Level {
    std::vector<Chunk> chunks;
    bool fast = false;                 // lists + static counts present (else: atomics, dynamic T)
    uint32_t *d_inc_wid = nullptr, *d_inc_slot = nullptr;
    float *d_inc_d = nullptr;
    std::vector<uint32_t> inc_begin, inc_end;   // per chunk, entries (multiples of PULL_RUN)
    long long *d_t_static = nullptr;   // [rows][T[W] | h[W]]: static update counts, curvature bounds
    uint32_t rows = 0;
    double c_max = 0.0, t_max = 0.0;   // largest h and largest static T of any (chunk, weight)
    // not empty: a mini-batch of this level can take a weight's int64 sums past 2^63 - 1
    // (learning_range_error); the level holds its chunks only and no plan may use it
    std::string range_error;
    // block pull (pull_ell_kernel; graphs with many weights): per group of the tables (the
    // un-split sweep, or each chunk of a split one) entry rows per (variable block, weight);
    // d_inc_* then only holds what did not fit a row, and d_ov_start where each weight's leftovers
    // start in the group's part of it (W + 1 offsets from inc_begin: fold_partials_kernel's lane of
    // the weight sums them).  blocks == 0: the group pulls its list with pull_grad_kernel.
    struct BlockTable {
      U32x4 *d_ell = nullptr;
      uint32_t *d_tile0 = nullptr, *d_ov_start = nullptr;
      uint32_t blocks = 0, depth = 0, parts = 0;
      uint32_t tiles = 0;                 // tiles per block
      bool one_plane = false;             // one-plane packed rows: pull_ell1_kernel (else pull_ell_kernel)
    };
    std::vector<BlockTable> bp;           // [groups] or empty
    long long *d_bp_qtab = nullptr, *d_bp_partial = nullptr;   // shared: deltas; [max blocks][Wp] sums
    uint32_t bp_deltas = 0, bp_wp = 0;
    // a split plan's own weight-sorted layout: super-tiles cut ALONG its chunks, as many per chunk
    // as workgroups are resident, so that every chunk's launch of sorted_sweep_kernel is as wide as
    // the chip (the graph's default super-tiles of 64 tiles leave a quarter-sweep chunk 95 workgroups
    // for 256 CUs).  Empty: the chunks use the default layout (whole super-tiles inside a chunk).
    std::vector<SuperTile> sorted_supers;
    SuperTile *d_supers = nullptr;
    SortRec8 *d_sorted = nullptr;
    uint32_t *d_chunk_tiles = nullptr; // [2 * chunks]: the chunks' tile ranges (persist_learn8_kernel)
    bool layout_done = false;          // ensure_level_layout ran (whatever it decided)
    uint64_t sweeps = 0;               // learning sweeps run at this level (plan_layouts == 0: the layout comes after 2048)
    // a split sweep of this level as ONE graph launch (dwx_sample_sgd_async): the instantiated graph,
    // patched in place every sweep; use_graph < 0: replay failed once, the level stays on plain launches
    rt::graph_exec_t gexec = nullptr;
    int use_graph = 0;
    ~Level() {
      rt::graph_exec_destroy(gexec);
      rt::dfree(d_supers); rt::dfree(d_sorted); rt::dfree(d_chunk_tiles);
      rt::dfree(d_inc_wid); rt::dfree(d_inc_slot); rt::dfree(d_inc_d); rt::dfree(d_t_static);
      for (auto &t : bp) { rt::dfree(t.d_ell); rt::dfree(t.d_tile0); rt::dfree(t.d_ov_start); }
      rt::dfree(d_bp_qtab); rt::dfree(d_bp_partial);
    }
  };
  std::map<uint32_t, std::unique_ptr<Level>> levels;
  Level *plan_level = nullptr;        // level of the current plan
  bool plan_force_dynamic = false;    // dwx_sgd_plan_force_dynamic (multi-GPU agreement)
  uint32_t cur_chunk = 0;             // last chunk handed to dwx_sgd_accumulate_async
  uint8_t *d_w_fixed = nullptr;
  long long *d_grad = nullptr;
  // a split learning sweep of an all-unary graph with few weights as ONE persistent launch
  // (persist_learn8_kernel; opt-in, DWX_PERSIST=1: measured slower than the chunk-by-chunk launches):
  // grid (<= one workgroup per CU), its rows [2][grid][row_stride], the barrier words, LDS layout
  uint32_t persist_grid = 0, persist_row_stride = 0;
  long long *d_persist_rows = nullptr;
  uint32_t *d_persist_bar = nullptr;
  uint32_t persist_w64_off = 0, persist_red_off = 0;
  bool persist_check_pending = false;
  uint64_t persist_launches = 0;
  // ... and with one launch per mini-batch (sweep8_merged_kernel: the update as the next sweep kernel's
  // prologue): three gradient buffers ([0] = d_grad) and two weight buffers in turn
  bool merge_ok = false;
  long long *d_gbuf[3] = {nullptr, nullptr, nullptr};
  double *d_wbuf64[2] = {nullptr, nullptr};
  float *d_wbuf32[2] = {nullptr, nullptr};
  uint32_t merge_lw32_off = 0;
  uint64_t merged_sweeps = 0;
  int *d_grad32 = nullptr;              // dwx_grad_pack32_async: the gradient sums as 32-bit counts
  uint32_t *d_pack_bad = nullptr;       // ... and its "not a multiple / does not fit" counter
  bool pack_check_pending = false;
  KernelParams base{};
  uint64_t sweep = 0;
  uint64_t infer_sweeps = 0;  // inference sweeps since the last clear_tallies
  // kernel timing
  bool timing = false;
  uint64_t graph_launches = 0;        // split learning sweeps handed over as one graph launch
  std::vector<TimedSpan> spans;
  double t_ms[4] = {0, 0, 0, 0};   // [0] inference sweep kernels, [1] learning sweep kernels, [2] pull_grad, [3] flushes of deferred draws
  uint64_t t_launches[4] = {0, 0, 0, 0}, t_sweeps[4] = {0, 0, 0, 0};

  ~dwx_sampler() {
    for (auto &sp : spans) { rt::event_destroy(sp.a); rt::event_destroy(sp.b); rt::event_destroy(sp.c); }
    rt::dfree(d_v_meta); rt::dfree(d_v_orig); rt::dfree(d_v_row); rt::dfree(d_v_init);
    rt::dfree(d_row_ptr); rt::dfree(d_tiles); rt::dfree(d_giant); rt::dfree(d_wide); rt::dfree(d_bgiant); rt::dfree(d_bgiant_piece_off);
    rt::dfree(d_bgiant_decision); rt::dfree(d_bgiant_pieces); rt::dfree(d_bgiant_partial); rt::dfree(d_row_truth); rt::dfree(d_edge_fval64);
    rt::dfree(d_sorted); rt::dfree(d_supers); rt::dfree(d_sort_dvals);
    rt::dfree(d_grad32); rt::dfree(d_pack_bad);
    rt::dfree(d_edges); rt::dfree(d_edges8); rt::dfree(d_vifs); rt::dfree(d_assign_free); rt::dfree(d_assign_evid);
    rt::dfree(d_tally); rt::dfree(d_weights); rt::dfree(d_w32); rt::dfree(d_w_init); rt::dfree(d_terms); rt::dfree(d_delta);
    rt::dfree(d_pot); rt::dfree(d_rb); rt::dfree(d_trace); rt::dfree(d_w32_prev);
    rt::dfree(d_frecs); rt::dfree(d_fvifs); rt::dfree(d_ffval64); rt::dfree(d_fwide);
    rt::dfree(d_w_fixed); rt::dfree(d_grad); rt::dfree(d_persist_rows); rt::dfree(d_persist_bar);
    rt::dfree(d_gbuf[1]); rt::dfree(d_gbuf[2]); rt::dfree(d_wbuf64[0]); rt::dfree(d_wbuf64[1]); rt::dfree(d_wbuf32[0]); rt::dfree(d_wbuf32[1]);
    for (int i = 0; i < 2; ++i) { if (side[i]) rt::stream_destroy(side[i]); if (ev_join[i]) rt::event_destroy(ev_join[i]); }
    if (ev_fork) rt::event_destroy(ev_fork);
    if (stream) rt::stream_destroy(stream);
  }
};

// One side of a halo exchange with one peer: the device positions of the variables whose
// assignments travel, and the buffer they travel in ([chain][i], both chains' worth).
struct dwx_halo {
  dwx_sampler *s = nullptr;
  uint32_t n = 0;
  uint32_t bits = 32;       // per value: 1 (all boolean), 8 (cardinalities <= 256) or 32
  uint32_t block = 0;       // 8-byte words of one chain's block
  uint32_t *d_pos = nullptr;
  unsigned long long *d_buf = nullptr;
  ~dwx_halo() { rt::dfree(d_pos); rt::dfree(d_buf); }
};

namespace {
// d_w32 is about to change: the terms table and the potential cache are stale from here on
void weights_change(dwx_sampler *s) {
  s->terms_state = 0;
  std::fill(s->pot_valid.begin(), s->pot_valid.end(), (uint8_t)0);
}

// no giant, boolean-giant or wide tile: every variable is in a lane tile (the degree bins run kernels of their own)
bool no_binned_tiles(const dwx_sampler *s) {
  return s->cgiant_tiles.empty() && s->bgiant_tiles.empty() && s->cg->wide_tiles.empty();
}

// The sampler's builds of the tile sweep kernels at K records staged per lane and RP row pointers prefetched --
// the one place that names them; lds_infer / lds_learn: the dynamic LDS of the inference and the learning sweep.
// Compact-record graphs run sweep8_kernel and its kin, the others sweep_kernel's smallest build that holds their
// tile classes.  No learning kernel has an RB build.
template <int K, int RP>
void make_builds(dwx_sampler *s, size_t lds_infer, size_t lds_learn, size_t lds_tab) {
  SweepVariants &v = s->kv;
  if (s->rec8) {
    v.infer[0] = SweepVariant::eager(sweep8_kernel<false, K, false, RP>, lds_infer);
    v.infer[1] = v.infer[0].lazy(sweep8_kernel<false, K, false, RP, false, true>);
    v.multi[0][0] = v.infer[0].lazy(sweep8_kernel<false, K, false, RP, true>);
    v.multi[1][0] = v.infer[0].lazy(sweep8_kernel<false, K, false, RP, true, true>);
    v.multi[0][1] = v.infer[0].lazy(sweep8_kernel<false, K, false, RP, true, false, true>);
    v.multi[1][1] = v.infer[0].lazy(sweep8_kernel<false, K, false, RP, true, true, true>);
    v.learn = SweepVariant::eager(sweep8_kernel<true, K, false, RP>, lds_learn);
    // (the smaller size needs no allowance of its own, and setting one would lower the kernel's)
    v.learn_pull = v.learn;
    v.learn_pull.lds = lds_tab;
    v.learn_pull.cap = rt::resident_blocks(v.learn.fn, BLOCK_THREADS, lds_tab);
    v.tab[0] = SweepVariant::eager(sweep8_kernel<false, K, true, RP>, lds_tab);
    v.tab[1] = v.tab[0].lazy(sweep8_kernel<false, K, true, RP, false, true>);
    // (sized and allowed by dwx_sampler_create where the graph qualifies for them)
    v.merged[0].fn = sweep8_merged_kernel<K, RP>;
    v.merged[1].fn = sweep8_merged_kernel<K, RP, true>;
    v.persist.fn = persist_learn8_kernel<K, RP>;
  } else if (s->tv_pair) {
    // every tile pre-signed unary and / or inline arity-2 records (config 3b / 5b): the small build (K == 6)
    v.infer[0] = SweepVariant::eager(sweep_kernel<false, 6, false, TV_PAIR>, lds_infer);
    v.infer[1] = v.infer[0].lazy(sweep_kernel<false, 6, false, TV_PAIR, true>);
    v.learn = SweepVariant::eager(sweep_kernel<true, 6, true, TV_PAIR>, lds_learn);
  } else {
    v.infer[0] = SweepVariant::eager(sweep_kernel<false, K>, lds_infer);
    v.infer[1] = v.infer[0].lazy(sweep_kernel<false, K, false, TV_ALL, true>);
    v.learn = s->wide_learn ? SweepVariant::eager(sweep_kernel<true, K, true>, lds_learn)
                            : SweepVariant::eager(sweep_kernel<true, K>, lds_learn);
  }
}
void resolve_builds(dwx_sampler *s, size_t lds_infer, size_t lds_learn, size_t lds_tab) {
  constexpr int RP = (int)ROWPTR_UNROLL;
  if (s->rp_cat) make_builds<6, (int)ROWPTR_UNROLL_CAT>(s, lds_infer, lds_learn, lds_tab);
  else switch (s->stage_k) {
    case 3: make_builds<3, RP>(s, lds_infer, lds_learn, lds_tab); break;
    case 6: make_builds<6, RP>(s, lds_infer, lds_learn, lds_tab); break;
    default: make_builds<12, RP>(s, lds_infer, lds_learn, lds_tab); break;
  }
}

// launch the sweep kernel (+ the oversized-variable kernel) over tiles [t0, t1) of launch l
// multi (inference of a graph without degree-binned variables): P.n_sweeps sweeps per launch
// covered (if given): the end of the gap-free run of weight-sorted super-tiles that starts at t0 (t0: none)
// P.rb (inference only): the builds that add every draw's conditional to it (dwx_rb_enable)
// P.trace (multi only): the builds that write every sweep's draws to the sample trace (dwx_trace_enable)
// default_layout (learning): never the plan level's own super-tiles -- a launch over one side of the query end
template <bool LEARN>
uint32_t launch_tiles(dwx_sampler *s, KernelParams &P, size_t l, uint32_t t0, uint32_t t1, const bool multi = false,
                      uint32_t *covered = nullptr, const bool default_layout = false) {
  if (LEARN && (P.rb || multi)) throw std::logic_error("Rao-Blackwellised sums, several sweeps per launch: inference sweeps only");
  const bool rb = P.rb != nullptr, trace = multi && P.trace != nullptr;
  // (no learning kernel has an RB build: a learning launch names its plain build both times)
  constexpr bool RBK = !LEARN;
  const CompiledGraph &c = *s->cg;
  SweepVariants &kv = s->kv;
  if (covered) *covered = t0;
  if (t1 <= t0) return 0;
  uint32_t launches = 0;
  P.tile_begin = t0;
  P.tile_end = t1;
  // the oversized and mid-degree variables among these tiles (the lists are sorted by tile index)
  const auto &cgt = s->cgiant_tiles;
  const uint32_t cg0 = (uint32_t)(std::lower_bound(cgt.begin(), cgt.end(), t0) - cgt.begin());
  const uint32_t cg1 = (uint32_t)(std::lower_bound(cgt.begin(), cgt.end(), t1) - cgt.begin());
  const auto &bgt = s->bgiant_tiles;
  const uint32_t bg0 = (uint32_t)(std::lower_bound(bgt.begin(), bgt.end(), t0) - bgt.begin());
  const uint32_t bg1 = (uint32_t)(std::lower_bound(bgt.begin(), bgt.end(), t1) - bgt.begin());
  const uint32_t *wb = c.wide_tiles.data() + c.launch_wide[l], *we = c.wide_tiles.data() + c.launch_wide[l + 1];
  const uint32_t w0 = (uint32_t)(std::lower_bound(wb, we, t0) - c.wide_tiles.data());
  const uint32_t w1 = (uint32_t)(std::lower_bound(wb, we, t1) - c.wide_tiles.data());
  const bool any_giant = cg1 > cg0 || bg1 > bg0, any_wide = w1 > w0;
  // fork: the side streams start where `stream` stands now, beside the tiles' kernel
  // (learning launches only: an inference launch is too short -- the joins cost more than they hide)
  const bool fork = LEARN && s->ev_fork && (any_giant || any_wide);
  rt::stream_t st_giant = fork ? s->side[0] : s->stream, st_wide = fork ? s->side[1] : s->stream;
  if (fork) {
    rt::event_record(s->ev_fork, s->stream);
    if (any_giant) rt::stream_wait_event(st_giant, s->ev_fork);
    if (any_wide) rt::stream_wait_event(st_wide, s->ev_fork);
  }
  // the lane-bin tiles of [a, b): the persistent tile sweep
  auto launch_lane_tiles = [&](uint32_t a, uint32_t b) {
  if (b <= a) return;
  P.tile_begin = a;
  P.tile_end = b;
  // persistent grid: as many workgroups as stay resident, each striding over tiles
  // all-unary graph: 8-byte record stream (a run on the terms table streams those instead;
  // all-unary graphs stage 8-byte terms whenever the compute phase needs no record)
  const bool tab8 = s->rec8 && !LEARN && P.edge_terms;   // inference on the 8-byte terms table
  const bool slim = LEARN && s->rec8 && s->all_pull && !(P.flags & OPT_NO_PULL);
  // (multi: only asked for on compact-record graphs, never on the terms table)
  SweepVariant &k = multi ? kv.multi[rb][trace] : tab8 ? kv.tab[rb] : !LEARN ? kv.infer[rb] : slim ? kv.learn_pull : kv.learn;
  k.launch(std::min<unsigned>(b - a, k.cap), BLOCK_THREADS, s->stream, P);
  ++launches;
  };
  // Weight-sorted super-tiles lying wholly inside [t0, t1): sorted_sweep_kernel, one workgroup
  // each (not on the terms table: repeated inference gathers nothing; not when this sweep
  // scatters its gradient or counts updates dynamically -- the kernel only publishes ballots);
  // the tiles before, between and behind them: the tile sweep.
  bool used_sorted = false;
  if (s->d_supers && !P.edge_terms && !multi && (!LEARN || (s->sorted_learn && !(P.flags & (OPT_NO_PULL | OPT_DYNAMIC_T))))) {
    // (a chunk of a split learning sweep: the plan level's own layout, cut along the chunks; a learning
    // launch on the potential cache: the default layout, whose super-tiles end at the query tiles' end)
    const dwx_sampler::Level *lv =
        (LEARN && !P.pot && !default_layout && s->plan_level && s->plan_level->d_supers) ? s->plan_level : nullptr;
    const std::vector<SuperTile> &sv = lv ? lv->sorted_supers : c.supers;
    const SuperTile *d_sv = lv ? lv->d_supers : s->d_supers;
    const SortRec8 *d_sr = lv ? lv->d_sorted : s->d_sorted;
    size_t a = std::lower_bound(sv.begin(), sv.end(), t0, [](const SuperTile &x, uint32_t t) { return x.tile0 < t; }) - sv.begin();
    size_t b = a;
    while (b < sv.size() && sv[b].tile0 + sv[b].ntiles <= t1) ++b;
    // gap-free runs of super-tiles
    struct Run { size_t a, b; };
    std::vector<Run> runs;
    for (size_t i = a; i < b;) {
      size_t j = i + 1;
      while (j < b && sv[j].tile0 == sv[j - 1].tile0 + sv[j - 1].ntiles) ++j;
      runs.push_back({i, j});
      i = j;
    }
    if (runs.size() > 8 && !s->sorted_fallback_said) {
      // (this used to be silent) ineligible tiles -- wave / workgroup bins, categorical rows --
      // interleave with the eligible ones: the launch falls back to the tile sweep, said once per sampler
      s->sorted_fallback_said = true;
      fprintf(stderr, "dwx: a launch's weight-sorted super-tiles form %zu gap-free runs (more than 8): its tiles take "
                      "the plain tile sweep (slower weight gathers)\n", runs.size());
    }
    if (!runs.empty() && runs.size() <= 8) {
      used_sorted = true;
      if (covered && sv[runs[0].a].tile0 == t0) *covered = sv[runs[0].b - 1].tile0 + sv[runs[0].b - 1].ntiles;
      uint32_t cursor = t0;
      for (const Run &r : runs) {
        launch_lane_tiles(cursor, sv[r.a].tile0);
        // learning on the potential cache: the cached super-tiles (the query tiles, at the head of the run)
        // cost a fraction of the streamed ones; the launch starts behind them so that they fill the tail
        // of the streamed super-tiles' last round (DWX_POT_QUERY_FIRST: in tile order)
        P.super_rot = 0;
        if (LEARN && P.pot) {
          uint32_t n_cached = 0;
          for (size_t i = r.a; i < r.b; ++i)
            if (sv[i].v0 >= P.pot_v0 && sv[i].v0 + sv[i].nv <= P.pot_v1) ++n_cached;
          s->pot_supers += n_cached;
          if (!s->pot_query_first && n_cached < r.b - r.a && sv[r.a].v0 >= P.pot_v0 && sv[r.a].v0 + sv[r.a].nv <= P.pot_v1)
            P.super_rot = n_cached;   // (cached ones lead the run: the range is the launch's first tiles)
        }
        // (one distinct d: the UNI build keeps it in a scalar register; DWX_NO_SORT_UNI: A/B knob)
        const bool uni = s->n_sort_dvals == 2 && !s->no_sort_uni;
        (LEARN ? kv.sorted_learn[uni] : kv.sorted_infer[uni][rb])
            .launch((unsigned)(r.b - r.a), SORT_THREADS, s->stream, P, (const SuperTile *)(d_sv + r.a), (uint32_t)(r.b - r.a), d_sr,
                    (const double *)s->d_sort_dvals, s->n_sort_dvals);
        ++launches;
        P.super_rot = 0;
        cursor = sv[r.b - 1].tile0 + sv[r.b - 1].ntiles;
      }
      launch_lane_tiles(cursor, t1);
    }
  }
  if (!used_sorted) launch_lane_tiles(t0, t1);
  P.tile_begin = t0;
  P.tile_end = t1;
  // categorical oversized variables: a workgroup each
  if (cg1 > cg0) {
    rt::launch(rb ? giant_kernel<LEARN, RBK> : giant_kernel<LEARN>, cg1 - cg0, GIANT_THREADS, 0, st_giant, P,
               (const uint32_t *)(s->d_giant + cg0), cg1 - cg0);
    ++launches;
  }
  // boolean: the pieces' partial potentials, the decisions, (learning) the pieces' gradients
  if (bg1 > bg0) {
    const uint32_t p0 = s->bgiant_piece_off[bg0], np = s->bgiant_piece_off[bg1] - p0;
    rt::launch(giant_pot_kernel<LEARN>, np, GIANT_THREADS, 0, st_giant, P, (const uint32_t *)s->d_bgiant,
               (const GiantPiece *)s->d_bgiant_pieces, p0, np, s->d_bgiant_partial);
    rt::launch(rb ? giant_decide_kernel<LEARN, RBK> : giant_decide_kernel<LEARN>, (bg1 - bg0 + BLOCK_THREADS - 1) / BLOCK_THREADS,
               BLOCK_THREADS, 0, st_giant, P, (const uint32_t *)s->d_bgiant, (const uint32_t *)s->d_bgiant_piece_off, bg0, bg1 - bg0,
               (const double *)s->d_bgiant_partial, s->d_bgiant_decision);
    launches += 2;
    if (LEARN) {
      rt::launch(giant_grad_kernel, np, GIANT_THREADS, 0, st_giant, P, (const uint32_t *)s->d_bgiant,
                 (const GiantPiece *)s->d_bgiant_pieces, p0, np, (const uint32_t *)s->d_bgiant_decision);
      ++launches;
    }
  }
  // mid-degree variables among these tiles: a wave each
  if (w1 > w0) {
    const uint32_t per_block = BLOCK_THREADS / 64u;
    rt::launch(rb ? wide_kernel<LEARN, RBK> : wide_kernel<LEARN>, (w1 - w0 + per_block - 1) / per_block, BLOCK_THREADS, 0,
               st_wide, P, (const uint32_t *)(s->d_wide + w0), w1 - w0);
    ++launches;
  }
  // join: whatever follows on `stream` (the next colour, the pull gradient, an update) waits for all three
  if (fork) {
    if (any_giant) { rt::event_record(s->ev_join[0], st_giant); rt::stream_wait_event(s->stream, s->ev_join[0]); }
    if (any_wide) { rt::event_record(s->ev_join[1], st_wide); rt::stream_wait_event(s->stream, s->ev_join[1]); }
  }
  return launches;
}

// n inference sweeps of a graph whose sweeps can share a launch: compact records (all-unary, so
// no variable reads another and the potentials of a variable are the same in every sweep while
// the weights rest) and no degree-binned variable (wide / giant tiles run kernels of their own).
// ONE launch of the gathering tile sweep stages every tile once and draws n times per variable
// (sweep8_kernel<..., MULTI>, infer_variable_multi): neither the terms table nor the weight-sorted
// copy is needed -- a record is read once per n sweeps.
bool multi_sweep_graph(const dwx_sampler *s) {
  return s->rec8 && no_binned_tiles(s) && !getenv("DWX_NO_MULTI_SWEEP");
}

// Sample trace: pack the inference chain's current assignment into n_planes planes of the ring from trace_next on
// (unsampled_only: only the positions inference sweeps do not draw, the others cleared -- the planes a one-launch
// run is about to fill), and enter sweeps [first_id, first_id + n_planes) as the ring's newest entries.
void flush_pending(dwx_sampler *s, int chains = 3);
void trace_pack(dwx_sampler *s, uint64_t first_id, uint32_t n_planes, bool unsampled_only) {
  const CompiledGraph &c = *s->cg;
  // (deferred draws: the callers pack behind an inference sweep, which has rewritten the evidence chain of every
  // query variable, or the unsampled positions only -- neither reads an owed value; any other use flushes)
  if (!unsampled_only) flush_pending(s, 2);
  const uint32_t n = (uint32_t)c.Vo;
  if (n) {
    const uint32_t items = s->trace_bits == 1 ? n : (n + 3u) / 4u;
    const unsigned grid = std::min<unsigned>((items + BLOCK_THREADS - 1) / BLOCK_THREADS, 256u * 16u);
    auto go = [&](auto kernel) {
      rt::launch(kernel, grid, BLOCK_THREADS, 0, s->stream, (const uint32_t *)s->d_assign_evid, (const uint32_t *)s->d_v_meta,
                 n, unsampled_only ? 1u : 0u, s->opts.sample_evidence ? 1u : 0u, s->d_trace, s->trace_words, s->trace_cap,
                 s->trace_next, n_planes);
    };
    if (s->trace_bits == 1) go(trace_pack_kernel<1>); else go(trace_pack_kernel<8>);
  }
  for (uint32_t j = 0; j < n_planes; ++j) {
    s->trace_ids[s->trace_next] = first_id + j;
    s->trace_next = s->trace_next + 1 == s->trace_cap ? 0 : s->trace_next + 1;
    s->trace_count = std::min(s->trace_count + 1, s->trace_cap);
  }
}

// Kernel timing (dwx_options timing): a span's event a goes on the stream where it opens ...
TimedSpan span_begin(dwx_sampler *s, int kind) {
  TimedSpan sp{};
  if (s->timing) {
    sp.a = rt::event_create(); sp.b = rt::event_create(); sp.c = rt::event_create(); sp.kind = kind;
    rt::event_record(sp.a, s->stream);
  }
  return sp;
}
// ... and b and c where it closes (b_recorded: the caller put b between its sweep kernels and its pull gradient)
void span_end(dwx_sampler *s, TimedSpan &sp, uint32_t launches, bool has_pull, bool new_sweep, uint32_t n_sweeps = 1,
              bool b_recorded = false) {
  if (!s->timing) return;
  if (!b_recorded) rt::event_record(sp.b, s->stream);
  rt::event_record(sp.c, s->stream);
  sp.launches = launches; sp.has_pull = has_pull; sp.new_sweep = new_sweep; sp.n_sweeps = n_sweeps;
  s->spans.push_back(sp);
}

// Deferred draws.  The query draws a learning sweep left out, run now if a chain in `chains`
// (bit 0 free, bit 1 evidence) still holds an earlier sweep's values: the learning kernels over the query tiles of
// every colour launch, with the sweep counter and the weights of that sweep -- the potential cache where it still
// holds the sums those weights give, else the records streamed against the snapshot of d_w32 -- and no gradient
// work (query variables trigger none).  Every reader and writer of the two arrays calls this first.
void flush_pending(dwx_sampler *s, int chains) {
  dwx_sampler::Pending &pd = s->pending;
  if (!(((pd.owed ? 1 : 0) | (pd.evid_owed ? 2 : 0)) & chains)) return;
  rt::set_device(s->device);
  const CompiledGraph &c = *s->cg;
  KernelParams P = s->base;
  P.sweep = pd.sweep;
  P.w32 = pd.snap ? s->d_w32_prev : s->d_w32;
  if (!pd.evid_owed) P.flags |= OPT_FREE_CHAIN_ONLY;   // (an inference sweep has drawn that chain since)
  TimedSpan sp = span_begin(s, 3);
  uint32_t launches = 0;
  for (size_t l = 0; l + 1 < c.launch_off.size(); ++l) {
    KernelParams Q = P;
    if (l < pd.cached.size() && pd.cached[l]) {
      Q.pot = s->d_pot;
      Q.pot_v0 = c.tile_v[c.launch_tile[l]];
      Q.pot_v1 = c.tile_v[c.launch_query_tile_end[l]];
    }
    launches += launch_tiles<true>(s, Q, l, c.launch_tile[l], c.launch_query_tile_end[l], false, nullptr, true);
  }
  span_end(s, sp, launches, false, false);
  pd.owed = pd.evid_owed = false;
  ++s->flushes;
}

// a learning sweep draws (or defers) both chains of every query variable itself: nothing older is owed
void drop_pending(dwx_sampler *s) { s->pending.owed = s->pending.evid_owed = false; }

// d_w32 is about to be rewritten by something other than apply_kernel (which saves the old values itself): if draws
// are owed under the weights it holds now, they move to d_w32_prev first
void keep_snapshot(dwx_sampler *s) {
  dwx_sampler::Pending &pd = s->pending;
  if (!pd.owed || pd.snap) return;
  rt::d2d(s->d_w32_prev, s->d_w32, ((size_t)s->cg->W + 1) * sizeof(float), s->stream);
  pd.snap = true;
}

void enqueue_inference_multi(dwx_sampler *s, uint32_t n) {
  const CompiledGraph &c = *s->cg;
  rt::set_device(s->device);
  KernelParams P = s->base;
  P.sweep = s->sweep;
  P.n_sweeps = n;
  P.edge_terms = nullptr;
  P.rb = s->rb_on ? s->d_rb : nullptr;
  s->pending.evid_owed = false;   // (deferred draws: these sweeps overwrite every query variable's evidence chain)
  TimedSpan sp = span_begin(s, 0);
  uint32_t launches = 0;
  // the sample trace: the last min(n, capacity) sweeps of the launch write their planes themselves
  // (sweep8_kernel<MULTI, TRACE>), over what trace_pack_kernel leaves there: the unsampled positions' values
  P.trace = nullptr;
  if (s->trace_on) {
    const uint32_t m = std::min(n, s->trace_cap);
    P.trace = s->d_trace; P.trace_words = s->trace_words; P.trace_cap = s->trace_cap; P.trace_bits = s->trace_bits;
    P.trace_slot0 = s->trace_next; P.trace_skip = n - m;
    trace_pack(s, s->sweep + (n - m), m, true);
    ++launches;
  }
  for (size_t l = 0; l + 1 < c.launch_off.size(); ++l) {
    const uint32_t t0 = c.launch_tile[l];
    const uint32_t t1 = s->opts.sample_evidence ? c.launch_tile[l + 1] : c.launch_query_tile_end[l];
    launches += launch_tiles<false>(s, P, l, t0, t1, true);
  }
  span_end(s, sp, launches, false, true, n);
  s->sweep += n;
}

// The potential cache's array, allocated on first use: compact-record graphs whose learning sweeps take
// the weight-sorted super-tiles.  false: this sampler runs without it (not eligible, DWX_NO_POT_CACHE, or
// no device memory for it even after the OOM hook).
bool pot_cache_ready(dwx_sampler *s) {
  if (s->pot_alloc == 0) {
    const CompiledGraph &c = *s->cg;
    s->pot_alloc = -1;
    if (s->rec8 && s->d_supers && s->sorted_learn && !getenv("DWX_NO_POT_CACHE")) {
      s->d_pot = (long long *)optional_dmalloc(c.V * sizeof(long long));
      if (s->d_pot) {
        s->pot_alloc = 1;
        s->pot_valid.assign(c.launch_tile.size(), 0);
      }
    }
  }
  return s->pot_alloc > 0;
}

// one inference sweep (GibbsSampler::sample)
void enqueue_inference(dwx_sampler *s) {
  const CompiledGraph &c = *s->cg;
  rt::set_device(s->device);
  KernelParams P = s->base;
  P.sweep = s->sweep;
  P.rb = s->rb_on ? s->d_rb : nullptr;
  s->last_infer = true;
  // The second consecutive inference sweep on the same weights tabulates the pre-signed
  // records' potential terms (one extra pass, about the cost of a sweep); from then on
  // sweeps stream the table and gather no weights.  (Not on the first one: learning and
  // inference sweeps may alternate, and then the table would be rebuilt for a single use.)
  if (s->has_simple_tiles && s->terms_state == 1 && c.NIdx) {
    const unsigned grid = std::min<unsigned>((unsigned)c.tiles.size(), 256u * 16u);
    if (s->rec8) {   // all-unary graph: the 8-byte table
      if (!s->d_terms) s->d_terms = (EdgeTerms *)rt::dmalloc(c.NIdx * 8);
      rt::launch(build_terms8_kernel, grid, BLOCK_THREADS, 0, s->stream, (const EdgeRec8 *)s->d_edges8,
                 (uint64_t)c.NIdx, (const float *)s->d_w32, (unsigned long long *)s->d_terms);
    } else {
      if (!s->d_terms) s->d_terms = (EdgeTerms *)rt::dmalloc(c.NIdx * sizeof(EdgeTerms));
      rt::launch(build_terms_kernel, grid, BLOCK_THREADS, 0, s->stream, (const TileDesc *)s->d_tiles,
                 (uint32_t)c.tiles.size(), (const EdgeRec *)s->d_edges, (const float *)s->d_w32, s->d_terms);
    }
    s->terms_state = 2;
  }
  P.edge_terms = s->terms_state == 2 ? s->d_terms : nullptr;
  if (s->terms_state == 0) s->terms_state = 1;
  // the potential cache is stored once a learning sweep is known to follow inference sweeps (on a
  // sampler that only infers, it would be bandwidth spent for nothing -- the rule of the terms table)
  P.pot = (s->pot_wanted && !P.edge_terms && pot_cache_ready(s)) ? s->d_pot : nullptr;
  // deferred draws: this sweep overwrites the evidence chain of every query variable, and where it stores into
  // the potential cache, the sums an owed draw would have read
  s->pending.evid_owed = false;
  if (P.pot) std::fill(s->pending.cached.begin(), s->pending.cached.end(), (uint8_t)0);
  TimedSpan sp = span_begin(s, 0);
  uint32_t launches = 0;
  for (size_t l = 0; l + 1 < c.launch_off.size(); ++l) {
    // only the query variables' tiles unless --sample_evidence (src/gibbs_sampler.h:157)
    const uint32_t t1 = s->opts.sample_evidence ? c.launch_tile[l + 1] : c.launch_query_tile_end[l];
    uint32_t covered = 0;
    launches += launch_tiles<false>(s, P, l, c.launch_tile[l], t1, false, &covered);
    // valid for launch l only if sorted_sweep_kernel stored the sum of EVERY query tile (none took the
    // tile sweep, the terms table or a degree-bin kernel)
    if (P.pot && c.launch_query_tile_end[l] > c.launch_tile[l] && covered >= c.launch_query_tile_end[l]) s->pot_valid[l] = 1;
  }
  // the sample trace: one pass over the assignment the sweep left, whatever kernels it took
  if (s->trace_on) {
    trace_pack(s, s->sweep, 1, false);
    ++launches;
  }
  span_end(s, sp, launches, false, true);
  ++s->sweep;
}

// A plan level's own weight-sorted layout (Level::sorted_supers): for a split plan cut ALONG its
// chunks, as many super-tiles per chunk as workgroups are resident; for an un-split sweep, where a
// launch holds query AND evidence tiles, one run per launch -- the default layout cuts those apart
// (an inference sweep launches over the query part only), so a learning launch over it ends two
// runs with a round of small super-tiles each (config 3: learning sweep 0.288 -> 0.269 ms with one).
// Worth it while a chunk still makes super-tiles of 8 tiles and more.  Costs 0.3 s of host time
// and a second copy of the records: dwx_options.plan_layouts says when it is built.
void ensure_level_layout(dwx_sampler *s, dwx_sampler::Level *L, uint32_t batches) {
  if (L->layout_done) return;
  // (deferred draws: an un-split sweep launches over the evidence tiles alone, which the default layout serves
  // whole -- no layout unless the caller asked for one with the level, plan_layouts == 1; not marked done: a sampler
  // whose deferral ends wants it after all)
  if (batches == 1 && s->defer_ok && s->opts.plan_layouts != 1) return;
  L->layout_done = true;
  const CompiledGraph &c = *s->cg;
  bool mixed_launch = false;
  for (size_t l = 0; l + 1 < c.launch_tile.size(); ++l)
    mixed_launch = mixed_launch || (c.launch_query_tile_end[l] > c.launch_tile[l] && c.launch_query_tile_end[l] < c.launch_tile[l + 1]);
  if (!(batches > 1 || mixed_launch) || c.supers.empty() || !s->sorted_learn || L->chunks.empty()) return;
  uint64_t tiles_in_chunks = 0;
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  for (const auto &ch : L->chunks) { ranges.push_back({ch.t0, ch.t1}); tiles_in_chunks += ch.t1 - ch.t0; }
  if (tiles_in_chunks / L->chunks.size() < 8ull * c.sorted_slots) return;
  rt::set_device(s->device);
  SortedLayout lay;
  const bool on_device = build_on_device();
  build_sorted_layout(c, ranges, c.sorted_per_super, c.sorted_slots, batches == 1, host_threads(), lay, on_device);
  if (lay.supers.empty()) return;
  SortRec8 *d_sorted = nullptr;
  SuperTile *d_supers = nullptr;
  if (on_device) {
    // (the records sit at their super-tiles' planned offsets whatever the order of the descriptors)
    d_supers = upload(lay.supers, s->stream);
    d_sorted = (SortRec8 *)rt::dmalloc((lay.n + 1) * sizeof(SortRec8));
    rt::dmemset(d_sorted + lay.n, 0, sizeof(SortRec8), s->stream);
    devb::build_sorted_records(s->d_tiles, s->d_edges, s->d_edges8, d_supers, (uint32_t)lay.supers.size(),
                               c.sort_dbits.data(), (uint32_t)c.sort_dbits.size(), lay.n, d_sorted, (void *)s->stream);
    rt::dfree(d_supers);
  }
  // (launch_tiles looks super-tiles up by their first tile: ascending, like the default layout)
  std::sort(lay.supers.begin(), lay.supers.end(), [](const SuperTile &a, const SuperTile &b) { return a.tile0 < b.tile0; });
  if (!on_device) d_sorted = upload(lay.recs, s->stream, 1);
  d_supers = upload(lay.supers, s->stream);
  rt::stream_sync(s->stream);   // (the host copies die with this scope; the sweeps queued so far used the default layout)
  L->sorted_supers.swap(lay.supers);
  L->d_sorted = d_sorted;
  L->d_supers = d_supers;
}

// Everything a plan level needs to run its chunks without per-record atomics: per chunk,
// (a) the static update counts of its boolean variables -- a boolean variable that triggers
// SGD visits every factor of its row once with t = 1 (src/factor_graph.cc:265-273),
// independent of the samples drawn -- and (b) the pull-gradient incidence list of its
// TILE_PULL tiles: every (triggering variable, non-fixed record) pair, sorted by weight
// (two stable parallel counting sorts: by weight, then by chunk).
dwx_sampler::Level *build_level(dwx_sampler *s, uint32_t batches) {
  auto it = s->levels.find(batches);
  if (it != s->levels.end()) return it->second.get();
  rt::set_device(s->device);
  const CompiledGraph &c = *s->cg;
  const dwx_options &o = s->opts;
  std::unique_ptr<dwx_sampler::Level> L(new dwx_sampler::Level());
  // The pieces of a split sweep are visited ROUND-ROBIN over the colour launches, piece b of n
  // at position (b + 1/2) / n of the sweep: any order of independent sets is a Gibbs scan, and
  // the reference's scan in id order meets the colours interleaved, not one after the other --
  // with heavily tied weights the weights at the end of a sweep are those the LAST visits want,
  // and a colour can be a biased sample of the model (the observed middle variables of a chain
  // a - b - c: tests/golden tied_chain; the reference itself run on the colour-major relabelling
  // of that graph learns 0.87 .. 1.0 in its first epoch against 0.34 .. 0.52 in id order).
  {
    struct Piece { double at; dwx_sampler::Chunk ch; };
    std::vector<Piece> pieces;
    for (size_t l = 0; l + 1 < c.launch_off.size(); ++l) {
      const std::vector<uint32_t> cut = cut_launch(c, s->sgd_work, s->sgd_work_max_launch, l, batches);
      const size_t n = cut.size() - 1;
      for (size_t b = 0; b < n; ++b)
        pieces.push_back({((double)b + 0.5) / (double)n, {(uint32_t)l, cut[b], cut[b + 1]}});
    }
    std::stable_sort(pieces.begin(), pieces.end(), [](const Piece &a, const Piece &b) { return a.at < b.at; });
    for (const Piece &pc : pieces) L->chunks.push_back(pc.ch);
  }
  // DWX_TIMING=1: wall time of the level's build steps on stderr (each ends on a stream sync)
  const bool lv_timing = getenv("DWX_TIMING") != nullptr;
  auto lv_t0 = std::chrono::steady_clock::now();
  auto lv_step = [&](const char *what) {
    if (!lv_timing) return;
    rt::stream_sync(s->stream);
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[dwx level B=%u] %-28s %.3f s\n", batches, what, std::chrono::duration<double>(t - lv_t0).count());
    lv_t0 = t;
  };
  lv_step("chunks");
  {
    // before any table is summed: the groups of variables that share an update (the un-split sweep:
    // ONE, whatever its colour launches) must keep every weight's sums inside int64
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    if (batches == 1) groups.push_back({c.tile_v.front(), c.tile_v.back()});
    else for (const auto &ch : L->chunks) groups.push_back({c.tile_v[ch.t0], c.tile_v[ch.t1]});
    L->range_error = learning_range_error(c, o, groups);
    lv_step("range of the learning sums");
    if (!L->range_error.empty()) {
      dwx_sampler::Level *ret = L.get();
      s->levels[batches] = std::move(L);
      return ret;
    }
  }
  const bool on_device = build_on_device();
  // (plan_layouts 0, the default: with the level wherever the records are sorted on the device -- it
  // costs milliseconds there; a host build pays 0.3 s per level and waits for 2048 sweeps)
  if (s->opts.plan_layouts == 1 || (s->opts.plan_layouts == 0 && on_device)) ensure_level_layout(s, L.get(), batches);
  lv_step("weight-sorted layout");
  // beyond this the per-chunk tables cost more than they save: such plans keep the
  // per-record atomics and dynamic counts
  uint32_t table_chunks = 4 * MAX_PLAN_BATCHES;
  uint64_t min_w = 131072, bp_tiles = 0;   // (fewer weights: the list pull is as fast, tools/tied_sweep.py; 0: the row format's block size)
  bool one_plane_ok = true;                // DWX_BP_TWO_PLANES=1: one-delta tables keep both ballot planes (A/B runs, tests)
  if (const char *e = getenv("DWX_PLAN_TABLE_CHUNKS")) table_chunks = (uint32_t)std::max(1L, atol(e));   // test hooks
  if (const char *e = getenv("DWX_BLOCK_PULL_MIN_W")) min_w = (uint64_t)std::max(0L, atol(e));
  if (const char *e = getenv("DWX_BLOCK_PULL_TILES")) bp_tiles = (uint64_t)std::max(1L, atol(e));   // (capped per format: bp_block_tiles)
  if (const char *e = getenv("DWX_BP_TWO_PLANES")) one_plane_ok = atol(e) == 0;
  const uint32_t n_chunks = (uint32_t)L->chunks.size();
  L->fast = n_chunks >= 1 && n_chunks <= table_chunks && (uint64_t)n_chunks * c.W * 16 <= ((uint64_t)2 << 30);
  if (batches == 1) L->fast = true;
  if (L->fast && c.W) {
    // groups of the tables: the chunks of a split sweep (an update follows each of them); ONE
    // group for an un-split sweep, whatever its number of colour launches (one update at the end)
    std::vector<hostb::TileGroup> groups;
    if (batches == 1) groups.push_back({0u, (uint32_t)c.tiles.size()});
    else for (const auto &ch : L->chunks) groups.push_back({ch.t0, ch.t1});
    const uint32_t nc = (uint32_t)groups.size();
    // (a) the static tables, one row pair [T[W] | h[W]] per group, and (b) the pull gradient's incidence list
    // and block tables: built on the device (device_build.hip), or on the host (level_build.cc) and uploaded
    // -- the same structures bit for bit
    L->rows = nc;
    long long tm = 0, hm = 0;
    devb::Incidence inc;
    if (on_device) {
      std::vector<uint32_t> group_of(c.tiles.size(), 0xFFFFFFFFu), tile_info(c.tiles.size(), 0xFFFFFFFFu);
      for (uint32_t k = 0; k < nc; ++k)
        for (uint32_t t = groups[k].t0; t < groups[k].t1; ++t) group_of[t] = k;
      L->d_t_static = (long long *)rt::dmalloc((size_t)nc * 2 * c.W * 8);
      devb::build_static_tables(s->d_tiles, (uint32_t)c.tiles.size(), group_of.data(), s->d_v_meta, s->d_v_row, s->d_row_ptr,
                                s->d_edges, s->d_edge_fval64, (const uint8_t *)s->d_w_fixed, (uint32_t)c.W, nc,
                                o.learn_non_evidence != 0, o.noise_aware != 0, L->d_t_static, &tm, &hm, (void *)s->stream);
      lv_step("static tables (device)");
      for (size_t ti = 0; ti < c.tiles.size(); ++ti) {
        const TileDesc &td = c.tiles[ti];
        const bool unary_only = !(td.flags & TILE_PULL) && (td.flags & TILE_PULL_UNARY) && c.ecap <= 6 * BLOCK_THREADS;
        if ((!(td.flags & TILE_PULL) && !unary_only) || (td.flags & TILE_OUTSIDE)) continue;
        tile_info[ti] = group_of[ti] | ((unary_only ? 2u : 1u) << 30);   // (the groups cover every tile: the launches do)
      }
      inc.d_v_init = one_plane_ok ? s->d_v_init : nullptr;   // (input: the signs of one-plane rows)
      devb::build_incidence(s->d_tiles, c.tiles.data(), (uint32_t)c.tiles.size(), tile_info.data(), s->d_v_meta, s->d_v_row,
                            s->d_row_ptr, s->d_edges, o.learn_non_evidence != 0, o.noise_aware != 0, (uint32_t)c.W, nc,
                            min_w, (uint32_t)std::min<uint64_t>(bp_tiles, BP1_TILES), inc, (void *)s->stream);
    } else {
      RawArray<long long> ts;
      hostb::build_static_tables(c, o, groups, ts, &tm, &hm);
      L->d_t_static = upload(ts, s->stream);
      rt::stream_sync(s->stream);
      ts.clear();
      lv_step("static tables (host)");
      hostb::Incidence h;
      hostb::build_incidence(c, o, groups, min_w, bp_tiles, one_plane_ok, h);
      inc.inc_begin = h.inc_begin; inc.inc_end = h.inc_end;
      inc.dvals = h.dvals; inc.max_blocks = h.max_blocks; inc.wp = h.wp;
      try {
        if (h.inc_wid.size()) {
          inc.d_inc_wid = upload(h.inc_wid, s->stream);
          inc.d_inc_slot = upload(h.inc_slot, s->stream);
          inc.d_inc_d = upload(h.inc_d, s->stream);
        }
        inc.bp.resize(h.bp.size());
        for (size_t k = 0; k < h.bp.size(); ++k) {
          if (!h.bp[k].blocks) continue;
          devb::Incidence::BlockTable &bt = inc.bp[k];
          bt.d_ell = (U32x4 *)upload(h.bp[k].ell, s->stream);
          const std::vector<uint32_t> ovs32(h.bp[k].ov_start.begin(), h.bp[k].ov_start.end());   // (< 2^32: the whole list is)
          bt.d_ov_start = upload(ovs32, s->stream);
          bt.tile0 = h.bp[k].tile0;
          bt.blocks = h.bp[k].blocks; bt.depth = h.bp[k].depth; bt.total = h.bp[k].total; bt.on_list = h.bp[k].on_list;
          bt.tiles = h.bp[k].tiles; bt.one_plane = h.bp[k].one_plane;
          rt::stream_sync(s->stream);   // (ovs32 dies with this scope, and the group's rows at once)
          h.bp[k].ell.clear();
        }
        rt::stream_sync(s->stream);     // (the host columns and rows die with this scope)
      } catch (...) {
        rt::dfree(inc.d_inc_wid); rt::dfree(inc.d_inc_slot); rt::dfree(inc.d_inc_d);
        for (auto &t : inc.bp) { rt::dfree(t.d_ell); rt::dfree(t.d_ov_start); }
        throw;
      }
    }
    // the level adopts the structures, whoever built them
    L->c_max = (double)hm / H_SCALE; L->t_max = (double)tm / FIX_SCALE;
    L->d_inc_wid = inc.d_inc_wid; L->d_inc_slot = inc.d_inc_slot; L->d_inc_d = inc.d_inc_d;
    L->inc_begin = inc.inc_begin; L->inc_end = inc.inc_end;
    L->bp.resize(inc.bp.size());
    for (size_t k = 0; k < inc.bp.size(); ++k) { L->bp[k].d_ell = inc.bp[k].d_ell; L->bp[k].d_ov_start = inc.bp[k].d_ov_start; }
    lv_step(on_device ? "incidence list (device)" : "incidence list (host)");
    if (!inc.bp.empty()) {
      const bool packed = inc.dvals.size() == 1;   // one delta: three 19-bit slots per 8-byte word
      for (uint32_t k = 0; k < nc; ++k) {
        if (!inc.bp[k].blocks) continue;
        dwx_sampler::Level::BlockTable &bt = L->bp[k];
        bt.d_tile0 = upload(inc.bp[k].tile0, s->stream);
        bt.blocks = inc.bp[k].blocks; bt.depth = inc.bp[k].depth;
        bt.tiles = inc.bp[k].tiles; bt.one_plane = inc.bp[k].one_plane;
        // parts per block: one workgroup per CU over all blocks (it owns the CU's whole LDS)
        bt.parts = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(rt::cu_count() / bt.blocks, inc.wp / BP_THREADS));
        if (lv_timing)
          fprintf(stderr, "[dwx block pull] group %u: %u blocks x depth %u (%u entries, %llu bytes of rows), %zu deltas, %llu of %llu entries on the list (%s build), %s rows, %u tiles per block\n",
                  k, bt.blocks, bt.depth, bt.depth * (packed ? BP_PK_ROW : BP_ROW),
                  (unsigned long long)((uint64_t)bt.blocks * bt.depth * inc.wp * (packed ? 8 : 16)), inc.dvals.size(),
                  (unsigned long long)inc.bp[k].on_list, (unsigned long long)inc.bp[k].total, on_device ? "device" : "host",
                  bt.one_plane ? "one-plane" : packed ? "two-plane" : "16-byte", bt.tiles);
      }
      std::vector<long long> qtab(inc.dvals.size());
      for (size_t i = 0; i < inc.dvals.size(); ++i) {
        float d; std::memcpy(&d, &inc.dvals[i], 4);
        qtab[i] = std::llrint(FIX_SCALE * (double)d);
      }
      L->d_bp_qtab = upload(qtab, s->stream);
      L->d_bp_partial = (long long *)rt::dmalloc(inc.max_blocks * inc.wp * 8);
      L->bp_deltas = (uint32_t)inc.dvals.size(); L->bp_wp = (uint32_t)inc.wp;
      rt::allow_dynamic_lds(pull_ell_kernel<1, false>, BP_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell_kernel<2, false>, BP_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell_kernel<1, true, true>, BP_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell_kernel<2, true, true>, BP_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell_kernel<3, true, true>, BP_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell_kernel<4, true, true>, BP_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell1_kernel<1>, BP1_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell1_kernel<2>, BP1_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell1_kernel<3>, BP1_LDS_BYTES);
      rt::allow_dynamic_lds(pull_ell1_kernel<4>, BP1_LDS_BYTES);
    }
    rt::stream_sync(s->stream);   // (qtab and the tile0 lists die with this scope)
  }
  dwx_sampler::Level *out = L.get();
  s->levels[batches] = std::move(L);
  return out;
}

// Curvature of one SGD mini-batch in weight space, when every colour launch is cut into `batches` runs
// of tiles: the largest eigenvalue lambda of the batch Hessian bound (hostb::batch_curvature,
// devb::batch_curvature) decides whether ONE batched step tracks the reference's sequential updates
// (stepsize * lambda < 2).  Estimated per chunk, times a safety factor; the result is the max over chunks.
double row_sum_bound(dwx_sampler *s, uint32_t batches) {
  auto it = s->row_sum_cache.find(batches);
  if (it != s->row_sum_cache.end()) return it->second;
  const CompiledGraph &c = *s->cg;
  const bool on_device = build_on_device();
  if (on_device) rt::set_device(s->device);
  devb::CurvatureScratch dev_sc;      // (the vectors of either estimate, kept over the chunks)
  hostb::CurvatureScratch host_sc;
  double lam_max = 0.0;
  for (size_t l = 0; l + 1 < c.launch_off.size(); ++l) {
    const std::vector<uint32_t> cut = cut_launch(c, s->sgd_work, s->sgd_work_max_launch, l, batches);
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
      const uint32_t ta = cut[b], tb = cut[b + 1];
      if (s->sgd_work[tb] == s->sgd_work[ta]) continue;   // nothing learns in this run
      const uint32_t p0 = c.tile_v[ta], p1 = c.tile_v[tb];
      const double lam = on_device && hostb::batch_is_dense(c, p0, p1)
          ? devb::batch_curvature(p0, p1, s->d_v_meta, s->d_v_row, s->d_row_ptr, s->d_edges, s->d_edge_fval64,
                                  s->opts.learn_non_evidence != 0, s->opts.noise_aware != 0, (uint32_t)c.W, dev_sc, (void *)s->stream)
          : hostb::batch_curvature(c, s->opts, p0, p1, host_sc);
      lam_max = std::max(lam_max, 1.1 * lam);
    }
  }
  if (getenv("DWX_TIMING")) fprintf(stderr, "[dwx curvature] batches=%u lambda=%.6g\n", batches, lam_max);
  s->row_sum_cache[batches] = lam_max;
  return lam_max;
}

void make_plan(dwx_sampler *s, double stepsize, uint32_t force_batches) {
  const CompiledGraph &c = *s->cg;
  uint32_t max_tiles = 1;
  for (size_t l = 0; l + 1 < c.launch_off.size(); ++l)
    max_tiles = std::max(max_tiles, c.launch_tile[l + 1] - c.launch_tile[l]);
  // No plan cuts finer than MAX_PLAN_BATCHES.  Stability does not depend on the cut: every
  // weight's step saturates at the inverse of its own curvature bound (apply_kernel), so a batch
  // can never overshoot.  The cut decides how closely the batches follow the reference's
  // sequential updates: inside a batch all draws see the weights of its start.
  max_tiles = std::min(max_tiles, MAX_PLAN_BATCHES);
  const double cap = s->opts.step_cap;
  uint32_t B = 1;
  const double eta = stepsize;
  if (force_batches) {
    // A forced count is the caller's GLOBAL plan (multi-GPU: every rank must run the same number
    // of batches, apply after each chunk and put the same vectors through the collectives): it is
    // NOT clamped by this shard's own tile count -- a shard with fewer tiles than batches simply
    // has fewer chunks and idles through the rest (a one-tile shard used to fall
    // back to plan_batches = 1, skip collectives its peers entered and apply whole-sweep counts).
    B = std::min(force_batches, MAX_PLAN_BATCHES);
  } else if (cap > 0 && stepsize > 0) {
    // Double the cut while the batches' curvature is above the cap AND cutting still lowers it:
    // a batch can be no finer than one variable, so a hub with 10^5 factors sets a floor no cut
    // gets under (its own kappa |d|^2) -- past it more batches only cost dependent launches
    // (the saturating step keeps the update stable there, section 3.5).
    while (B < max_tiles && stepsize * row_sum_bound(s, B) > cap) {
      // (looking two doublings ahead: one cut may fall on an unlucky boundary)
      if (row_sum_bound(s, 2 * B) > PLAN_MIN_GAIN * row_sum_bound(s, B) &&
          (4 * B > max_tiles || row_sum_bound(s, 4 * B) > PLAN_MIN_GAIN * PLAN_MIN_GAIN * row_sum_bound(s, B)))
        break;
      B *= 2;
    }
    B = std::min(B, max_tiles);
  }
  s->plan_batches = B;
  s->plan_eta = eta;
  // The step decays from sweep to sweep, so a run that starts at B batches walks down through
  // B/2, B/4, ...  Those levels are built when a plan first NEEDS them (round 4: at config 5's size a
  // level costs seconds of host time, and a `-l 10` run that starts at 4 batches never reaches 2 --
  // building them all up front was 15 s of its first learning epoch).  A caller that wants the
  // one-off work out of a timed region plans the coarser counts itself (bench.py: dist.py's
  // prepare), or sets DWX_EAGER_LEVELS.
  if (B > 1 && !s->levels.count(B) && getenv("DWX_EAGER_LEVELS")) {
    for (uint32_t b = B / 2; b >= 2; b /= 2) {
      if (cap > 0) (void)row_sum_bound(s, b);
      (void)build_level(s, b);
    }
  }
  // Nothing has been sampled yet: a plan whose mini-batches could wrap a weight's int64 sums is refused
  // here (DWX_E_LIMIT; learning_range_error), and so is one that would borrow the curvature bounds of
  // an un-split level that does not fit (plans without per-chunk tables apply with the whole sweep's).
  {
    dwx_sampler::Level *L = build_level(s, B);
    const std::string *why = !L->range_error.empty() ? &L->range_error : nullptr;
    if (!why && !L->fast) {
      auto it = s->levels.find(1);
      if (it != s->levels.end() && !it->second->range_error.empty()) why = &it->second->range_error;
    }
    if (why) {
      s->plan_valid = false;
      s->plan_level = nullptr;
      throw RangeError(*why);
    }
  }
  s->plan_level = build_level(s, B);
  s->plan_chunks = s->plan_level->chunks;
  s->cur_chunk = 0;
  s->plan_force_dynamic = false;
  s->plan_valid = true;
}

// The smallest step any weight takes under the current plan: stepsize saturated by the largest
// curvature bound (+ regularisation pull) of the plan's tables -- what `effective_stepsize`
// reports (== stepsize for weights with few factors; ~1/h for heavily tied ones).
double plan_min_step(dwx_sampler *s) {
  const dwx_sampler::Level *L = s->plan_level;
  if (!L || L->c_max <= 0.0 || s->plan_eta <= 0.0) return s->plan_eta;
  const double r = s->opts.regularization == 1 ? s->opts.reg_param * L->t_max : 0.0;
  const double c = DWX_CURV_MID * L->c_max + r, st = -std::expm1(-c * s->plan_eta) / c;
  return st * (L->c_max + r) > 1.0 ? 1.0 / (L->c_max + r) : st;   // batch_step (aux_kernels.h)
}

uint64_t layout_after_sweeps() {
  uint64_t n = 2048;
  if (const char *e = getenv("DWX_LAYOUT_AFTER_SWEEPS")) n = (uint64_t)std::max(1L, atol(e));   // test hook
  return n;
}

// accumulate the gradient of one chunk of the plan (sampling both chains on the way)
void enqueue_learn_chunk(dwx_sampler *s, uint32_t chunk) {
  rt::set_device(s->device);
  if (chunk >= s->plan_chunks.size()) return;   // ranks with fewer chunks idle through the rest
  const dwx_sampler::Chunk &ch = s->plan_chunks[chunk];
  KernelParams P = s->base;
  P.sweep = s->sweep;
  // a level that has run this many sweeps is worth a layout of its own (dwx_options.plan_layouts
  // == 0: the run pays 0.3 s once where it has already spent as much on the default layout)
  if (chunk == 0 && s->plan_level && ++s->plan_level->sweeps == layout_after_sweeps() && s->opts.plan_layouts == 0)
    ensure_level_layout(s, s->plan_level, s->plan_batches);
  const dwx_sampler::Level &L = *s->plan_level;
  const bool split = s->plan_batches > 1;
  // a split sweep without per-chunk tables falls back to per-record atomics and counts
  const bool fast = L.fast && !(split && s->plan_force_dynamic);
  if (split && !fast) P.flags |= OPT_DYNAMIC_T | OPT_NO_PULL;
  // an un-split sweep on weights the last inference sweep summed: its query super-tiles read the cache
  if (chunk == 0) {
    if (s->last_infer) s->pot_wanted = true;
    s->last_infer = false;
  }
  const uint32_t l = ch.launch;
  const CompiledGraph &c = *s->cg;
  const bool pot_hit = !split && s->pot_alloc > 0 && l < s->pot_valid.size() && s->pot_valid[l];
  // Deferred draws: an un-split sweep of an all-unary graph draws its evidence tiles only.
  // Nothing reads a query variable's two values while sweeps follow each other, so its draws are owed --
  // with this sweep's counter, d_w32 as it stands before the update (the snapshot) and, for now, the
  // potential cache -- until a reader asks (flush_pending) or a later sweep overwrites them unread.
  const bool defer = s->defer_ok && !split;
  dwx_sampler::Pending &pd = s->pending;
  if (chunk == 0 || !defer || pd.sweep != s->sweep) drop_pending(s);
  if (defer) {
    if (!pd.owed) {
      // (no copy of d_w32 here: the update that follows saves the old values as it overwrites them -- enqueue_apply;
      // the one copy at allocation defines the padding entry behind the W weights, which nothing rewrites)
      if (!s->d_w32_prev) {
        const size_t w32_bytes = ((size_t)c.W + 1) * sizeof(float);
        s->d_w32_prev = (float *)rt::dmalloc(w32_bytes);
        rt::d2d(s->d_w32_prev, s->d_w32, w32_bytes, s->stream);
      }
      pd.owed = pd.evid_owed = true;
      pd.snap = false;
      pd.sweep = s->sweep;
      pd.cached.assign(c.launch_tile.size(), 0);
      ++s->deferred_sweeps;
    }
    pd.cached[l] = pot_hit ? 1 : 0;
  }
  if (pot_hit) {
    // (a deferring launch has no query tile to read the cache: it is counted as the sweep that would have)
    if (!defer) {
      P.pot = s->d_pot;
      P.pot_v0 = c.tile_v[c.launch_tile[l]];
      P.pot_v1 = c.tile_v[c.launch_query_tile_end[l]];
    }
    if (chunk == 0) ++s->pot_sweeps;
  }
  TimedSpan sp = span_begin(s, 1);
  const uint32_t launches = defer ? launch_tiles<true>(s, P, l, std::max(ch.t0, c.launch_query_tile_end[l]), ch.t1, false, nullptr, true)
                                  : launch_tiles<true>(s, P, l, ch.t0, ch.t1);
  if (s->timing) rt::event_record(sp.b, s->stream);
  bool pulled = false;
  // the pull-based gradient of the TILE_PULL tiles: un-split sweeps once, after the last
  // chunk (= colour launch), over the whole list; split sweeps per chunk over its part
  uint32_t pb = 0, pe = 0;
  if (fast && !L.inc_end.empty()) {
    if (!split) { if (chunk + 1 == s->plan_chunks.size()) { pb = L.inc_begin.front(); pe = L.inc_end.back(); } }
    else { pb = L.inc_begin[chunk]; pe = L.inc_end[chunk]; }
  }
  // block pull of the same group as the list: the whole sweep (un-split, after the last colour
  // launch) or this chunk; what did not fit the block tables' rows stays on the weight-sorted list
  // (config 3: 3.7 % of the entries) and is summed by fold_partials_kernel's lane of the weight.
  // A group without a table pulls its whole list with pull_grad_kernel.
  const dwx_sampler::Level::BlockTable *bt = nullptr;
  if (fast && !L.bp.empty() && (split || chunk + 1 == s->plan_chunks.size())) {
    bt = &L.bp[split ? chunk : 0];
    if (!bt->blocks) bt = nullptr;
  }
  auto launch_list = [&](rt::stream_t st) {
    const uint32_t n = pe - pb;
    const unsigned chunk_sz = BLOCK_THREADS * PULL_RUN;
    const unsigned grid = std::min<unsigned>((n + chunk_sz - 1) / chunk_sz, 256u * DWX_PULL_GRID);
    auto go = [&](auto kernel) {
      rt::launch(kernel, grid, BLOCK_THREADS, 0, st, (const uint32_t *)(L.d_inc_wid + pb),
                 (const uint32_t *)(L.d_inc_slot + pb), (const float *)(L.d_inc_d + pb), n,
                 (const unsigned long long *)s->d_delta, s->d_grad);
    };
    // (a weight's entries span lanes only when it has many: what the block tables left over of a
    // million weights does not)
    if ((uint64_t)n >= 8 * s->cg->W) go(pull_grad_kernel<true>); else go(pull_grad_kernel<false>);
    pulled = true;
  };
  if (bt) {
    const unsigned grid = bt->blocks * bt->parts;
    auto go = [&](auto kernel) {
      rt::launch(kernel, grid, BP_THREADS, BP_LDS_BYTES, s->stream, (const U32x4 *)bt->d_ell,
                 (const uint32_t *)bt->d_tile0, bt->parts, (const long long *)L.d_bp_qtab, L.bp_deltas, L.bp_wp,
                 (const unsigned long long *)s->d_delta, L.d_bp_partial);
    };
    auto go1 = [&](auto kernel) {
      rt::launch(kernel, grid, BP_THREADS, BP1_LDS_BYTES, s->stream, (const unsigned long long *)bt->d_ell,
                 (const uint32_t *)bt->d_tile0, bt->parts, bt->tiles, L.bp_wp, (const unsigned long long *)s->d_delta,
                 (signed char *)L.d_bp_partial);
    };
    const bool uni = L.bp_deltas == 1;   // one delta: packed rows of 1 to 4 planes; else 32-bit entries, 1 or 2 rows
    if (bt->one_plane) {                 // ... with the signs in the rows and one ballot plane in LDS
      switch (bt->depth) {
        case 1: go1(pull_ell1_kernel<1>); break;
        case 2: go1(pull_ell1_kernel<2>); break;
        case 3: go1(pull_ell1_kernel<3>); break;
        default: go1(pull_ell1_kernel<4>); break;
      }
    } else if (uni) {
      switch (bt->depth) {
        case 1: go(pull_ell_kernel<1, true, true>); break;
        case 2: go(pull_ell_kernel<2, true, true>); break;
        case 3: go(pull_ell_kernel<3, true, true>); break;
        default: go(pull_ell_kernel<4, true, true>); break;
      }
    } else if (bt->depth == 2) {
      go(pull_ell_kernel<2, false>);
    } else {
      go(pull_ell_kernel<1, false>);
    }
    const uint32_t W = (uint32_t)s->cg->W;
    const unsigned fgrid = std::min<unsigned>((W + BLOCK_THREADS * FOLD_W - 1) / (BLOCK_THREADS * FOLD_W), 4096u);
    const uint32_t *ov = pe > pb ? (const uint32_t *)bt->d_ov_start : nullptr;   // (nothing left over: no list to walk)
    if (uni)
      rt::launch(fold_partials_kernel<true>, fgrid, BLOCK_THREADS, 0, s->stream, (const long long *)L.d_bp_partial,
                 bt->blocks, L.bp_wp, W, s->d_grad, (const long long *)L.d_bp_qtab, ov, (const uint32_t *)(L.d_inc_slot + pb),
                 (const float *)(L.d_inc_d + pb), (const unsigned long long *)s->d_delta);
    else
      rt::launch(fold_partials_kernel<false>, fgrid, BLOCK_THREADS, 0, s->stream, (const long long *)L.d_bp_partial,
                 bt->blocks, L.bp_wp, W, s->d_grad, (const long long *)L.d_bp_qtab, ov, (const uint32_t *)(L.d_inc_slot + pb),
                 (const float *)(L.d_inc_d + pb), (const unsigned long long *)s->d_delta);
    pulled = true;
  } else if (pe > pb) {
    launch_list(s->stream);
  }
  span_end(s, sp, launches, pulled, chunk == 0, 1, true);
}

void enqueue_apply(dwx_sampler *s) {
  rt::set_device(s->device);
  weights_change(s);
  const uint32_t W = (uint32_t)s->cg->W;
  if (!W) return;
  const unsigned grid = std::min<unsigned>((W + BLOCK_THREADS - 1) / BLOCK_THREADS, 2048u);
  // static tables of what was just accumulated: row pair 0 of an un-split sweep, the chunk's of
  // a split one.  On the atomics fallback (a split plan without tables, or one a multi-GPU
  // driver forced to count dynamically) the counts are in the grad buffer and the curvature
  // bounds are those of the WHOLE sweep (level 1: >= any chunk's, so the step only saturates
  // earlier)
  const dwx_sampler::Level *L = s->plan_level;
  const bool split = s->plan_batches > 1;
  const long long *ts = nullptr, *hs = nullptr;
  if (L && L->fast && L->d_t_static && !(split && s->plan_force_dynamic)) {
    const uint32_t row = split ? s->cur_chunk : 0u;
    if (row < L->rows) { ts = L->d_t_static + (size_t)row * 2 * W; hs = ts + W; }
  } else {
    auto it = s->levels.find(1);
    if (it != s->levels.end() && it->second->d_t_static) hs = it->second->d_t_static + W;
  }
  // draws owed under the weights this update overwrites: the kernel saves them on its way
  dwx_sampler::Pending &pd = s->pending;
  float *prev = pd.owed && !pd.snap ? s->d_w32_prev : nullptr;
  if (prev) pd.snap = true;
  rt::launch(apply_kernel, grid, BLOCK_THREADS, 0, s->stream, s->d_weights, s->d_w32,
             (const uint8_t *)s->d_w_fixed, s->d_grad, ts, hs, W, s->plan_eta, s->opts.reg_param,
             (int)(s->opts.regularization == 1), (const double *)nullptr, (long long *)nullptr, prev);
}

// A split learning sweep of an all-unary graph with few weights (LDS gradient accumulators), one launch
// per mini-batch: the update of mini-batch c - 1 is the prologue of mini-batch c's sweep kernel
// (sweep8_merged_kernel, persist_kernels.h); three gradient buffers and two weight buffers in turn, the
// last update by apply_kernel into the sampler's own arrays.  false: the sweep does not qualify.
bool enqueue_merged_sweep(dwx_sampler *s) {
  dwx_sampler::Level *L = s->plan_level;
  const uint32_t n = (uint32_t)s->plan_chunks.size();
  const CompiledGraph &c = *s->cg;
  const uint32_t W = (uint32_t)c.W;
  if (!s->merge_ok || !L || s->plan_batches < 2 || n < 2 || !L->fast || !L->d_t_static || L->rows < n || s->plan_force_dynamic)
    return false;
  rt::set_device(s->device);
  if (!s->d_gbuf[1]) {
    for (int k = 1; k < 3; ++k) {
      s->d_gbuf[k] = (long long *)rt::dmalloc((size_t)W * 16);
      rt::dmemset(s->d_gbuf[k], 0, (size_t)W * 16, s->stream);
    }
    for (int k = 0; k < 2; ++k) { s->d_wbuf64[k] = (double *)rt::dmalloc((size_t)W * 8); s->d_wbuf32[k] = (float *)rt::dmalloc((size_t)W * 4 + 4); }
  }
  s->d_gbuf[0] = s->d_grad;
  drop_pending(s);   // (a split sweep draws every variable's two chains)
  if (s->plan_level) ++s->plan_level->sweeps;
  const unsigned cap = s->kv.learn.cap;
  // The leading tiles of the first mini-batch in which NOTHING learns -- the query part of the colour launch:
  // half of config 4's tiles, 190 us of bandwidth work at the head of 63 latency-bound launches of 16 us -- run
  // beside the mini-batches instead of ahead of them: on a side stream, one workgroup per CU (the mini-batches'
  // workgroups keep the other two slots of every CU).  They read the sweep's starting weights -- the sampler's
  // own arrays, which no merged launch writes; the closing update waits for them -- add nothing to any gradient
  // (flush_accumulators skips zeros) and, on an all-unary graph, nobody reads their samples: the same results.
  uint32_t quiet_end = s->plan_chunks[0].t0;
  if (s->side[0] && s->ev_fork && s->ev_join[0] && !getenv("DWX_NO_QUIET_ASIDE")) {
    const dwx_sampler::Chunk &c0 = s->plan_chunks[0];
    while (quiet_end < c0.t1 && quiet_end + 1 < s->sgd_work.size() && s->sgd_work[quiet_end + 1] == s->sgd_work[quiet_end]) ++quiet_end;
    if (quiet_end - c0.t0 < 4 * rt::grid_barrier_blocks()) quiet_end = c0.t0;   // (too few to be worth a launch)
  }
  const bool aside = quiet_end > s->plan_chunks[0].t0;
  if (aside) {
    KernelParams Q = s->base;
    Q.sweep = s->sweep;
    Q.tile_begin = s->plan_chunks[0].t0; Q.tile_end = quiet_end;
    rt::event_record(s->ev_fork, s->stream);
    rt::stream_wait_event(s->side[0], s->ev_fork);
    unsigned side_wgs = std::max(1u, rt::grid_barrier_blocks());
    if (const char *e = getenv("DWX_QUIET_GRID")) side_wgs = (unsigned)std::max(1L, atol(e));   // (tuning knob)
    const unsigned grid = std::min<unsigned>(quiet_end - Q.tile_begin, side_wgs);
    s->kv.learn.launch(grid, BLOCK_THREADS, s->side[0], Q);
    rt::event_record(s->ev_join[0], s->side[0]);
  }
  for (uint32_t ci = 0; ci < n; ++ci) {
    dwx_sampler::Chunk ch = s->plan_chunks[ci];
    if (ci == 0) ch.t0 = quiet_end;
    s->cur_chunk = ci;
    KernelParams P = s->base;
    P.sweep = s->sweep;
    P.grad = s->d_gbuf[ci % 3];
    P.tile_begin = ch.t0; P.tile_end = ch.t1;
    MergeArgs M{};
    M.prev_grad = ci ? s->d_gbuf[(ci - 1) % 3] : nullptr;
    M.zero = s->d_gbuf[(ci + 1) % 3];
    M.w_src = ci <= 1 ? s->d_weights : s->d_wbuf64[(ci - 2) % 2];
    M.w_dst = ci ? s->d_wbuf64[(ci - 1) % 2] : nullptr;
    M.w32_dst = ci ? s->d_wbuf32[(ci - 1) % 2] : nullptr;
    M.w_fixed = s->d_w_fixed;
    M.t_static = ci ? L->d_t_static + (size_t)(ci - 1) * 2 * W : nullptr;
    M.stepsize = s->plan_eta; M.reg_param = s->opts.reg_param;
    M.l2 = s->opts.regularization == 1 ? 1 : 0;
    M.lds_lw32_off = s->merge_lw32_off;
    TimedSpan sp = span_begin(s, 1);
    if (ch.t1 > ch.t0 && ch.t1 - ch.t0 <= cap && !getenv("DWX_NO_ONE_TILE")) {
      // a workgroup per tile (the usual shape of a mini-batch): the build without the next-tile machinery
      s->kv.merged[1].launch(ch.t1 - ch.t0, BLOCK_THREADS, s->stream, P, M);
    } else if (ch.t1 > ch.t0) {
      s->kv.merged[0].launch(std::min<unsigned>(ch.t1 - ch.t0, cap), BLOCK_THREADS, s->stream, P, M);
    } else {
      // (an empty chunk: the update alone, through a one-workgroup launch over no tile)
      P.tile_begin = P.tile_end = 0;
      s->kv.merged[0].launch(1u, BLOCK_THREADS, s->stream, P, M);
    }
    span_end(s, sp, 1, false, ci == 0);
  }
  // the last mini-batch's update: from the weights the last merged launch wrote, into the sampler's own arrays
  if (aside) rt::stream_wait_event(s->stream, s->ev_join[0]);   // (the quiet tiles still read those arrays)
  {
    const uint32_t last = n - 1;
    const unsigned grid = std::min<unsigned>((W + BLOCK_THREADS - 1) / BLOCK_THREADS, 2048u);
    const long long *ts = L->d_t_static + (size_t)last * 2 * W;
    const double *w_in = last == 0 ? (const double *)nullptr : (const double *)s->d_wbuf64[(last - 1) % 2];
    rt::launch(apply_kernel, grid, BLOCK_THREADS, 0, s->stream, s->d_weights, s->d_w32, (const uint8_t *)s->d_w_fixed,
               s->d_gbuf[last % 3], ts, ts + W, W, s->plan_eta, s->opts.reg_param, (int)(s->opts.regularization == 1), w_in,
               last ? s->d_gbuf[(last - 1) % 3] : (long long *)nullptr, (float *)nullptr);
  }
  weights_change(s);
  ++s->merged_sweeps;
  return true;
}

// A split learning sweep of a few-weights, all-unary graph as ONE persistent launch
// (persist_kernels.h): every chunk's draws, gradient rows, the barrier and the update inside it.
// false: this sweep does not qualify (the caller enqueues it chunk by chunk).
bool enqueue_persistent_sweep(dwx_sampler *s) {
  dwx_sampler::Level *L = s->plan_level;
  const uint32_t n = (uint32_t)s->plan_chunks.size();
  if (!s->persist_grid || !L || s->plan_batches < 2 || n < PERSIST_MIN_CHUNKS || !L->fast || !L->d_t_static ||
      L->rows < n || s->plan_force_dynamic)
    return false;
  rt::set_device(s->device);
  uint32_t most = 0;
  for (const auto &ch : s->plan_chunks) most = std::max(most, ch.t1 - ch.t0);
  if (!most) return false;
  if (!L->d_chunk_tiles) {
    std::vector<uint32_t> ct;
    for (const auto &ch : L->chunks) { ct.push_back(ch.t0); ct.push_back(ch.t1); }
    L->d_chunk_tiles = upload(ct, s->stream);
    rt::stream_sync(s->stream);      // (the host copy dies with this scope)
  }
  ++L->sweeps;
  drop_pending(s);   // (a split sweep draws every variable's two chains)
  KernelParams P = s->base;
  P.sweep = s->sweep;
  PersistArgs A{};
  A.chunk_tiles = L->d_chunk_tiles;
  A.n_chunks = n;
  A.grid = std::min(most, s->persist_grid);
  A.rows = s->d_persist_rows;
  A.row_stride = s->persist_row_stride;
  A.bar = s->d_persist_bar;
  A.t_static = L->d_t_static;
  A.weights = s->d_weights; A.w32 = s->d_w32; A.w_fixed = s->d_w_fixed;
  A.stepsize = s->plan_eta; A.reg_param = s->opts.reg_param;
  A.l2 = s->opts.regularization == 1 ? 1 : 0;
  A.spin_limit = 4u << 20;
  A.lds_w64_off = s->persist_w64_off; A.lds_red_off = s->persist_red_off;
  TimedSpan sp = span_begin(s, 1);
  rt::dmemset(s->d_persist_bar, 0, 16, s->stream);
  s->kv.persist.launch(A.grid, BLOCK_THREADS, s->stream, P, A);
  span_end(s, sp, 1, false, true);
  weights_change(s);
  s->cur_chunk = n - 1;
  s->persist_check_pending = true;
  ++s->persist_launches;
  return true;
}

void drain_spans(dwx_sampler *s) {
  if (s->spans.empty()) return;
  rt::stream_sync(s->stream);
  for (auto &sp : s->spans) {
    s->t_ms[sp.kind] += rt::event_elapsed_ms(sp.a, sp.b);
    s->t_launches[sp.kind] += sp.launches;
    s->t_sweeps[sp.kind] += sp.new_sweep ? sp.n_sweeps : 0;   // (a learning sweep is one or more chunks)
    if (sp.has_pull) {
      s->t_ms[2] += rt::event_elapsed_ms(sp.b, sp.c);
      s->t_launches[2] += 1;
    }
    if (sp.kind == 1 && sp.new_sweep) s->t_sweeps[2] += 1;
    rt::event_destroy(sp.a); rt::event_destroy(sp.b); rt::event_destroy(sp.c);
  }
  s->spans.clear();
}
}  // namespace

extern "C" {

const char *dwx_last_error(void) { return g_err.c_str(); }
int dwx_version(void) { return DWX_VERSION; }

void dwx_default_options(dwx_options *o) {
  std::memset(o, 0, sizeof *o);
  o->regularization = 1;  // l2 (src/cmd_parser.cc:163-166)
  o->reg_param = 0.01;    // src/cmd_parser.cc:162
  o->step_cap = 1.5;   // stepsize * lambda of one SGD mini-batch (the hard limit is 2)
  o->seed = 0x5eed5eedULL;
}

// ------------------------------------------------------------------ graph
int dwx_graph_create(const dwx_graph_desc *desc, const dwx_compile_opts *opts, dwx_graph **out) {
  if (!desc || !out) return fail(DWX_E_INVALID, "null argument");
  dwx_compile_opts o{};
  if (opts) o = *opts;
  o.defer_sorted_records = build_on_device();   // (the weight-sorted copy of the records: built by every sampler)
  bool limit = false;
  try {
    auto cg = std::make_shared<CompiledGraph>();
    compile_graph(*desc, o, *cg, &limit);
    *out = new dwx_graph{cg};
    return DWX_OK;
  } catch (const std::bad_alloc &) {
    return fail(DWX_E_NOMEM, "out of host memory while compiling the graph");
  } catch (const std::exception &e) {
    return fail(limit ? DWX_E_LIMIT : DWX_E_INVALID, e.what());
  }
}

void dwx_graph_destroy(dwx_graph *g) { delete g; }

int dwx_graph_get_info(const dwx_graph *g, dwx_graph_info *out) {
  if (!g || !out) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *g->cg;
  std::memset(out, 0, sizeof *out);
  out->num_owned_variables = c.Vo;
  out->num_variables = c.V; out->num_factors = c.F; out->num_edges = c.E; out->num_weights = c.W;
  out->num_values = c.R; out->num_index_entries = c.NIdx; out->num_vif_entries = c.NVif;
  out->num_colors = c.n_colors; out->num_launches = c.launch_off.size() - 1;
  out->num_tiles = c.tile_v.size() - 1; out->num_giant_tiles = c.n_giant_tiles;
  out->num_wide_tiles = c.n_wide_tiles;
  out->num_staged_tiles = c.ecap <= 6 * BLOCK_THREADS ? c.n_terms2_tiles : 0;
  out->max_cardinality = c.max_card; out->device_bytes = c.device_bytes();
  out->num_query_variables = c.n_query;
  out->has_categorical = c.has_categorical; out->order_is_identity = c.order_is_identity;
  out->num_super_tiles = c.supers.size(); out->num_sorted_records = c.n_sorted;
  out->max_super_tile_variables = 0;
  for (const SuperTile &st : c.supers) out->max_super_tile_variables = std::max<uint64_t>(out->max_super_tile_variables, st.nv);
  out->grad_shift = c.grad_shift; out->grad_unit_max = c.grad_unit_max; out->max_records_per_weight = c.max_records_per_weight;
  out->factor_table_bytes = c.factor_table_bytes();
  return DWX_OK;
}

int dwx_graph_get_schedule(const dwx_graph *g, uint64_t *order, uint64_t *launch_off) {
  if (!g || !order || !launch_off) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *g->cg;
  for (uint64_t p = 0; p < c.Vo; ++p) order[p] = c.perm[p];
  std::copy(c.launch_off.begin(), c.launch_off.end(), launch_off);
  return DWX_OK;
}

int dwx_graph_get_fixed_point_mask(const dwx_graph *g, uint8_t *mask) {
  if (!g || !mask) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *g->cg;
  std::fill(mask, mask + c.V, (uint8_t)0);
  if (c.edges8.size() == 0) return DWX_OK;      // compact records only (sweep8_kernel, sorted_sweep_kernel)
  for (const TileDesc &t : c.tiles) {
    if (t.flags & (TILE_OUTSIDE | TILE_CATEGORICAL)) continue;   // wave / workgroup bins, value rows: f64 sums
    for (uint32_t l = 0; l < t.nv; ++l) mask[c.perm[t.v0 + l]] = 1;
  }
  return DWX_OK;
}

int dwx_graph_get_values(const dwx_graph *g, uint64_t *var_val_base, uint64_t *value_sparse) {
  if (!g) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *g->cg;
  // (by all host threads: 1.6 GB at config 5's size, and the first touch of the caller's arrays)
  auto copy = [](const std::vector<uint64_t> &src, uint64_t *dst) {
    parallel_ranges(src.size(), host_threads(), [&](uint64_t b, uint64_t e) { std::memcpy(dst + b, src.data() + b, (e - b) * 8); });
  };
  if (var_val_base) copy(c.ref_var_val_base, var_val_base);
  if (value_sparse) copy(c.value_sparse, value_sparse);
  return DWX_OK;
}

int dwx_graph_get_positions(const dwx_graph *g, const uint64_t *vids, uint64_t n, uint64_t *out) {
  if (!g || (n && (!vids || !out))) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *g->cg;
  for (uint64_t i = 0; i < n; ++i) {
    if (vids[i] >= c.V) return fail(DWX_E_INVALID, "variable id out of range");
    out[i] = c.pos[vids[i]];
  }
  return DWX_OK;
}

int dwx_graph_get_index(const dwx_graph *g, uint64_t *index_base, uint64_t *index_len,
                        uint64_t *factor_index) {
  if (!g) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *g->cg;
  for (uint64_t r = 0; r < c.R; ++r) {
    if (index_base) index_base[r] = c.ref_row_ptr[r];
    if (index_len) index_len[r] = c.ref_row_ptr[r + 1] - c.ref_row_ptr[r];
  }
  if (factor_index) for (uint64_t i = 0; i < c.NIdx; ++i) factor_index[i] = c.ref_fidx[i];
  return DWX_OK;
}

int dwx_graph_get_tiles(const dwx_graph *g, uint64_t n, dwx_tile_info *out) {
  if (!g || (n && !out)) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *g->cg;
  if (n != c.tiles.size()) return fail(DWX_E_INVALID, "dwx_graph_get_tiles: n is not dwx_graph_info.num_tiles");
  for (uint64_t i = 0; i < n; ++i) {
    const TileDesc &t = c.tiles[i];
    out[i] = dwx_tile_info{t.flags, t.v0, t.nv, t.nrows, t.nedges};
  }
  return DWX_OK;
}

// ------------------------------------------------------------------ sampler
int dwx_sampler_create(const dwx_graph *g, const dwx_options *opts, dwx_sampler **out) {
  if (!g || !opts || !out) return fail(DWX_E_INVALID, "null argument");
  std::unique_ptr<dwx_sampler> s(new dwx_sampler());
  int rc = guarded([&]() {
    rt::init_device(opts->device);
    rt::oom_hook() = [](int dev) { devb::release_scratch(dev, false); };
    s->cg = g->cg;
    s->opts = *opts;
    s->device = opts->device;
    const CompiledGraph &c = *s->cg;
    s->stream = rt::stream_create();
    rt::stream_t st = s->stream;
    if (!getenv("DWX_NO_SIDE_STREAMS")) {   // (A/B knob)
      for (int i = 0; i < 2; ++i) { s->side[i] = rt::stream_create(); s->ev_join[i] = rt::event_create_ordering(); }
      s->ev_fork = rt::event_create_ordering();
    }
    const bool timing = getenv("DWX_TIMING") != nullptr;   // wall time of every phase on stderr
    auto t_phase = std::chrono::steady_clock::now();
    auto phase = [&](const char *what) {
      if (!timing) return;
      rt::stream_sync(st);
      auto t = std::chrono::steady_clock::now();
      fprintf(stderr, "[dwx sampler_create] %-24s %.3f s\n", what, std::chrono::duration<double>(t - t_phase).count());
      t_phase = t;
    };
    s->d_v_meta = upload(c.v_meta, st, 1);
    s->d_v_orig = upload(c.perm, st, 1);
    s->d_v_row = upload(c.v_row, st);
    s->d_v_init = upload(c.v_init, st, 1);
    s->d_row_ptr = upload(c.row_ptr, st, 1);
    {
      // edge-parallel evaluation of binary factors is compiled for K <= 6 only (register
      // budget): with 3072-record tiles such tiles take the generic path
      std::vector<TileDesc> tiles = c.tiles;
      if (c.ecap > 6 * BLOCK_THREADS) for (auto &t : tiles) t.flags &= ~(TILE_TERMS2 | TILE_TERMS3 | TILE_PULL_UNARY);
      s->d_tiles = upload(tiles, st);
    }
    for (uint32_t ti : c.giant_tiles) ((c.tiles[ti].flags & TILE_CATEGORICAL) ? s->cgiant_tiles : s->bgiant_tiles).push_back(ti);
    s->d_giant = upload(s->cgiant_tiles, st);
    s->d_wide = upload(c.wide_tiles, st);
    {
      std::vector<GiantPiece> pieces;
      s->bgiant_piece_off.assign(1, 0u);
      for (uint32_t slot = 0; slot < s->bgiant_tiles.size(); ++slot) {
        const TileDesc &td = c.tiles[s->bgiant_tiles[slot]];
        for (uint32_t e = td.e0; e < td.e0 + td.nedges; e += GIANT_PIECE)
          pieces.push_back(GiantPiece{slot, e, std::min(e + GIANT_PIECE, td.e0 + td.nedges), 0u});
        if (!td.nedges) pieces.push_back(GiantPiece{slot, td.e0, td.e0, 0u});
        s->bgiant_piece_off.push_back((uint32_t)pieces.size());
      }
      s->d_bgiant = upload(s->bgiant_tiles, st);
      s->d_bgiant_piece_off = upload(s->bgiant_piece_off, st);
      s->d_bgiant_pieces = upload(pieces, st);
      s->d_bgiant_partial = (double *)rt::dmalloc(std::max<size_t>(1, pieces.size()) * 4 * 8);
      rt::dmemset(s->d_bgiant_partial, 0, std::max<size_t>(1, pieces.size()) * 4 * 8, st);
      s->d_bgiant_decision = (uint32_t *)rt::dmalloc(std::max<size_t>(1, s->bgiant_tiles.size()) * 16);
    }
    if (!c.row_truth.empty()) s->d_row_truth = upload(c.row_truth, st);
    if (!c.edge_fval64.empty()) s->d_edge_fval64 = upload(c.edge_fval64, st);
    s->d_edges = upload(c.edges, st, 1);
    s->rec8 = c.edges8.size() != 0;
    if (s->rec8) s->d_edges8 = upload(c.edges8, st, 1);
    // deferred draws: all-unary graphs on which a query variable triggers no SGD (DWX_NO_DEFER: A/B knob)
    s->defer_ok = s->rec8 && !opts->learn_non_evidence && !opts->noise_aware && !getenv("DWX_NO_DEFER");
    if (!c.supers.empty()) {
      s->d_supers = upload(c.supers, st);
      if (c.sorted_deferred) {
        // planned on the host, built here: emit + radix sort by (super-tile, weight id) on the device
        s->d_sorted = (SortRec8 *)rt::dmalloc((c.n_sorted + 1) * sizeof(SortRec8));
        rt::dmemset(s->d_sorted + c.n_sorted, 0, sizeof(SortRec8), st);
        devb::build_sorted_records(s->d_tiles, s->d_edges, s->d_edges8, s->d_supers, (uint32_t)c.supers.size(),
                                   c.sort_dbits.data(), (uint32_t)c.sort_dbits.size(), c.n_sorted, s->d_sorted, (void *)st);
      } else {
        s->d_sorted = upload(c.sorted_recs, st, 1);
      }
      s->d_sort_dvals = upload(c.sort_dvals, st);
      s->n_sort_dvals = (uint32_t)c.sort_dvals.size();
      s->sorted_learn = c.W > LDS_AGG_MAX_W;     // == their tiles are TILE_PULL
      // [UNI: one distinct d]; the RB builds are allowed by their first launch
      const size_t lds_sorted = sort_lds_bytes(s->n_sort_dvals);
      auto set = [&](SortedVariant &k, auto fn, bool rb) { k.fn = fn; k.lds = lds_sorted; if (!rb) k.allow(); };
      set(s->kv.sorted_infer[0][0], sorted_sweep_kernel<false, false>, false);
      set(s->kv.sorted_infer[0][1], sorted_sweep_kernel<false, false, true>, true);
      set(s->kv.sorted_infer[1][0], sorted_sweep_kernel<false, true>, false);
      set(s->kv.sorted_infer[1][1], sorted_sweep_kernel<false, true, true>, true);
      set(s->kv.sorted_learn[0], sorted_sweep_kernel<true, false>, false);
      set(s->kv.sorted_learn[1], sorted_sweep_kernel<true, true>, false);
      s->no_sort_uni = getenv("DWX_NO_SORT_UNI") != nullptr;
      s->pot_query_first = getenv("DWX_POT_QUERY_FIRST") != nullptr;
    }
    {
      // the batched walks load a factor's first entries branch-free (a unary record reads entry
      // 0 and ignores it): the array is never empty, entry 0 names a real variable
      std::vector<VifRec> vifs = c.vifs;
      if (vifs.size() < 4) vifs.resize(4, VifRec{0u, 0u});
      s->d_vifs = upload(vifs, st, 4);
    }
    // InferenceResult init (src/inference_result.cc:24-42): both chains start at the
    // evidence value or 0, tallies zero, weights at their initial values
    std::vector<uint32_t> a0(c.V);
    for (uint64_t p = 0; p < c.V; ++p) a0[p] = (c.v_meta[p] & VM_EVIDENCE) ? c.v_init[p] : 0u;
    s->d_assign_free = upload(a0, st);
    s->d_assign_evid = upload(a0, st);
    s->d_tally = (uint32_t *)rt::dmalloc((c.R + 1) * 4);
    rt::dmemset(s->d_tally, 0, (c.R + 1) * 4, st);
    s->d_weights = upload(c.w_init, st);
    phase("upload graph");
    {
      std::vector<float> w32(c.W);
      for (uint64_t i = 0; i < c.W; ++i) w32[i] = (float)c.w_init[i];
      s->d_w32 = upload(w32, st, 1);
      // (+ one variable block of padding: pull_ell_kernel copies whole blocks)
      const size_t n_delta = c.tiles.size() * 8 + 2 + (size_t)BP1_TILES * 8;
      s->d_delta = (unsigned long long *)rt::dmalloc(n_delta * 8);
      rt::dmemset(s->d_delta, 0, n_delta * 8, st);
    }
    s->d_w_fixed = upload(c.w_fixed, st);
    s->d_grad = (long long *)rt::dmalloc(c.W * 16);
    rt::dmemset(s->d_grad, 0, c.W * 16, st);

    KernelParams &P = s->base;
    P.v_meta = s->d_v_meta; P.v_orig = s->d_v_orig; P.v_row = s->d_v_row; P.v_init = s->d_v_init;
    P.row_ptr = s->d_row_ptr; P.row_truth = s->d_row_truth; P.edges = s->d_edges; P.edges8 = s->d_edges8; P.edge_terms = nullptr;
    for (const TileDesc &td : c.tiles) if (td.flags & (TILE_SIMPLE | TILE_INLINE2)) { s->has_simple_tiles = true; break; }
    P.edge_fval64 = s->d_edge_fval64; P.vifs = s->d_vifs; P.tiles = s->d_tiles;
    P.assign_free = s->d_assign_free; P.assign_evid = s->d_assign_evid; P.tally = s->d_tally;
    P.w32 = s->d_w32; P.grad = s->d_grad; P.delta = s->d_delta;
    P.seed = opts->seed; P.sweep = 0; P.vid_offset = opts->var_id_offset; P.tile_begin = 0; P.num_weights = (uint32_t)c.W;
    P.flags = (opts->sample_evidence ? OPT_SAMPLE_EVIDENCE : 0) |
              (opts->learn_non_evidence ? OPT_LEARN_NON_EVIDENCE : 0) |
              (opts->noise_aware ? OPT_NOISE_AWARE : 0) |
              (c.has_f64_fval ? OPT_HAS_F64_FVAL : 0) | (c.has_truthiness ? OPT_HAS_TRUTHINESS : 0);
    P.ecap = c.ecap; P.rcap = c.rcap;
    // dynamic LDS layout: [row pointers | potentials scratch (categorical) | K*256 edge
    // records | K*256 f32 weights (learning kernel only)]; K = records staged per lane
    if (c.ecap > MAX_ECAP) throw std::invalid_argument("tile_edges exceeds the staging capacity");
    s->stage_k = c.ecap <= 3 * BLOCK_THREADS ? 3 : (c.ecap <= 6 * BLOCK_THREADS ? 6 : 12);
    const size_t slots = (size_t)s->stage_k * BLOCK_THREADS;
    s->rp_cat = c.edges8.size() != 0 && c.has_categorical && s->stage_k == 6;
    const size_t nrp = std::max<size_t>(c.rcap + 1, (s->rp_cat ? ROWPTR_UNROLL_CAT : ROWPTR_UNROLL) * BLOCK_THREADS);
    size_t off = (nrp * 4 + 15) & ~(size_t)15;
    P.lds_pot_off = c.has_categorical ? (uint32_t)off : 0u;
    if (c.has_categorical) off += (size_t)c.rcap * 8;
    off = (off + 15) & ~(size_t)15;
    P.lds_edge_off = (uint32_t)off;
    s->wide_learn = c.n_terms2_tiles > 0 && s->stage_k <= 6;
    off += slots * sizeof(EdgeRec);
    P.lds_w_off = (uint32_t)off;     // f32 weights right behind the 16-byte records
    const size_t lds_infer = off;
    {
      // the tile classes this graph holds: sweep_kernel's smallest build that contains them
      uint32_t tv = 0;
      for (const TileDesc &td : c.tiles) {
        if (td.flags & TILE_OUTSIDE) continue;
        if (td.flags & TILE_CATEGORICAL) tv |= TV_CATEGORICAL;
        if (td.flags & TILE_TERMS3) tv |= TV_TERMS3;
        else if (td.flags & TILE_TERMS2) tv |= (td.flags & TILE_INLINE2) ? TV_TERMS2_INLINE : TV_TERMS2_VIFS;
        else if (td.flags & TILE_SIMPLE) tv |= TV_SIMPLE;
        else tv |= TV_GENERIC;
      }
      // (TV_PAIR stages 16-byte learning records: the weight id shares its word with two flags)
      s->tv_pair = s->wide_learn && s->stage_k == 6 && (tv & TV_TERMS2_INLINE) && !(tv & ~TV_PAIR) &&
                   c.W <= LR16_WID_MASK && !getenv("DWX_NO_TILE_VARIANTS");
    }
    // learning: 16-byte records + f32 weights (20 B per slot); with TILE_TERMS2 tiles the same region
    // alternatively holds 32-byte LearnRecs (which carry their weight) -- 16-byte ones in the TV_PAIR build
    size_t lds_learn = P.lds_edge_off + slots * (s->wide_learn && !s->tv_pair ? 32 : 20);
    P.lds_agg_off = 0;
    P.n_sweeps = 1;
    if (c.W > 0 && c.W <= LDS_AGG_MAX_W) {
      P.lds_agg_off = (uint32_t)((lds_learn + 15) & ~(size_t)15);
      lds_learn = P.lds_agg_off + (size_t)c.W * 16;
    }
    if (lds_learn > 160 * 1024) throw std::invalid_argument("tile does not fit the 160 KiB LDS");
    if (s->rec8) {
      s->all_pull = P.lds_agg_off == 0;   // (TILE_PULL implies it; a graph of oversized variables only has no such tile)
      for (const TileDesc &td : c.tiles)
        if (!(td.flags & TILE_OUTSIDE) && !(td.flags & TILE_PULL)) { s->all_pull = false; break; }
    }
    // (inference on the 8-byte terms table, learning with the pull gradient alone: 8 bytes staged per record)
    resolve_builds(s.get(), lds_infer, lds_learn, P.lds_edge_off + slots * 8);
    if (P.lds_agg_off && s->rec8 && no_binned_tiles(s.get()) && !getenv("DWX_NO_MERGED_APPLY")) {
      // split learning sweeps, one launch per mini-batch: the update as the next sweep kernel's prologue
      s->merge_lw32_off = (uint32_t)((lds_learn + 15) & ~(size_t)15);
      const size_t lds_merge = s->merge_lw32_off + (size_t)c.W * 4 + 16;
      s->merge_ok = lds_merge <= 160 * 1024;
      if (s->merge_ok)
        for (auto &k : s->kv.merged) { k.lds = lds_merge; k.allow(); }
    }
    if (P.lds_agg_off && c.W <= PERSIST_MAX_W && s->rec8 && no_binned_tiles(s.get()) && getenv("DWX_PERSIST") &&
        !getenv("DWX_NO_PERSIST")) {
      // a split learning sweep as one persistent launch (opt-in): at most one workgroup per CU, all resident
      s->persist_grid = rt::grid_barrier_blocks();
      if (const char *e = getenv("DWX_PERSIST_WG_PER_CU")) s->persist_grid *= (uint32_t)std::max(1L, std::min(3L, atol(e)));   // (experiment)
      s->persist_row_stride = (uint32_t)((2 * c.W + 15) / 16 * 16);
      s->d_persist_rows = (long long *)rt::dmalloc((size_t)2 * s->persist_grid * s->persist_row_stride * 8);
      s->d_persist_bar = (uint32_t *)rt::dmalloc(16);
      s->persist_w64_off = (uint32_t)((lds_learn + 15) & ~(size_t)15);
      s->persist_red_off = (uint32_t)((s->persist_w64_off + c.W * 12 + 15) & ~(size_t)15);
      s->kv.persist.lds = s->persist_red_off + (size_t)BLOCK_THREADS * 8 + 16;
      if (s->kv.persist.lds > 160 * 1024) s->persist_grid = 0;
      else s->kv.persist.allow();
    }
    rt::stream_sync(st);
    // the un-split sweep's curvature estimate is needed by the first dwx_sgd_plan: pay
    // for it here (one host pass over the records), not inside the first learning sweep
    {
      // SGD work per tile (records sgd_on_variable visits, src/factor_graph.cc:262-314):
      // what the mini-batch plan balances its cuts on
      std::vector<uint64_t> work(c.tiles.size() + 1, 0);
      parallel_ranges(c.tiles.size(), host_threads(), [&](uint64_t tb, uint64_t te) {
        for (uint64_t ti = tb; ti < te; ++ti) {
          const TileDesc &td = c.tiles[ti];
          uint64_t n = 0;
          for (uint32_t p = td.v0; p < td.v0 + td.nv; ++p) {
            if (!triggers_sgd(*opts, c.v_meta[p])) continue;
            for (uint32_t e = c.row_ptr[c.v_row[p]]; e < c.row_ptr[c.v_row[p + 1]]; ++e)
              n += !(c.edges[e].packed & EDGE_FIXED_FLAG);
          }
          work[ti + 1] = n;
        }
      }, 64);
      for (size_t i = 0; i < c.tiles.size(); ++i) work[i + 1] += work[i];
      s->sgd_work.swap(work);
      for (size_t l = 0; l + 1 < c.launch_off.size(); ++l)
        s->sgd_work_max_launch = std::max(s->sgd_work_max_launch,
                                          s->sgd_work[c.launch_tile[l + 1]] - s->sgd_work[c.launch_tile[l]]);
    }
    phase("kernel setup");
    (void)build_level(s.get(), 1);
    phase("static counts + gradient incidence list");
    if (opts->step_cap > 0) (void)row_sum_bound(s.get(), 1);
    phase("curvature estimate");
    devb::release_scratch(s->device, true);   // (the builds' cached temporaries: kept unless memory is tight)
    rt::stream_sync(st);
    rt::stage_trim();                          // (the uploads' pinned staging chunks)
  });
  if (rc != DWX_OK) return rc;
  *out = s.release();
  return DWX_OK;
}

int dwx_device_count(int32_t *count) {
  if (!count) return fail(DWX_E_INVALID, "null argument");
  return guarded([&]() { *count = rt::device_count(); });
}

int dwx_buffer_copy(dwx_sampler *s, void *dst, const void *src, uint64_t nbytes, int to_device) {
  if (!s || (nbytes && (!dst || !src))) return fail(DWX_E_INVALID, "null argument");
  return guarded([&]() {
    rt::set_device(s->device);
    if (to_device) rt::h2d(dst, src, nbytes, s->stream);
    else rt::d2h(dst, src, nbytes, s->stream);
    rt::stream_sync(s->stream);
  });
}

int dwx_device_init(int32_t device) {
  return guarded([&]() {
    rt::init_device(device);
    rt::oom_hook() = [](int dev) { devb::release_scratch(dev, false); };
    rt::dfree(rt::dmalloc(16));   // forces the context
  });
}

void dwx_sampler_destroy(dwx_sampler *s) {
  if (!s) return;
  try {
    rt::set_device(s->device);
    rt::stream_sync(s->stream);
  } catch (...) {
  }
  const int device = s->device;
  delete s;
  devb::release_scratch(device, false);
}


int dwx_sample_async(dwx_sampler *s) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    enqueue_inference(s);
    ++s->infer_sweeps;
  });
}

int dwx_sample_n_async(dwx_sampler *s, uint32_t n_sweeps) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    if (n_sweeps > 1 && multi_sweep_graph(s)) {
      enqueue_inference_multi(s, n_sweeps);
    } else {
      for (uint32_t k = 0; k < n_sweeps; ++k) enqueue_inference(s);
    }
    s->infer_sweeps += n_sweeps;
  });
}

int dwx_sgd_plan(dwx_sampler *s, double stepsize, uint32_t force_batches, uint32_t *batches,
                 uint32_t *n_chunks, double *effective_stepsize) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    make_plan(s, stepsize, force_batches);
    if (batches) *batches = s->plan_batches;
    if (n_chunks) *n_chunks = (uint32_t)s->plan_chunks.size();
    if (effective_stepsize) *effective_stepsize = plan_min_step(s);
  });
}

int dwx_sgd_curvature(dwx_sampler *s, uint32_t batches, double *lambda) {
  if (!s || !lambda) return fail(DWX_E_INVALID, "null argument");
  if (batches == 0) return fail(DWX_E_INVALID, "batches must be >= 1");
  return guarded([&]() { *lambda = row_sum_bound(s, batches); });
}

int dwx_sgd_plan_rows(dwx_sampler *s, uint32_t n_rows) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->plan_valid || !s->plan_level) return fail(DWX_E_INVALID, "no plan: call dwx_sgd_plan first");
  return guarded([&]() {
    dwx_sampler::Level &L = *s->plan_level;
    const uint64_t W = s->cg->W;
    if (!L.fast || s->plan_batches <= 1 || n_rows <= L.rows || !W) return;
    rt::set_device(s->device);
    long long *grown = (long long *)rt::dmalloc((size_t)n_rows * 2 * W * 8);
    rt::dmemset(grown, 0, (size_t)n_rows * 2 * W * 8, s->stream);
    rt::d2d(grown, L.d_t_static, (size_t)L.rows * 2 * W * 8, s->stream);
    rt::stream_sync(s->stream);
    rt::dfree(L.d_t_static);
    L.d_t_static = grown;
    L.rows = n_rows;
  });
}

int dwx_sgd_plan_force_dynamic(dwx_sampler *s, int on) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->plan_valid || !s->plan_level) return fail(DWX_E_INVALID, "no plan: call dwx_sgd_plan first");
  s->plan_force_dynamic = on != 0;
  return DWX_OK;
}

int dwx_sgd_get_chunks(dwx_sampler *s, uint64_t *chunk_range) {
  if (!s || !chunk_range) return fail(DWX_E_INVALID, "null argument");
  if (!s->plan_valid) return fail(DWX_E_INVALID, "no plan: call dwx_sgd_plan first");
  const CompiledGraph &c = *s->cg;
  size_t i = 0;
  for (const auto &ch : s->plan_chunks) { chunk_range[i++] = c.tile_v[ch.t0]; chunk_range[i++] = c.tile_v[ch.t1]; }
  return DWX_OK;
}

int dwx_sgd_accumulate_async(dwx_sampler *s, uint32_t chunk) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->plan_valid) return fail(DWX_E_INVALID, "no plan: call dwx_sgd_plan first");
  return guarded([&]() {
    s->cur_chunk = chunk;
    enqueue_learn_chunk(s, chunk);
  });
}

int dwx_sgd_apply_async(dwx_sampler *s) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->plan_valid) return fail(DWX_E_INVALID, "no plan: call dwx_sgd_plan first");
  return guarded([&]() { enqueue_apply(s); });
}

int dwx_sgd_finish(dwx_sampler *s) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  ++s->sweep;
  s->plan_valid = false;
  return DWX_OK;
}

int dwx_sample_sgd_async(dwx_sampler *s, double stepsize) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    make_plan(s, stepsize, 0);
    const size_t n = s->plan_chunks.size();
    auto enqueue_sweep = [&]() {
      for (size_t c = 0; c < n; ++c) {
        s->cur_chunk = (uint32_t)c;
        enqueue_learn_chunk(s, (uint32_t)c);
        if (s->plan_batches > 1 || c + 1 == n) enqueue_apply(s);
      }
    };
    // Graph replay (DWX_GRAPH=n in the environment: sweeps of at least n mini-batches; default
    // off).  A split sweep is a chain of 2-4 short dependent launches per mini-batch; from the
    // level's second sweep on (the first one has done every lazy allocation) it can be captured,
    // patched into the level's instantiated graph -- only the sweep counter and the step differ
    // from sweep to sweep -- and launched as ONE graph.  Measured on config 4's learning sweep
    // (64 mini-batches, 128 launches): 1.610 -> 1.603 ms, i.e. nothing: the chain is bound by the
    // latency of the chunk kernels themselves (17.5-22 us each for 3 us of work at full width,
    // profiles/r03/kernel_stats_cfg4learn.csv), not by the host's launches -- hence off.  Never
    // while kernels are being timed (the events would land inside the graph), nor on the sweep
    // that builds the level's own layout (host work and uploads).
    dwx_sampler::Level *L = s->plan_level;
    const char *genv = getenv("DWX_GRAPH");
    const int graph_min_chunks = genv ? atoi(genv) : 0;
    const bool replay = L && graph_min_chunks > 0 && s->plan_batches > 1 && n >= (size_t)graph_min_chunks &&
                        !s->timing && L->use_graph >= 0 && L->sweeps >= 1 &&
                        !(s->opts.plan_layouts == 0 && L->sweeps + 1 == layout_after_sweeps());
    if (enqueue_persistent_sweep(s)) {
      // (few weights, many mini-batches: the whole split sweep is one persistent launch; opt-in)
    } else if (!replay && enqueue_merged_sweep(s)) {
      // (few weights, split sweep: one launch per mini-batch, the update as the next one's prologue)
    } else if (!replay) {
      enqueue_sweep();
    } else {
      rt::set_device(s->device);
      rt::graph_t g = nullptr;
      rt::capture_begin(s->stream);
      try {
        enqueue_sweep();
        g = rt::capture_end(s->stream);
      } catch (...) {
        rt::capture_abandon(s->stream);
        L->use_graph = -1;
        throw;
      }
      bool launched = false;
      try {
        if (L->gexec && !rt::graph_exec_update(L->gexec, g)) { rt::graph_exec_destroy(L->gexec); L->gexec = nullptr; }
        if (!L->gexec) L->gexec = rt::graph_instantiate(g);
        rt::graph_launch(L->gexec, s->stream);
        launched = true;
        L->use_graph = 1;
        ++s->graph_launches;
      } catch (...) {
        // nothing of the captured sweep has run: this level goes back to plain launches for good
        L->use_graph = -1;
        rt::graph_exec_destroy(L->gexec);
        L->gexec = nullptr;
      }
      rt::graph_destroy(g);
      if (!launched) { --L->sweeps; enqueue_sweep(); }
    }
    ++s->sweep;
    s->plan_valid = false;
  });
}

int dwx_grad_pack_async(dwx_sampler *s, uint32_t shift, uint32_t bits, void **dev32, uint64_t *n_words) {
  if (!s || !dev32 || !n_words) return fail(DWX_E_INVALID, "null argument");
  if (shift == 0 || shift > 62) return fail(DWX_E_INVALID, "gradient shift out of range (dwx_graph_info.grad_shift)");
  if (bits != 32 && bits != 16) return fail(DWX_E_INVALID, "gradient counts travel as 32- or 16-bit integers");
  return guarded([&]() {
    rt::set_device(s->device);
    const uint32_t W = (uint32_t)s->cg->W;
    if (!s->d_grad32) {
      s->d_grad32 = (int *)rt::dmalloc((size_t)W * 4 + 4);
      s->d_pack_bad = (uint32_t *)rt::dmalloc(4);
      rt::dmemset(s->d_pack_bad, 0, 4, s->stream);
    }
    const uint32_t words = bits == 32 ? W : (W + 1u) / 2u;
    const unsigned grid = std::max(1u, std::min((words + BLOCK_THREADS - 1) / BLOCK_THREADS, 1024u));
    if (bits == 32)
      rt::launch(grad_pack32_kernel, grid, BLOCK_THREADS, 0, s->stream, (const long long *)s->d_grad, s->d_grad32, W, shift,
                 s->d_pack_bad);
    else
      rt::launch(grad_pack16_kernel, grid, BLOCK_THREADS, 0, s->stream, (const long long *)s->d_grad, s->d_grad32, W, shift,
                 s->d_pack_bad);
    s->pack_check_pending = true;
    *dev32 = s->d_grad32;
    *n_words = words;
  });
}

int dwx_grad_unpack_async(dwx_sampler *s, uint32_t shift, uint32_t bits) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->d_grad32) return fail(DWX_E_INVALID, "dwx_grad_unpack_async without dwx_grad_pack_async");
  if (bits != 32 && bits != 16) return fail(DWX_E_INVALID, "gradient counts travel as 32- or 16-bit integers");
  return guarded([&]() {
    rt::set_device(s->device);
    const uint32_t W = (uint32_t)s->cg->W;
    const uint32_t words = bits == 32 ? W : (W + 1u) / 2u;
    const unsigned grid = std::max(1u, std::min((words + BLOCK_THREADS - 1) / BLOCK_THREADS, 1024u));
    if (bits == 32)
      rt::launch(grad_unpack32_kernel, grid, BLOCK_THREADS, 0, s->stream, (const int *)s->d_grad32, s->d_grad, W, shift);
    else
      rt::launch(grad_unpack16_kernel, grid, BLOCK_THREADS, 0, s->stream, (const int *)s->d_grad32, s->d_grad, W, shift);
  });
}

int dwx_grad_pack32_async(dwx_sampler *s, uint32_t shift, void **dev32, uint64_t *n) {
  return dwx_grad_pack_async(s, shift, 32, dev32, n);
}
int dwx_grad_unpack32_async(dwx_sampler *s, uint32_t shift) { return dwx_grad_unpack_async(s, shift, 32); }

int dwx_wait(dwx_sampler *s) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    rt::set_device(s->device);
    rt::stream_sync(s->stream);
    if (s->persist_check_pending) {   // (a persistent split sweep whose workgroups were not all resident gave up)
      uint32_t bar[4] = {0, 0, 0, 0};
      rt::d2h(bar, s->d_persist_bar, 16, s->stream);
      rt::stream_sync(s->stream);
      s->persist_check_pending = false;
      if (bar[1]) {
        s->persist_grid = 0;          // (never again on this sampler)
        throw std::runtime_error("a persistent learning sweep gave up at its grid barrier (its workgroups were not all "
                                 "resident): the weights and chains of that sweep are invalid; DWX_NO_PERSIST=1 disables it");
      }
    }
    if (s->pack_check_pending) {      // (the 32-bit gradient counts: exact by construction, verified here)
      uint32_t bad = 0;
      rt::d2h(&bad, s->d_pack_bad, 4, s->stream);
      rt::stream_sync(s->stream);
      s->pack_check_pending = false;
      if (bad) rt::dmemset(s->d_pack_bad, 0, 4, s->stream);   // (a later pack reports its own count only)
      if (bad) throw std::runtime_error("dwx_grad_pack_async: " + std::to_string(bad) +
                                        " gradient sums were not multiples of 2^shift or did not fit the count width");
    }
  });
}

int dwx_get_weights(dwx_sampler *s, double *out) {
  if (!s || !out) return fail(DWX_E_INVALID, "null argument");
  return guarded([&]() {
    rt::set_device(s->device);
    rt::d2h(out, s->d_weights, s->cg->W * 8, s->stream);
    rt::stream_sync(s->stream);
  });
}

int dwx_set_weights(dwx_sampler *s, const double *in) {
  if (!s || !in) return fail(DWX_E_INVALID, "null argument");
  {
    std::string why;
    const int bad = check_sampling_weights(*s->cg, in, &why);
    if (bad) return fail(bad == 2 ? DWX_E_LIMIT : DWX_E_INVALID, why);
  }
  return guarded([&]() {
    rt::set_device(s->device);
    const uint32_t W = (uint32_t)s->cg->W;
    weights_change(s);
    keep_snapshot(s);
    rt::h2d(s->d_weights, in, (size_t)W * 8, s->stream);
    if (W) {
      const unsigned grid = std::min<unsigned>((W + BLOCK_THREADS - 1) / BLOCK_THREADS, 2048u);
      rt::launch(refresh_w32_kernel, grid, BLOCK_THREADS, 0, s->stream,
                 (const double *)s->d_weights, s->d_w32, W);
    }
    rt::stream_sync(s->stream);
  });
}

int dwx_average_weights_async(dwx_sampler *s, uint32_t n_replicas) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (n_replicas == 0) return fail(DWX_E_INVALID, "n_replicas must be >= 1");
  return guarded([&]() {
    rt::set_device(s->device);
    const uint32_t W = (uint32_t)s->cg->W;
    if (!W) return;
    weights_change(s);
    if (!s->d_w_init) {
      s->d_w_init = upload(s->cg->w_init, s->stream);
      rt::stream_sync(s->stream);
    }
    keep_snapshot(s);
    const unsigned grid = std::min<unsigned>((W + BLOCK_THREADS - 1) / BLOCK_THREADS, 2048u);
    rt::launch(average_weights_kernel, grid, BLOCK_THREADS, 0, s->stream, s->d_weights, s->d_w32,
               (const uint8_t *)s->d_w_fixed, (const double *)s->d_w_init, W, (double)n_replicas);
  });
}

int dwx_clear_tallies(dwx_sampler *s) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    rt::set_device(s->device);
    rt::dmemset(s->d_tally, 0, s->cg->R * 4, s->stream);
    if (s->d_rb) rt::dmemset(s->d_rb, 0, s->cg->R * 8, s->stream);
    s->trace_next = s->trace_count = 0;   // (the planes are overwritten whole before they are read again)
    s->infer_sweeps = 0;
  });
}

int dwx_rb_enable(dwx_sampler *s, int on) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!on) { s->rb_on = false; return DWX_OK; }
  if (!s->d_rb) {
    int rc = guarded([&]() {
      rt::set_device(s->device);
      const size_t bytes = ((size_t)s->cg->R + 1) * 8;
      void *p = optional_dmalloc(bytes);
      if (!p) return;
      rt::dmemset(p, 0, bytes, s->stream);
      s->d_rb = (unsigned long long *)p;
    });
    if (rc != DWX_OK) return rc;
    if (!s->d_rb) return fail(DWX_E_NOMEM, "no device memory for the Rao-Blackwellised sums (8 bytes per value row)");
  }
  s->rb_on = true;
  return DWX_OK;
}

int dwx_get_rb_sums(dwx_sampler *s, uint64_t *sums, uint64_t *nsamples) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->d_rb) return fail(DWX_E_INVALID, "Rao-Blackwellised sums were never enabled (dwx_rb_enable)");
  int rc = DWX_OK;
  if (sums) rc = guarded([&]() {
    const CompiledGraph &c = *s->cg;
    rt::set_device(s->device);
    RawArray<unsigned long long> t(c.R);
    rt::d2h(t.data(), s->d_rb, c.R * 8, s->stream);
    rt::stream_sync(s->stream);
    parallel_ranges(c.Vo, host_threads(), [&](uint64_t pb, uint64_t pe) {
      for (uint64_t p = pb; p < pe; ++p) {
        const uint64_t rb = c.ref_var_val_base[c.perm[p]];
        for (uint32_t r = c.v_row[p]; r < c.v_row[p + 1]; ++r) sums[rb + (r - c.v_row[p])] = t[r];
      }
    });
  });
  if (rc != DWX_OK) return rc;
  return nsamples ? dwx_get_tallies(s, nullptr, nsamples) : DWX_OK;
}

int dwx_trace_enable(dwx_sampler *s, uint32_t capacity_sweeps) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!capacity_sweeps) { s->trace_on = false; return DWX_OK; }
  const CompiledGraph &c = *s->cg;
  if (c.max_card > 256) return fail(DWX_E_LIMIT, "the sample trace holds a byte per variable: cardinalities up to 256");
  if (!s->d_trace || capacity_sweeps != s->trace_cap) {
    bool boolean = true;
    for (uint64_t p = 0; p < c.Vo && boolean; ++p) boolean = !(c.v_meta[p] & VM_CATEGORICAL);
    const uint32_t bits = boolean ? 1u : 8u;
    // a plane: whole 8-byte words, ceil(Vo / 64) of them at a bit per position, ceil(Vo / 8) at a byte; no other padding
    const uint64_t words = bits == 1 ? (c.Vo + 63) / 64 : (c.Vo + 7) / 8;
    const size_t bytes = std::max<size_t>((size_t)capacity_sweeps * words * 8, 8);
    void *p = nullptr;
    int rc = guarded([&]() {
      rt::set_device(s->device);
      rt::stream_sync(s->stream);   // (a sweep in flight may still write the ring about to be freed)
      rt::dfree(s->d_trace);
      s->d_trace = nullptr; s->trace_on = false; s->trace_cap = s->trace_next = s->trace_count = 0;
      p = optional_dmalloc(bytes);
      if (p) rt::dmemset(p, 0, bytes, s->stream);
    });
    if (rc != DWX_OK) return rc;
    if (!p) return fail(DWX_E_NOMEM, "no device memory for the sample trace (capacity x ceil(V / 64) x 8 bytes, or x V bytes)");
    s->d_trace = (unsigned long long *)p;
    s->trace_cap = capacity_sweeps; s->trace_words = (uint32_t)words; s->trace_bits = bits;
    s->trace_ids.assign(capacity_sweeps, 0);
  }
  s->trace_on = true;
  return DWX_OK;
}

int dwx_trace_info(dwx_sampler *s, uint64_t *count, uint64_t *capacity, uint64_t *sweep_ids) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (count) *count = s->trace_count;
  if (capacity) *capacity = s->trace_cap;
  if (sweep_ids)
    for (uint32_t e = 0; e < s->trace_count; ++e)
      sweep_ids[e] = s->trace_ids[(s->trace_next + s->trace_cap - s->trace_count + e) % s->trace_cap];
  return DWX_OK;
}

int dwx_trace_read(dwx_sampler *s, uint64_t first_entry, uint64_t n_entries, const uint64_t *vids, uint64_t n_vids,
                   uint8_t *out) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->d_trace) return fail(DWX_E_INVALID, "the sample trace was never enabled (dwx_trace_enable)");
  if (first_entry > s->trace_count || n_entries > s->trace_count - first_entry)
    return fail(DWX_E_INVALID, "entries outside the sample trace (dwx_trace_info: count)");
  const CompiledGraph &c = *s->cg;
  if (!vids) n_vids = c.Vo;
  if (n_entries > 0xFFFFFFFFull) return fail(DWX_E_INVALID, "entries outside the sample trace");
  if (!n_entries || !n_vids) return DWX_OK;
  if (!out) return fail(DWX_E_INVALID, "null argument");
  std::vector<uint32_t> pos(n_vids);
  for (uint64_t i = 0; i < n_vids; ++i) {
    const uint64_t v = vids ? vids[i] : i;
    if (v >= c.V) return fail(DWX_E_INVALID, "variable id out of range");
    pos[i] = c.pos[v];
    if (pos[i] >= c.Vo) return fail(DWX_E_INVALID, "ghost variables are not traced");
  }
  return guarded([&]() {
    rt::set_device(s->device);
    const uint64_t total = n_entries * n_vids;
    uint32_t *d_pos = upload(pos, s->stream);
    unsigned char *d_out = nullptr;
    try {
      d_out = (unsigned char *)rt::dmalloc(total);
      const uint32_t slot0 = (uint32_t)((s->trace_next + s->trace_cap - s->trace_count + first_entry) % s->trace_cap);
      const unsigned grid = (unsigned)std::min<uint64_t>((total + BLOCK_THREADS - 1) / BLOCK_THREADS, 256u * 16u);
      auto go = [&](auto kernel) {
        rt::launch(kernel, grid, BLOCK_THREADS, 0, s->stream, (const unsigned long long *)s->d_trace, s->trace_words,
                   s->trace_cap, slot0, (uint32_t)n_entries, (const uint32_t *)d_pos, n_vids, d_out);
      };
      if (s->trace_bits == 1) go(trace_gather_kernel<1>); else go(trace_gather_kernel<8>);
      rt::d2h(out, d_out, total, s->stream);
      rt::stream_sync(s->stream);
    } catch (...) {
      rt::dfree(d_pos); rt::dfree(d_out);
      throw;
    }
    rt::dfree(d_pos); rt::dfree(d_out);
  });
}

int dwx_trace_diagnostics(dwx_sampler *s, uint32_t max_lag, double rhat_threshold, double *rhat, double *ess,
                          uint8_t *flags, dwx_trace_diag_summary *summary) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->d_trace) return fail(DWX_E_INVALID, "the sample trace was never enabled (dwx_trace_enable)");
  if (s->trace_count < 4) return fail(DWX_E_INVALID, "split-R-hat needs at least 4 entries in the sample trace");
  if (max_lag < 1 || max_lag > DIAG_MAX_LAG) return fail(DWX_E_INVALID, "max_lag must be 1 .. 64");
  if (!rhat && !ess && !flags && !summary) return fail(DWX_E_INVALID, "null argument: nothing to return");
  if (s->trace_count > 0x7FFFFFFFu) return fail(DWX_E_LIMIT, "the diagnostics take at most 2^31 - 1 entries");
  const CompiledGraph &c = *s->cg;
  const uint32_t n = s->trace_count, n_rows = c.v_row[c.Vo];
  const uint32_t slot0 = (uint32_t)(((uint64_t)s->trace_next + s->trace_cap - n) % s->trace_cap);
  const bool bit = s->trace_bits == 1;
  const unsigned block = bit ? DIAG_BIT_THREADS : DIAG_BYTE_THREADS;
  const unsigned grid = bit ? (s->trace_words + block / 64u - 1u) / (block / 64u) : (n_rows + block - 1u) / block;
  if (!grid) return fail(DWX_E_INVALID, "no owned variables");
  bool nomem = false;
  unsigned long long counts[4] = {0, 0, 0, 0};
  DiagPartial best;
  int rc = guarded([&]() {
    rt::set_device(s->device);
    void *d_rhat = nullptr, *d_ess = nullptr, *d_flags = nullptr, *d_counts = nullptr, *d_part = nullptr;
    auto release = [&]() { rt::dfree(d_rhat); rt::dfree(d_ess); rt::dfree(d_flags); rt::dfree(d_counts); rt::dfree(d_part); };
    try {
      d_counts = optional_dmalloc(sizeof(counts));
      d_part = optional_dmalloc((size_t)grid * sizeof(DiagPartial));
      if (rhat) d_rhat = optional_dmalloc((size_t)n_rows * 8);
      if (ess) d_ess = optional_dmalloc((size_t)n_rows * 8);
      if (flags) d_flags = optional_dmalloc(n_rows);
      if (!d_counts || !d_part || (rhat && !d_rhat) || (ess && !d_ess) || (flags && !d_flags)) {
        nomem = true;
        release();
        return;
      }
      rt::dmemset(d_counts, 0, sizeof(counts), s->stream);
      auto go = [&](auto kernel) {
        rt::launch(kernel, grid, block, 0, s->stream, (const unsigned long long *)s->d_trace, s->trace_words, s->trace_cap,
                   slot0, n, (uint32_t)c.Vo, n_rows, (const uint32_t *)s->d_v_row, (const uint32_t *)s->d_v_meta, max_lag,
                   rhat_threshold, (double *)d_rhat, (double *)d_ess, (unsigned char *)d_flags,
                   (unsigned long long *)d_counts, (DiagPartial *)d_part);
      };
      if (bit) go(trace_diag_kernel<1>); else go(trace_diag_kernel<8>);
      rt::launch(trace_diag_fold_kernel, 1u, BLOCK_THREADS, 0, s->stream, (DiagPartial *)d_part, (uint32_t)grid);
      rt::d2h(counts, d_counts, sizeof(counts), s->stream);
      rt::d2h(&best, d_part, sizeof(best), s->stream);
      // device row order -> the reference numbering: the tallies' translation
      auto fetch = [&](auto *out, const void *d_arr) {
        typedef typename std::remove_pointer<decltype(out)>::type T;
        RawArray<T> t(n_rows);
        rt::d2h(t.data(), d_arr, (size_t)n_rows * sizeof(T), s->stream);
        rt::stream_sync(s->stream);
        parallel_ranges(c.Vo, host_threads(), [&](uint64_t pb, uint64_t pe) {
          for (uint64_t p = pb; p < pe; ++p) {
            const uint64_t rb = c.ref_var_val_base[c.perm[p]];
            for (uint32_t r = c.v_row[p]; r < c.v_row[p + 1]; ++r) out[rb + (r - c.v_row[p])] = t[r];
          }
        });
      };
      if (rhat) fetch(rhat, d_rhat);
      if (ess) fetch(ess, d_ess);
      if (flags) fetch(flags, d_flags);
      rt::stream_sync(s->stream);
    } catch (...) {
      release();
      throw;
    }
    release();
  });
  if (rc != DWX_OK) return rc;
  if (nomem) return fail(DWX_E_NOMEM, "no device memory for the diagnostics' temporary arrays (up to 17 bytes per value row)");
  if (summary) {
    auto ref_row = [&](uint32_t r) -> uint64_t {
      if (r == DIAG_NO_ROW) return ~0ull;
      const uint32_t *first = c.v_row.data();
      const uint64_t p = (uint64_t)(std::upper_bound(first, first + c.Vo + 1, r) - first) - 1;   // v_row[p] <= r < v_row[p + 1]
      return c.ref_var_val_base[c.perm[p]] + (r - c.v_row[p]);
    };
    summary->n_entries = n;
    summary->max_lag = max_lag;
    summary->contiguous = 1;
    for (uint32_t e = 1; e < n; ++e)
      if (s->trace_ids[(slot0 + e) % s->trace_cap] != s->trace_ids[(slot0 + e - 1) % s->trace_cap] + 1) summary->contiguous = 0;
    summary->rows_finite = counts[0]; summary->rows_constant = counts[1];
    summary->rows_truncated = counts[2]; summary->rows_rhat_above = counts[3];
    const double nan = std::nan("");
    summary->max_rhat = best.max_row == DIAG_NO_ROW ? nan : best.max_rhat; summary->max_rhat_row = ref_row(best.max_row);
    summary->min_ess = best.min_row == DIAG_NO_ROW ? nan : best.min_ess; summary->min_ess_row = ref_row(best.min_row);
  }
  return DWX_OK;
}

int dwx_trace_cooccurrence(dwx_sampler *s, const uint64_t *rows_a, const uint64_t *rows_b, uint64_t n_pairs,
                           uint64_t first_entry, uint64_t n_entries, uint64_t *n_ab, uint64_t *n_a, uint64_t *n_b) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  if (!s->d_trace) return fail(DWX_E_INVALID, "the sample trace was never enabled (dwx_trace_enable)");
  if (n_pairs > 0xFFFFFFFFull) return fail(DWX_E_LIMIT, "the co-occurrence counts take at most 2^32 - 1 pairs a call");
  if (n_entries > 0x7FFFFFFFull || s->trace_cap > 0x7FFFFFFFu)
    return fail(DWX_E_LIMIT, "the co-occurrence counts take at most 2^31 - 1 entries, of a ring of at most 2^31 - 1");
  if (first_entry > s->trace_count || n_entries > s->trace_count - first_entry)
    return fail(DWX_E_INVALID, "entries outside the sample trace (dwx_trace_info: count)");
  if (!n_pairs) return DWX_OK;
  if (!rows_a || !rows_b || !n_ab) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *s->cg;
  const bool bit = s->trace_bits == 1;
  // reference row -> (device position, dense value), once per call: the variable by a search in the rows' bases
  // (the inverse of the translation dwx_trace_diagnostics returns its rows with), its position from CompiledGraph::pos
  std::vector<uint32_t> pos[2];
  std::vector<unsigned char> val[2];
  RawArray<unsigned long long> counts;   // (staged: an error leaves the caller's arrays as they were)
  // (ghost variables have no rows in the reference numbering -- graph_compile.cc: rows_of -- so every row < R is an owned
  // variable's and what would be a ghost's row is out of range; the position check below is a guard, not an error case)
  std::atomic<int> bad{0};               // 1: a row out of range, 2: the guard
  int rc = guarded([&]() {
    for (int side = 0; side < 2; ++side) {
      const uint64_t *rows = side ? rows_b : rows_a;
      pos[side].resize(n_pairs);
      if (!bit) val[side].resize(n_pairs);
      const uint64_t *first = c.ref_var_val_base.data();
      parallel_ranges(n_pairs, host_threads(), [&](uint64_t ib, uint64_t ie) {
        for (uint64_t i = ib; i < ie; ++i) {
          if (rows[i] >= c.R) { bad = 1; return; }
          const uint64_t v = (uint64_t)(std::upper_bound(first, first + c.V, rows[i]) - first) - 1;   // base[v] <= row < base[v + 1]
          const uint32_t p = c.pos[v];
          if (p >= c.Vo) { bad = 2; return; }
          pos[side][i] = p;
          if (!bit) val[side][i] = (c.v_meta[p] & VM_CATEGORICAL) ? (unsigned char)(rows[i] - first[v]) : (unsigned char)1;
        }
      });
    }
    if (n_entries) counts.reset(3 * n_pairs);
  });
  if (rc != DWX_OK) return rc;
  if (bad == 1) return fail(DWX_E_INVALID, "value row out of range (dwx_graph_info: num_values)");
  if (bad) return fail(DWX_E_INVALID, "ghost variables are not traced");
  auto zero = [&](uint64_t *out) { if (out) std::fill(out, out + n_pairs, (uint64_t)0); };
  if (!n_entries) { zero(n_ab); zero(n_a); zero(n_b); return DWX_OK; }
  bool nomem = false;
  rc = guarded([&]() {
    rt::set_device(s->device);
    void *d_pos[2] = {nullptr, nullptr}, *d_val[2] = {nullptr, nullptr}, *d_out = nullptr;
    auto release = [&]() { for (int k = 0; k < 2; ++k) { rt::dfree(d_pos[k]); rt::dfree(d_val[k]); } rt::dfree(d_out); };
    try {
      d_out = optional_dmalloc(3 * n_pairs * 8);
      for (int k = 0; k < 2; ++k) {
        d_pos[k] = optional_dmalloc(n_pairs * 4);
        if (!bit) d_val[k] = optional_dmalloc(n_pairs);
      }
      if (!d_out || !d_pos[0] || !d_pos[1] || (!bit && (!d_val[0] || !d_val[1]))) {
        nomem = true;
        release();
        return;
      }
      for (int k = 0; k < 2; ++k) {
        rt::h2d(d_pos[k], pos[k].data(), n_pairs * 4, s->stream);
        if (!bit) rt::h2d(d_val[k], val[k].data(), n_pairs, s->stream);
      }
      const uint32_t slot0 = (uint32_t)((s->trace_next + s->trace_cap - s->trace_count + first_entry) % s->trace_cap);
      const unsigned grid = (unsigned)std::min<uint64_t>((n_pairs + BLOCK_THREADS - 1) / BLOCK_THREADS, COOC_MAX_BLOCKS);
      auto go = [&](auto kernel) {
        rt::launch(kernel, grid, BLOCK_THREADS, 0, s->stream, (const unsigned long long *)s->d_trace, s->trace_words,
                   s->trace_cap, slot0, (uint32_t)n_entries, (const uint32_t *)d_pos[0], (const uint32_t *)d_pos[1],
                   (const unsigned char *)d_val[0], (const unsigned char *)d_val[1], n_pairs, (unsigned long long *)d_out);
      };
      if (bit) go(trace_cooc_kernel<1>); else go(trace_cooc_kernel<8>);
      rt::d2h(counts.data(), d_out, 3 * n_pairs * 8, s->stream);
      rt::stream_sync(s->stream);
    } catch (...) {
      release();
      throw;
    }
    release();
  });
  if (rc != DWX_OK) return rc;
  if (nomem) return fail(DWX_E_NOMEM, "no device memory for the co-occurrence counts' temporary arrays (up to 34 bytes per pair)");
  uint64_t *outs[3] = {n_ab, n_a, n_b};
  for (int k = 0; k < 3; ++k)
    if (outs[k]) std::copy(counts.data() + k * n_pairs, counts.data() + (k + 1) * n_pairs, outs[k]);
  return DWX_OK;
}

namespace {
// dwx_score / dwx_trace_score: the device copy of the graph's factor-major table, uploaded by the first call.
// *nomem: the device has no room (nothing is kept, the sampler stays usable).
void ensure_score_table(dwx_sampler *s, bool *nomem) {
  if (s->score_ready) return;
  const CompiledGraph &c = *s->cg;
  void *p[4] = {nullptr, nullptr, nullptr, nullptr};
  const void *h[4] = {c.frecs.data(), c.fvifs.data(), c.ffval64.data(), c.fwide.data()};
  const size_t bytes[4] = {c.frecs.size() * sizeof(FactorRec), c.fvifs.size() * sizeof(VifRec), c.ffval64.size() * 8,
                           c.fwide.size() * 4};
  try {
    for (int i = 0; i < 4; ++i) {
      if (!bytes[i]) continue;
      p[i] = optional_dmalloc(bytes[i]);
      if (!p[i]) {
        for (int k = 0; k < 4; ++k) rt::dfree(p[k]);
        *nomem = true;
        return;
      }
      rt::h2d(p[i], h[i], bytes[i], s->stream);
    }
    rt::stream_sync(s->stream);
  } catch (...) {
    for (int k = 0; k < 4; ++k) rt::dfree(p[k]);
    throw;
  }
  s->d_frecs = (FactorRec *)p[0]; s->d_fvifs = (VifRec *)p[1]; s->d_ffval64 = (double *)p[2]; s->d_fwide = (uint32_t *)p[3];
  s->score_ready = true;
}

// The scores of n states into out[n] (staged by the caller: an error leaves its arrays as they were).  mode 0: the
// one state src = a chain's assignments; mode 1 / 8: entries of the ring, the first in plane slot0.  Passes of
// SCORE_EB entries, each a launch over the table and one over the wide factors.  -> 0, DWX_E_NOMEM or DWX_E_LIMIT.
int run_score(dwx_sampler *s, int mode, const void *src, uint32_t slot0, uint64_t n, double *out) {
  const CompiledGraph &c = *s->cg;
  if (!c.F) { std::fill(out, out + n, 0.0); return DWX_OK; }
  bool nomem = false;
  ensure_score_table(s, &nomem);
  if (nomem) return DWX_E_NOMEM;
  std::vector<unsigned long long> acc(2 * n + 1);
  unsigned long long *d_acc = (unsigned long long *)optional_dmalloc(acc.size() * 8);
  if (!d_acc) return DWX_E_NOMEM;
  try {
    rt::dmemset(d_acc, 0, acc.size() * 8, s->stream);
    const uint32_t F = (uint32_t)c.F, n_wide = (uint32_t)c.fwide.size();
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)F + BLOCK_THREADS - 1) / BLOCK_THREADS, SCORE_MAX_BLOCKS);
    const unsigned wgrid = (unsigned)std::min<uint64_t>(((uint64_t)n_wide + 3) / 4, SCORE_MAX_BLOCKS);
    const uint32_t eb = mode == 0 ? 1u : (uint32_t)SCORE_EB;
    for (uint64_t e0 = 0; e0 < n; e0 += eb) {
      const uint32_t ne = (uint32_t)std::min<uint64_t>(eb, n - e0);
      const uint32_t slot = mode == 0 ? 0u : (uint32_t)(((uint64_t)slot0 + e0) % s->trace_cap);
      unsigned long long *a = d_acc + 2 * e0;
      unsigned *flag = (unsigned *)(d_acc + 2 * n);
      auto go = [&](auto lane_kernel, auto wide_kernel) {
        rt::launch(lane_kernel, grid, BLOCK_THREADS, 0, s->stream, (const FactorRec *)s->d_frecs, (const double *)s->d_ffval64,
                   (const VifRec *)s->d_fvifs, F, (const double *)s->d_weights, src, s->trace_words, s->trace_cap, slot, ne, a, flag);
        if (n_wide)
          rt::launch(wide_kernel, wgrid, BLOCK_THREADS, 0, s->stream, (const FactorRec *)s->d_frecs, (const double *)s->d_ffval64,
                     (const VifRec *)s->d_fvifs, (const uint32_t *)s->d_fwide, n_wide, (const double *)s->d_weights, src,
                     s->trace_words, s->trace_cap, slot, ne, a, flag);
      };
      if (mode == 0) go(score_kernel<0, 1>, score_wide_kernel<0, 1>);
      else if (mode == 1) go(score_kernel<1, SCORE_EB>, score_wide_kernel<1, SCORE_EB>);
      else go(score_kernel<8, SCORE_EB>, score_wide_kernel<8, SCORE_EB>);
    }
    rt::d2h(acc.data(), d_acc, acc.size() * 8, s->stream);
    rt::stream_sync(s->stream);
  } catch (...) {
    rt::dfree(d_acc);
    throw;
  }
  rt::dfree(d_acc);
  if ((uint32_t)acc[2 * n]) return DWX_E_LIMIT;
  for (uint64_t e = 0; e < n; ++e) {
    // one correctly rounded conversion of the exact integer sum, then an exact scaling
    const __int128 total = (__int128)(long long)acc[2 * e] * ((__int128)1 << 32) + (__int128)acc[2 * e + 1];
    out[e] = (double)total * (1.0 / 4294967296.0);
  }
  return DWX_OK;
}

int score_error(int rc) {
  if (rc == DWX_E_NOMEM) return fail(rc, "no device memory for the factor table (dwx_graph_info: factor_table_bytes) or the sums of the call");
  return fail(rc, "a term w * (sign * feature value) of the score is not finite or reaches 2^30: outside the sums' domain");
}
}  // namespace

int dwx_score(dwx_sampler *s, int chain, double *score) {
  if (!s || !score) return fail(DWX_E_INVALID, "null argument");
  if (!s->cg->keep_factors) return fail(DWX_E_INVALID, "the graph was compiled without dwx_compile_opts.keep_factors");
  if (chain != 0 && chain != 1) return fail(DWX_E_INVALID, "chain must be 0 (free) or 1 (evidence)");
  double v = 0.0;
  int code = DWX_OK;
  int rc = guarded([&]() {
    rt::set_device(s->device);
    flush_pending(s, chain == 0 ? 1 : 2);
    code = run_score(s, 0, chain == 0 ? s->d_assign_free : s->d_assign_evid, 0u, 1, &v);
  });
  if (rc != DWX_OK) return rc;
  if (code != DWX_OK) return score_error(code);
  *score = v;
  return DWX_OK;
}

int dwx_trace_score(dwx_sampler *s, uint64_t first_entry, uint64_t n_entries, double *scores, uint64_t *best_entry) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  const CompiledGraph &c = *s->cg;
  if (!c.keep_factors) return fail(DWX_E_INVALID, "the graph was compiled without dwx_compile_opts.keep_factors");
  if (!s->d_trace) return fail(DWX_E_INVALID, "the sample trace was never enabled (dwx_trace_enable)");
  if (c.Vo != c.V) return fail(DWX_E_INVALID, "ghost variables are not traced: a shard's trace holds no joint state to score");
  if (first_entry > s->trace_count || n_entries > s->trace_count - first_entry)
    return fail(DWX_E_INVALID, "entries outside the sample trace (dwx_trace_info: count)");
  if (!n_entries) {
    if (best_entry) *best_entry = ~0ull;
    return DWX_OK;
  }
  if (!scores) return fail(DWX_E_INVALID, "null argument");
  std::vector<double> v;
  int code = DWX_OK;
  int rc = guarded([&]() {
    v.resize(n_entries);
    rt::set_device(s->device);
    const uint32_t slot0 = (uint32_t)(((uint64_t)s->trace_next + s->trace_cap - s->trace_count + first_entry) % s->trace_cap);
    code = run_score(s, (int)s->trace_bits, s->d_trace, slot0, n_entries, v.data());
  });
  if (rc != DWX_OK) return rc;
  if (code != DWX_OK) return score_error(code);
  uint64_t best = 0;
  for (uint64_t e = 1; e < n_entries; ++e)
    if (v[e] > v[best]) best = e;           // (strictly: the oldest on a tie)
  std::copy(v.begin(), v.end(), scores);
  if (best_entry) *best_entry = first_entry + best;
  return DWX_OK;
}

namespace {
// a launch of the per-weight sums covers this many entries; 0: the whole range in ONE launch, the kernel loops
// over the groups of WSTATS_EB entries itself (profiles/r18/README.md has both forms' times)
#ifndef DWX_WSTATS_PASS_ENTRIES
#define DWX_WSTATS_PASS_ENTRIES 0
#endif

// dwx_weight_stats / dwx_trace_weight_stats: sum over n states and over the factors on each weight of sign * fval
// into out[W] (staged by the caller).  mode / src / slot0 as run_score.  -> 0, DWX_E_NOMEM, or DWX_E_LIMIT with
// *limit_wid < W: the term-count guard refused (nothing was launched), *limit_wid == W: a term outside the domain.
int run_weight_stats(dwx_sampler *s, int mode, const void *src, uint32_t slot0, uint64_t n, double *out, uint64_t *limit_wid) {
  const CompiledGraph &c = *s->cg;
  std::fill(out, out + c.W, 0.0);
  *limit_wid = c.W;
  if (!c.F || !n || !c.W) return DWX_OK;
  bool nomem = false;
  ensure_score_table(s, &nomem);
  if (nomem) return DWX_E_NOMEM;
  if (!s->wstats_ready) {
    std::vector<uint32_t> count(c.W, 0u);
    for (uint64_t f = 0; f < c.F; ++f) ++count[c.frecs[f].wid];
    const auto m = std::max_element(count.begin(), count.end());
    s->wstats_max_count = *m;
    s->wstats_max_wid = (uint64_t)(m - count.begin());
    s->wstats_ready = true;
  }
  // the two-limb sums hold fewer than 2^32 terms per weight (n <= trace capacity < 2^32: the product fits 64 bits)
  if (n * s->wstats_max_count >= (1ull << 32)) {
    *limit_wid = s->wstats_max_wid;
    return DWX_E_LIMIT;
  }
  std::vector<unsigned long long> acc(2 * c.W + 1);
  unsigned long long *d_acc = (unsigned long long *)optional_dmalloc(acc.size() * 8);
  if (!d_acc) return DWX_E_NOMEM;
  try {
    rt::dmemset(d_acc, 0, acc.size() * 8, s->stream);
    const uint32_t F = (uint32_t)c.F, n_wide = (uint32_t)c.fwide.size();
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)F + BLOCK_THREADS - 1) / BLOCK_THREADS, WSTATS_MAX_BLOCKS);
    const unsigned wgrid = (unsigned)std::min<uint64_t>(((uint64_t)n_wide + 3) / 4, WSTATS_MAX_BLOCKS);
    unsigned *flag = (unsigned *)(d_acc + 2 * c.W);
    const uint64_t pass = (mode == 0 || !DWX_WSTATS_PASS_ENTRIES) ? n : (uint64_t)DWX_WSTATS_PASS_ENTRIES;
    for (uint64_t e0 = 0; e0 < n; e0 += pass) {
      const uint32_t ne = (uint32_t)std::min<uint64_t>(pass, n - e0);
      const uint32_t slot = mode == 0 ? 0u : (uint32_t)(((uint64_t)slot0 + e0) % s->trace_cap);
      auto go = [&](auto lane_kernel, auto wide_kernel) {
        rt::launch(lane_kernel, grid, BLOCK_THREADS, 0, s->stream, (const FactorRec *)s->d_frecs, (const double *)s->d_ffval64,
                   (const VifRec *)s->d_fvifs, F, src, s->trace_words, s->trace_cap, slot, ne, d_acc, flag);
        if (n_wide)
          rt::launch(wide_kernel, wgrid, BLOCK_THREADS, 0, s->stream, (const FactorRec *)s->d_frecs, (const double *)s->d_ffval64,
                     (const VifRec *)s->d_fvifs, (const uint32_t *)s->d_fwide, n_wide, src, s->trace_words, s->trace_cap, slot, ne,
                     d_acc, flag);
      };
      if (mode == 0) go(weight_stats_kernel<0, 1>, weight_stats_wide_kernel<0, 1>);
      else if (mode == 1) go(weight_stats_kernel<1, WSTATS_EB>, weight_stats_wide_kernel<1, WSTATS_EB>);
      else go(weight_stats_kernel<8, WSTATS_EB>, weight_stats_wide_kernel<8, WSTATS_EB>);
    }
    rt::d2h(acc.data(), d_acc, acc.size() * 8, s->stream);
    rt::stream_sync(s->stream);
  } catch (...) {
    rt::dfree(d_acc);
    throw;
  }
  rt::dfree(d_acc);
  if ((uint32_t)acc[2 * c.W]) return DWX_E_LIMIT;
  for (uint64_t w = 0; w < c.W; ++w) {
    const __int128 total = (__int128)(long long)acc[2 * w] * ((__int128)1 << 32) + (__int128)acc[2 * w + 1];
    out[w] = (double)total * (1.0 / 4294967296.0);
  }
  return DWX_OK;
}

int weight_stats_error(const dwx_sampler *s, int rc, uint64_t limit_wid) {
  if (rc == DWX_E_NOMEM)
    return fail(rc, "no device memory for the factor table (dwx_graph_info: factor_table_bytes) or the sums of the call (16 bytes per weight)");
  if (limit_wid < s->cg->W)
    return fail(rc, "weight " + std::to_string(limit_wid) + " has " + std::to_string(s->wstats_max_count) +
                        " factors: entries x factors reaches 2^32 terms, beyond the exact sums (split the entry range)");
  return fail(rc, "a term sign * feature value is not finite or reaches 2^30: outside the sums' domain");
}
}  // namespace

int dwx_weight_stats(dwx_sampler *s, int chain, double *stats) {
  if (!s || !stats) return fail(DWX_E_INVALID, "null argument");
  if (!s->cg->keep_factors) return fail(DWX_E_INVALID, "the graph was compiled without dwx_compile_opts.keep_factors");
  if (chain != 0 && chain != 1) return fail(DWX_E_INVALID, "chain must be 0 (free) or 1 (evidence)");
  std::vector<double> v;
  int code = DWX_OK;
  uint64_t limit_wid = 0;
  int rc = guarded([&]() {
    v.resize(s->cg->W);
    rt::set_device(s->device);
    flush_pending(s, chain == 0 ? 1 : 2);
    code = run_weight_stats(s, 0, chain == 0 ? s->d_assign_free : s->d_assign_evid, 0u, 1, v.data(), &limit_wid);
  });
  if (rc != DWX_OK) return rc;
  if (code != DWX_OK) return weight_stats_error(s, code, limit_wid);
  std::copy(v.begin(), v.end(), stats);
  return DWX_OK;
}

int dwx_trace_weight_stats(dwx_sampler *s, uint64_t first_entry, uint64_t n_entries, double *sums) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  const CompiledGraph &c = *s->cg;
  if (!c.keep_factors) return fail(DWX_E_INVALID, "the graph was compiled without dwx_compile_opts.keep_factors");
  if (!sums) return fail(DWX_E_INVALID, "null argument");
  if (!s->d_trace) return fail(DWX_E_INVALID, "the sample trace was never enabled (dwx_trace_enable)");
  if (c.Vo != c.V) return fail(DWX_E_INVALID, "ghost variables are not traced: a shard's trace holds no joint state to evaluate");
  if (first_entry > s->trace_count || n_entries > s->trace_count - first_entry)
    return fail(DWX_E_INVALID, "entries outside the sample trace (dwx_trace_info: count)");
  std::vector<double> v;
  int code = DWX_OK;
  uint64_t limit_wid = 0;
  int rc = guarded([&]() {
    v.resize(c.W);
    rt::set_device(s->device);
    const uint32_t slot0 = (uint32_t)(((uint64_t)s->trace_next + s->trace_cap - s->trace_count + first_entry) % s->trace_cap);
    code = run_weight_stats(s, (int)s->trace_bits, s->d_trace, slot0, n_entries, v.data(), &limit_wid);
  });
  if (rc != DWX_OK) return rc;
  if (code != DWX_OK) return weight_stats_error(s, code, limit_wid);
  std::copy(v.begin(), v.end(), sums);
  return DWX_OK;
}

int dwx_get_tallies(dwx_sampler *s, uint64_t *tallies, uint64_t *nsamples) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    const CompiledGraph &c = *s->cg;
    rt::set_device(s->device);
    if (tallies) {
      RawArray<uint32_t> t(c.R);
      rt::d2h(t.data(), s->d_tally, c.R * 4, s->stream);
      rt::stream_sync(s->stream);
      parallel_ranges(c.Vo, host_threads(), [&](uint64_t pb, uint64_t pe) {
        for (uint64_t p = pb; p < pe; ++p) {
          const uint64_t rb = c.ref_var_val_base[c.perm[p]];
          for (uint32_t r = c.v_row[p]; r < c.v_row[p + 1]; ++r) tallies[rb + (r - c.v_row[p])] = t[r];
        }
      });
    }
    if (nsamples)  // agg_nsamples: +1 per inference sweep for every sampled variable
      parallel_ranges(c.V, host_threads(), [&](uint64_t vb, uint64_t ve) {
        for (uint64_t v = vb; v < ve; ++v)
          nsamples[v] = (v < c.Vo && (!c.var_is_evid[v] || s->opts.sample_evidence)) ? s->infer_sweeps : 0;
      });
  });
}

int dwx_get_assignments(dwx_sampler *s, int chain, uint64_t *out) {
  if (!s || !out) return fail(DWX_E_INVALID, "null argument");
  return guarded([&]() {
    const CompiledGraph &c = *s->cg;
    rt::set_device(s->device);
    flush_pending(s, chain == 0 ? 1 : 2);
    std::vector<uint32_t> a(c.V);
    rt::d2h(a.data(), chain == 0 ? s->d_assign_free : s->d_assign_evid, c.V * 4, s->stream);
    rt::stream_sync(s->stream);
    for (uint64_t p = 0; p < c.V; ++p) out[c.perm[p]] = a[p];
  });
}

int dwx_set_assignments(dwx_sampler *s, int chain, const uint64_t *in) {
  if (!s || !in) return fail(DWX_E_INVALID, "null argument");
  return guarded([&]() {
    const CompiledGraph &c = *s->cg;
    rt::set_device(s->device);
    flush_pending(s);   // (owed draws must not land on top of the caller's values)
    std::vector<uint32_t> a(c.V);
    for (uint64_t p = 0; p < c.V; ++p) a[p] = (uint32_t)in[c.perm[p]];
    rt::h2d(chain == 0 ? s->d_assign_free : s->d_assign_evid, a.data(), c.V * 4, s->stream);
    rt::stream_sync(s->stream);
  });
}

int dwx_get_sweep(dwx_sampler *s, uint64_t *out) {
  if (!s || !out) return fail(DWX_E_INVALID, "null argument");
  *out = s->sweep;
  return DWX_OK;
}

int dwx_set_sweep(dwx_sampler *s, uint64_t sweep) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  // (owed draws carry their own counter; flushed all the same, so that a counter set back meets no older record)
  return guarded([&]() {
    flush_pending(s);
    s->sweep = sweep;
  });
}

int dwx_device_buffer(dwx_sampler *s, int which, void **dev_ptr, uint64_t *nbytes) {
  if (!s || !dev_ptr || !nbytes) return fail(DWX_E_INVALID, "null argument");
  const CompiledGraph &c = *s->cg;
  if (which == DWX_BUF_ASSIGN_FREE || which == DWX_BUF_ASSIGN_EVID) {
    // the caller keeps the pointer and reads or writes behind the library's back: what is owed is drawn now, and
    // no learning sweep of this sampler defers again (an un-split level then wants the layout it went without)
    int rc = guarded([&]() {
      flush_pending(s);
      if (!s->defer_ok) return;
      s->defer_ok = false;
      auto it = s->levels.find(1);
      if (it != s->levels.end() && s->opts.plan_layouts == 0 && (build_on_device() || it->second->sweeps >= layout_after_sweeps()))
        ensure_level_layout(s, it->second.get(), 1);
    });
    if (rc != DWX_OK) return rc;
  }
  switch (which) {
    case DWX_BUF_WEIGHTS: *dev_ptr = s->d_weights; *nbytes = c.W * 8; break;
    case DWX_BUF_GRAD: *dev_ptr = s->d_grad; *nbytes = c.W * 16; break;
    case DWX_BUF_ASSIGN_FREE: *dev_ptr = s->d_assign_free; *nbytes = c.V * 4; break;
    case DWX_BUF_ASSIGN_EVID: *dev_ptr = s->d_assign_evid; *nbytes = c.V * 4; break;
    case DWX_BUF_TALLIES: *dev_ptr = s->d_tally; *nbytes = c.R * 4; break;
    case DWX_BUF_RB: *dev_ptr = s->d_rb; *nbytes = s->d_rb ? c.R * 8 : 0; break;
    case DWX_BUF_TRACE: *dev_ptr = s->d_trace; *nbytes = s->d_trace ? (uint64_t)s->trace_cap * s->trace_words * 8 : 0; break;
    case DWX_BUF_TSTATIC: {
      auto it = s->levels.find(1);
      *dev_ptr = it == s->levels.end() ? nullptr : it->second->d_t_static;
      *nbytes = *dev_ptr ? c.W * 16 : 0;   // (none: the un-split sweep is outside the learning domain)
      break;
    }
    case DWX_BUF_TSTATIC_PLAN:
      if (!s->plan_valid || !s->plan_level) return fail(DWX_E_INVALID, "no plan: call dwx_sgd_plan first");
      {
        const bool tables = s->plan_level->fast && !(s->plan_batches > 1 && s->plan_force_dynamic);
        *dev_ptr = tables ? s->plan_level->d_t_static : nullptr;
        *nbytes = tables ? (uint64_t)s->plan_level->rows * c.W * 16 : 0;
      }
      break;
    case DWX_BUF_SORTED_RECORDS:     // (test hook: the device-built copy against the host builder's)
      *dev_ptr = s->d_sorted; *nbytes = s->d_sorted ? c.n_sorted * sizeof(SortRec8) : 0;
      break;
    case DWX_BUF_SORTED_RECORDS_PLAN:
      if (!s->plan_level) return fail(DWX_E_INVALID, "no plan: call dwx_sgd_plan first");
      *dev_ptr = s->plan_level->d_sorted;
      {
        uint64_t n = 0;
        for (const SuperTile &st : s->plan_level->sorted_supers) n += st.nrec;
        *nbytes = s->plan_level->d_sorted ? n * sizeof(SortRec8) : 0;
      }
      break;
    default: return fail(DWX_E_INVALID, "unknown buffer id");
  }
  return DWX_OK;
}

int dwx_halo_create(dwx_sampler *s, const uint64_t *vids, uint64_t n, dwx_halo **out) {
  if (!s || !out || (n && !vids)) return fail(DWX_E_INVALID, "null argument");
  if (n >= 0xFFFFFFFFull) return fail(DWX_E_LIMIT, "halo list exceeds 2^32-1 entries");
  std::unique_ptr<dwx_halo> h(new dwx_halo());
  int rc = guarded([&]() {
    const CompiledGraph &c = *s->cg;
    rt::set_device(s->device);
    std::vector<uint32_t> pos(n);
    uint32_t max_card = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (vids[i] >= c.V) throw std::invalid_argument("halo list: variable id out of range");
      pos[i] = c.pos[vids[i]];
      max_card = std::max(max_card, c.v_meta[pos[i]] >> VM_CARD_SHIFT);
    }
    h->s = s; h->n = (uint32_t)n;
    // (both ends list the same variables, so they choose the same width)
    h->bits = max_card <= 2 ? 1u : (max_card <= 256 ? 8u : 32u);
    h->block = (uint32_t)(((uint64_t)n * h->bits + 63) / 64);
    h->d_pos = upload(pos, s->stream);
    const size_t bytes = std::max<size_t>((size_t)2 * h->block * 8, 8);
    h->d_buf = (unsigned long long *)rt::dmalloc(bytes);
    rt::dmemset(h->d_buf, 0, bytes, s->stream);
    rt::stream_sync(s->stream);
  });
  if (rc != DWX_OK) return rc;
  *out = h.release();
  return DWX_OK;
}

void dwx_halo_destroy(dwx_halo *h) { delete h; }

int dwx_halo_buffer(dwx_halo *h, void **dev_ptr, uint64_t *nbytes) {
  if (!h || !dev_ptr || !nbytes) return fail(DWX_E_INVALID, "null argument");
  *dev_ptr = h->d_buf;
  *nbytes = (uint64_t)2 * h->block * 8;
  return DWX_OK;
}

int dwx_halo_message_bytes(dwx_halo *h, int chains, uint64_t *nbytes) {
  if (!h || !nbytes) return fail(DWX_E_INVALID, "null argument");
  if (chains < 1 || chains > 3) return fail(DWX_E_INVALID, "chains: bit 0 = free chain, bit 1 = evidence chain");
  *nbytes = (uint64_t)(chains == 3 ? 2 : 1) * h->block * 8;
  return DWX_OK;
}

namespace {
int halo_move(dwx_halo *h, int chains, bool pack) {
  if (!h) return fail(DWX_E_INVALID, "null halo list");
  if (chains < 1 || chains > 3) return fail(DWX_E_INVALID, "chains: bit 0 = free chain, bit 1 = evidence chain");
  if (!h->n) return DWX_OK;
  return guarded([&]() {
    dwx_sampler *s = h->s;
    rt::set_device(s->device);
    flush_pending(s);   // (packing reads the chains; owed draws must not land on top of unpacked values)
    const unsigned grid = std::min<unsigned>((h->n + BLOCK_THREADS - 1) / BLOCK_THREADS, 4096u);
    auto go = [&](auto pk, auto unpk) {
      if (pack)
        rt::launch(pk, grid, BLOCK_THREADS, 0, s->stream, (const uint32_t *)h->d_pos, h->n,
                   (const uint32_t *)s->d_assign_free, (const uint32_t *)s->d_assign_evid, (uint32_t)chains,
                   h->d_buf, h->block);
      else
        rt::launch(unpk, grid, BLOCK_THREADS, 0, s->stream, (const uint32_t *)h->d_pos, h->n,
                   s->d_assign_free, s->d_assign_evid, (uint32_t)chains, (const unsigned long long *)h->d_buf, h->block);
    };
    if (h->bits == 1) go(halo_pack_kernel<1>, halo_unpack_kernel<1>);
    else if (h->bits == 8) go(halo_pack_kernel<8>, halo_unpack_kernel<8>);
    else go(halo_pack_kernel<32>, halo_unpack_kernel<32>);
  });
}
}  // namespace

int dwx_halo_pack_async(dwx_halo *h, int chains) { return halo_move(h, chains, true); }
int dwx_halo_unpack_async(dwx_halo *h, int chains) { return halo_move(h, chains, false); }

int dwx_stream(dwx_sampler *s, void **stream) {
  if (!s || !stream) return fail(DWX_E_INVALID, "null argument");
  *stream = (void *)s->stream;
  return DWX_OK;
}

int dwx_kernel_time_reset(dwx_sampler *s, int enable) {
  if (!s) return fail(DWX_E_INVALID, "null sampler");
  return guarded([&]() {
    rt::set_device(s->device);
    drain_spans(s);
    for (int k = 0; k < 4; ++k) { s->t_ms[k] = 0; s->t_launches[k] = 0; s->t_sweeps[k] = 0; }
    s->timing = enable != 0;
  });
}

int dwx_kernel_time(dwx_sampler *s, int kind, double *ms, uint64_t *launches, uint64_t *sweeps) {
  if (!s || kind < 0 || kind > 7) return fail(DWX_E_INVALID, "bad argument");
  if (kind == 7) {   // deferred draws: device time of the flushes since the last reset; flushes and deferring sweeps since create
    return guarded([&]() {
      rt::set_device(s->device);
      drain_spans(s);
      if (ms) *ms = s->t_ms[3];
      if (launches) *launches = s->flushes;
      if (sweeps) *sweeps = s->deferred_sweeps;
    });
  }
  if (kind == 6) {   // learning sweeps (and their super-tiles) that took sums from the potential cache
    if (ms) *ms = 0.0;
    if (launches) *launches = s->pot_supers;
    if (sweeps) *sweeps = s->pot_sweeps;
    return DWX_OK;
  }
  if (kind == 5) {   // split learning sweeps run with one (merged) launch per mini-batch since the sampler was created
    if (ms) *ms = 0.0;
    if (launches) *launches = s->merged_sweeps;
    if (sweeps) *sweeps = s->merged_sweeps;
    return DWX_OK;
  }
  if (kind == 4) {   // split learning sweeps run as ONE persistent launch since the sampler was created (no device time)
    if (ms) *ms = 0.0;
    if (launches) *launches = s->persist_launches;
    if (sweeps) *sweeps = s->persist_launches;
    return DWX_OK;
  }
  if (kind == 3) {   // graph replays of split learning sweeps since the sampler was created (no device time)
    if (ms) *ms = 0.0;
    if (launches) *launches = s->graph_launches;
    if (sweeps) *sweeps = s->graph_launches;
    return DWX_OK;
  }
  return guarded([&]() {
    rt::set_device(s->device);
    drain_spans(s);
    if (ms) *ms = s->t_ms[kind];
    if (launches) *launches = s->t_launches[kind];
    if (sweeps) *sweeps = s->t_sweeps[kind];
  });
}

int dwx_test_philox(int device, const uint32_t key[2], const uint32_t ctr[4], uint32_t out[4], double uniforms[2]) {
  if (!key || !ctr || !out || !uniforms) return fail(DWX_E_INVALID, "null argument");
  return guarded([&]() {
    rt::init_device(device);
    rt::stream_t st = rt::stream_create();
    uint32_t *dout = (uint32_t *)rt::dmalloc(8 * 4);
    double *duni = (double *)rt::dmalloc(16);
    rt::h2d(dout + 4, ctr, 16, st);     // (the counter again, for the uniforms' entry point)
    rt::launch(test_philox_kernel, 1, 64, 0, st, key[0], key[1], ctr[0], ctr[1], ctr[2], ctr[3], dout, duni);
    rt::d2h(out, dout, 16, st);
    rt::d2h(uniforms, duni, 16, st);
    rt::stream_sync(st);
    rt::dfree(dout); rt::dfree(duni);
    rt::stream_destroy(st);
  });
}

int dwx_test_wave_ops(int device, int op, const uint64_t *in, uint64_t n, uint64_t *out) {
  if (!in || !out || n == 0) return fail(DWX_E_INVALID, "null argument");
  uint64_t n_rec = 0, first = 0, head = 0, rec_words = 0, n_out = BLOCK_THREADS;
  switch (op) {
    case DWX_WAVE_OP_SEG_SUM: if (n != 2 * BLOCK_THREADS) return fail(DWX_E_INVALID, "dwx_test_wave_ops: 512 input words"); n_out = 2 * BLOCK_THREADS; break;
    case DWX_WAVE_OP_SUM_F64: case DWX_WAVE_OP_BALLOT: case DWX_WAVE_OP_PAIR_SWAP:
      if (n != BLOCK_THREADS) return fail(DWX_E_INVALID, "dwx_test_wave_ops: 256 input words");
      break;
    case DWX_WAVE_OP_LOAD16: head = 1; rec_words = 2; n_out = (uint64_t)WAVE_OP_LOAD_K * BLOCK_THREADS * 2; break;
    case DWX_WAVE_OP_LOAD8: head = 1; rec_words = 1; n_out = (uint64_t)WAVE_OP_LOAD_K * BLOCK_THREADS; break;
    case DWX_WAVE_OP_LOAD_SORTED: head = 2; rec_words = 1; n_out = (uint64_t)WAVE_OP_SORT_K * BLOCK_THREADS; break;
    default: return fail(DWX_E_INVALID, "dwx_test_wave_ops: unknown op");
  }
  if (head) {
    if (n < head) return fail(DWX_E_INVALID, "dwx_test_wave_ops: input too short");
    n_rec = in[0];
    first = head == 2 ? in[1] : 0;
    if (n_rec > (1u << 20) || first > (1u << 20) || n != head + n_rec * rec_words)
      return fail(DWX_E_INVALID, "dwx_test_wave_ops: the input does not hold n_rec records");
  }
  return guarded([&]() {
    rt::init_device(device);
    rt::stream_t st = rt::stream_create();
    // the records in an allocation of exactly their size: a load past the end would leave it
    const size_t rec_bytes = (size_t)(n_rec * rec_words * 8), in_bytes = (size_t)((head ? head : n) * 8);
    unsigned long long *din = (unsigned long long *)rt::dmalloc(in_bytes);
    void *drec = rt::dmalloc(rec_bytes ? rec_bytes : 16);
    unsigned long long *dout = (unsigned long long *)rt::dmalloc(n_out * 8);
    rt::h2d(din, in, in_bytes, st);
    if (rec_bytes) rt::h2d(drec, in + head, rec_bytes, st);
    rt::dmemset(dout, 0xEE, n_out * 8, st);
    rt::launch(test_wave_ops_kernel, 1, BLOCK_THREADS, 0, st, (uint32_t)op, (const unsigned long long *)din,
               (const void *)drec, (uint32_t)n_rec, (uint32_t)first, dout);
    rt::d2h(out, dout, n_out * 8, st);
    rt::stream_sync(st);
    rt::dfree(din); rt::dfree(drec); rt::dfree(dout);
    rt::stream_destroy(st);
  });
}

int dwx_test_factor_sign(int device, int func, uint64_t arity, const uint8_t *sat, double *out) {
  if (!sat || !out || arity == 0 || arity > 4096) return fail(DWX_E_INVALID, "bad argument");
  return guarded([&]() {
    rt::init_device(device);
    rt::stream_t st = rt::stream_create();
    std::vector<VifRec> vifs(arity);
    std::vector<uint32_t> assign(arity);
    for (uint64_t i = 0; i < arity; ++i) { vifs[i] = VifRec{(uint32_t)i, 1u}; assign[i] = sat[i]; }
    VifRec *dv = upload(vifs, st);
    uint32_t *da = upload(assign, st);
    double *dout = (double *)rt::dmalloc(8);
    rt::launch(test_sign_kernel, 1, 64, 0, st, (uint32_t)func, (uint32_t)arity,
               (const VifRec *)dv, (const uint32_t *)da, dout);
    rt::d2h(out, dout, 8, st);
    rt::stream_sync(st);
    rt::dfree(dv); rt::dfree(da); rt::dfree(dout);
    rt::stream_destroy(st);
  });
}

}  // extern "C"
