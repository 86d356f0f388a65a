/*
 * dwx.h -- C ABI of the MI355X-native DimmWitted Gibbs sweep ("dwx").
 *
 * This is the drop-in boundary for the reference's ONE hot path: the seam between
 * the epoch driver (DimmWitted::learn / inference, /root/reference/src/dimmwitted.cc:
 * 121-207) and the per-replica sampler (class GibbsSampler,
 * /root/reference/src/gibbs_sampler.h:18-57).  The reference has no FFI of its own;
 * every entry point below names the internal C++ interface it replaces.  Plain
 * pointers and sizes only -- no C++ or torch types cross this boundary.
 *
 * Conventions: every function returns 0 on success and a negative DWX_E_* code on
 * error (dwx_last_error() gives the text; the reference assert()s/abort()s in the
 * same situations).  Handles are opaque.  Host arrays passed in are copied during
 * the call; the library owns all device memory until *_destroy.  One host thread
 * drives one sampler handle; *_async calls enqueue on the handle's HIP stream and
 * dwx_wait() is the barrier, exactly like GibbsSampler::sample()/wait().
 *
 * There is NO CPU fallback: dwx_sampler_create fails with DWX_E_DEVICE when no HIP
 * device is usable.  dwx_graph_* functions are host-only (graph compilation) and
 * work without a GPU.
 */
#ifndef DWX_H_
#define DWX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWX_VERSION 1

enum {
  DWX_OK = 0,
  DWX_E_INVALID = -1,  /* malformed graph / argument (reference: assert/abort)   */
  DWX_E_LIMIT = -2,    /* graph exceeds the compact 32-bit layout / a numeric domain */
  DWX_E_DEVICE = -3,   /* HIP error or no device                                */
  DWX_E_NOMEM = -4
};

/* Columnar image of the reference's binary input files
 * (/root/reference/doc/binary_format.md; loaders src/binary_format.cc:48-226).
 * Ids must be dense (0..N-1), as FactorGraph::safety_check demands
 * (src/factor_graph.cc:201-219). */
typedef struct dwx_graph_desc {
  uint64_t num_variables, num_factors, num_edges, num_weights;
  const uint8_t *var_role;         /* isEvidence byte; evidence iff >= 1          */
  const uint64_t *var_init_value;  /* initialValue as in the file                 */
  const uint16_t *var_dtype;       /* 0 boolean, 1 categorical                    */
  const uint64_t *var_cardinality;
  uint64_t num_domains;            /* categorical domain blocks (may be 0)        */
  const uint64_t *dom_vid;         /* [num_domains]                               */
  const uint64_t *dom_offset;      /* [num_domains+1] into dom_value/truthiness   */
  const uint64_t *dom_value;
  const double *dom_truthiness;
  const uint16_t *fac_func;        /* FACTOR_FUNCTION_TYPE (src/common.h:35-48)   */
  const uint64_t *fac_edge_offset; /* [num_factors+1]; a factor holds at most 65535 variable
                                      positions (its arity, duplicates counted; the 16-bit field
                                      of an edge record) -- DWX_E_LIMIT beyond                */
  const uint64_t *fac_weight_id;
  const double *fac_feature_value; /* finite; |value| <= 65536 on a learnable weight (DWX_E_LIMIT
                                      beyond: gradients are summed in 2^-30 fixed point, int64 --
                                      and the sums of one mini-batch must fit: dwx_sgd_plan);
                                      |value| below ~5e-10 contributes no gradient            */
  const uint64_t *edge_vid;
  const uint64_t *edge_equal_to;   /* equalPredicate as in the file               */
  const double *w_initial_value;   /* indexed by weight id                        */
  const uint8_t *w_is_fixed;
  /* Sharding: the LAST num_ghost_variables variables are ghosts -- remote variables
   * that local factors read.  They hold an assignment (refreshed by the caller's halo
   * exchange) but are never sampled, tallied or given rows.  0 for a whole graph. */
  uint64_t num_ghost_variables;
} dwx_graph_desc;

/* Graph-compilation knobs; zero-initialise for defaults. */
typedef struct dwx_compile_opts {
  uint32_t tile_vars;          /* variables per workgroup tile (default 256, max 256)  */
  uint32_t tile_edges;         /* edge records staged in LDS per tile (default 3072)   */
  uint32_t tile_rows;          /* value rows per tile (default 256 bool / 1536 categ.) */
  uint32_t conflict_arity_cap; /* factors wider than this do not constrain the
                                  colouring (Hogwild reads, as in the reference);
                                  default 256, at most 65535 (the arity limit).  Over a
                                  wider factor an INFERENCE sweep is still a sequential
                                  scan where all but one of the factor's variables are
                                  evidence (and evidence is not sampled); a LEARNING sweep
                                  is Hogwild on the free chain even then: the free chain
                                  draws evidence variables too                          */
  uint32_t n_threads;          /* host threads for the build (0 = DWX_HOST_THREADS, else the hardware
                                  concurrency capped at 64 and at twice the cgroup's CPU quota)  */
  uint32_t no_compact_records; /* 1: keep 16-byte records even for all-unary graphs
                                  (default 0: such graphs stream 8-byte records)       */
  uint32_t no_weight_order;    /* 1: keep variables in id order inside a class (default 0: an
                                  all-unary graph orders them by the weight id of their first
                                  factor -- locality for the weight gathers)              */
  uint32_t wide_min_records;   /* degree binning: a variable with more edge records than this
                                  is walked by a whole wave instead of one lane (default 192;
                                  0xFFFFFFFF: never)                                   */
  uint32_t no_record_vifs;     /* 1: factors of arity 2-3 keep their factor->variable entries once
                                  per factor (default 0: once per edge record, in record order,
                                  streamed by the staging pass -- 2-3x the entries; chosen
                                  automatically when the copies would not fit 32-bit bases) */
  uint32_t no_pull_unary;      /* 1: tiles with non-unary factors scatter the gradient of all their
                                  records (default 0: their unary records take the pull gradient
                                  of all-unary tiles when the graph has more than 1024 weights) */
  uint32_t no_sorted_records;  /* 1: no weight-sorted second copy of the records of boolean all-unary
                                  tiles (default 0: compact-record graphs with >= 4096 weights get
                                  one, and their sweeps gather weights in sorted order)        */
  uint32_t super_tiles;        /* tiles per weight-sorted super-tile, at most (default 75 to 79 = 19 200 to
                                  20 224 variables: the fixed-point sums that fit the CU's 160 KiB of LDS
                                  beside the graph's table of distinct record values; more tiles than
                                  that only where tiles are smaller than 256 variables)                  */
  uint32_t sorted_slots;       /* workgroups of sorted_sweep_kernel resident at once (default 256: one
                                  1024-thread workgroup per CU of an MI355X); runs of tiles are cut into
                                  multiples of it                                                       */
  uint32_t defer_sorted_records; /* set by dwx_graph_create itself where the library can build on the device
                                  (always in the product; DWX_HOST_BUILD=1 in the environment keeps the host
                                  builder): the weight-sorted copy is only PLANNED here and every sampler
                                  builds its records on its own device (device_build.hip)               */
  uint32_t no_narrow_info;     /* 1: do not scan the records for dwx_graph_info.grad_shift / grad_unit_max /
                                  max_records_per_weight (they read 0: "nothing is known, send int64") -- a
                                  pass over every record with a histogram per weight that only multi-GPU
                                  drivers need; `dw gibbs` on one GPU sets it (2 s at config 5's size)      */
  uint32_t keep_factors;       /* 1: also keep a factor-major table (16 bytes per factor, 8 per edge of a factor
                                  of arity >= 2, 8 more per factor where a feature value is no exact f32;
                                  dwx_graph_info.factor_table_bytes) -- what dwx_score / dwx_trace_score read.
                                  Changes nothing else the compiler produces.  Default 0: nothing is kept    */
} dwx_compile_opts;

typedef struct dwx_graph_info {
  uint64_t num_variables, num_factors, num_edges, num_weights;
  uint64_t num_owned_variables; /* num_variables - ghosts: the variables this graph samples */
  uint64_t num_values;         /* value rows: 1 per boolean, cardinality per categorical
                                  (== FactorGraph size.num_values)                     */
  uint64_t num_index_entries;  /* |factor_index| after dedup (src/factor_graph.cc:177) */
  uint64_t num_vif_entries;    /* factor->variable entries kept for arity >= 2         */
  uint64_t num_colors, num_launches, num_tiles, num_giant_tiles;   /* giant: workgroup-per-variable */
  uint64_t max_cardinality;
  uint64_t num_query_variables; /* non-evidence variables (sampled by an inference sweep
                                   unless --sample_evidence)                            */
  uint64_t device_bytes;       /* bytes the sampler will hold in HBM                   */
  uint32_t has_categorical, order_is_identity;
  uint64_t num_wide_tiles;     /* variables walked by a wave each (degree bin, see
                                  dwx_compile_opts.wide_min_records)                   */
  uint64_t num_staged_tiles;   /* tiles whose non-unary factors (arity <= 3) are evaluated
                                  edge-parallel while the tile is staged  */
  uint64_t num_super_tiles;    /* weight-sorted super-tiles (sorted_sweep_kernel) and the records of */
  uint64_t num_sorted_records; /* their sorted second copy; 0: no sorted copy             */
  /* Multi-GPU drivers: on an all-boolean all-unary graph every contribution to DWX_BUF_GRAD's
   * gradient sums is a multiple of 2^grad_shift (fixed point 2^-30), at most grad_unit_max such
   * units, and no weight has more than max_records_per_weight records -- so the sums may travel as
   * 32-bit counts (G >> grad_shift) while ranks x max_records_per_weight x grad_unit_max < 2^31.
   * grad_shift == 0: nothing is known (categorical variables, non-unary factors): send int64. */
  uint64_t grad_shift, grad_unit_max, max_records_per_weight;
  uint64_t max_super_tile_variables; /* variables of the largest weight-sorted super-tile (0: no sorted copy) */
  uint64_t factor_table_bytes; /* the factor-major table of dwx_compile_opts.keep_factors (0 without): host bytes,
                                  and device bytes once dwx_score / dwx_trace_score has run; NOT in device_bytes */
} dwx_graph_info;

/* Runtime options of one sampler (the CmdParser fields the hot path reads:
 * src/gibbs_sampler.cc:46-48, src/inference_result.h:66-85). */
typedef struct dwx_options {
  int32_t device;              /* HIP device ordinal                                   */
  int32_t sample_evidence;     /* --sample_evidence                                    */
  int32_t learn_non_evidence;  /* --learn_non_evidence                                 */
  int32_t noise_aware;         /* --noise_aware                                        */
  int32_t regularization;      /* 0 = l1, 1 = l2 (reference enum order)                */
  int32_t plan_layouts;        /* weight-sorted layouts of the LEARNING sweeps' own (cut along a
                                  split plan's mini-batches, or -- un-split -- over whole launches
                                  instead of their query / evidence parts: a few % per sweep for
                                  a second copy of the records each):
                                  0 = default: built with the plan level (the records are sorted on the
                                  device in milliseconds; a DWX_HOST_BUILD=1 run builds them on the host
                                  -- 0.3 s per level -- once the level has run 2048 sweeps),
                                  1 = always with the level, 2 = never                      */
  double reg_param;            /* -b / --reg_param                                     */
  double step_cap;             /* bound on stepsize x R of one SGD mini-batch (see
                                  dwx_sgd_plan); <= 0: never split a sweep; default 1.5
                                  (dwx_default_options)                                 */
  uint64_t seed;               /* Philox key                                           */
  uint64_t var_id_offset;      /* added to local variable ids in the Philox counter: the
                                  global id of this shard's variable 0 (multi-GPU)     */
} dwx_options;

typedef struct dwx_graph dwx_graph;
typedef struct dwx_sampler dwx_sampler;

const char *dwx_last_error(void);
int dwx_version(void);
void dwx_default_options(dwx_options *o);

/* ---- graph compilation (host only) --------------------------------------------
 * Replaces FactorGraph::load_* conversions + construct_index
 * (src/binary_format.cc:128-226, src/factor_graph.cc:90-199) and adds what the
 * device needs: chromatic partition, colour-major variable order, LDS tiles. */
int dwx_graph_create(const dwx_graph_desc *desc, const dwx_compile_opts *opts, dwx_graph **out);
void dwx_graph_destroy(dwx_graph *g);
int dwx_graph_get_info(const dwx_graph *g, dwx_graph_info *out);
/* Execution schedule: order[num_owned_variables] = original variable ids in device order;
 * launch_off[num_launches+1] = offsets into order; every launch is an independent
 * set of the variable conflict graph. */
int dwx_graph_get_schedule(const dwx_graph *g, uint64_t *order, uint64_t *launch_off);
/* mask[num_variables] (reference numbering): 1 where the device sums the variable's potentials
 * in fixed point (2^-32; boolean variables of an all-unary graph on the lane path -- the sums
 * are then independent of the order of the records, which the weight-sorted sweep relies on),
 * 0 where it adds f64 terms in the reference's row order (src/factor_graph.h:127-145).  Test
 * hook: the CPU oracle's schedule mode follows it, so device-vs-oracle parity stays exact. */
int dwx_graph_get_fixed_point_mask(const dwx_graph *g, uint8_t *mask);
/* Value table for result dumps (src/inference_result.cc:211-243):
 * var_val_base[V] (reference numbering) and value_sparse[num_values]. */
int dwx_graph_get_values(const dwx_graph *g, uint64_t *var_val_base, uint64_t *value_sparse);
/* Device positions of variables (index into DWX_BUF_ASSIGN_*), for halo exchange:
 * out[i] = position of original variable id vids[i]. */
int dwx_graph_get_positions(const dwx_graph *g, const uint64_t *vids, uint64_t n, uint64_t *out);
/* Reference-order CSR, for parity checks against construct_index:
 * index_base/index_len[num_values], factor_index[num_index_entries]. */
int dwx_graph_get_index(const dwx_graph *g, uint64_t *index_base, uint64_t *index_len,
                        uint64_t *factor_index);
/* Test hook: the compiled workgroup tiles, in device order (tile i of launch l: the launches' tiles follow each
 * other).  flags are the TILE_* bits of sampler_amd/csrc/device_types.h as the compiler set them (bit 0 SIMPLE,
 * 1 CATEGORICAL, 2 PULL, 3 TERMS2, 4 INLINE2, 5 GIANT, 6 WIDE, 7 TERMS3, 8 PULL_UNARY, 9 UNIT_ROWS); v0 / nv the
 * tile's variables as device positions [v0, v0 + nv), nrows its value rows, nedges its edge records.  out[n] with
 * n == dwx_graph_info.num_tiles (DWX_E_INVALID otherwise).  Host only: no device call. */
typedef struct dwx_tile_info {
  uint32_t flags, v0, nv, nrows, nedges;
} dwx_tile_info;
int dwx_graph_get_tiles(const dwx_graph *g, uint64_t n, dwx_tile_info *out);

/* ---- sampler (device) -----------------------------------------------------------
 * Replaces GibbsSampler(pfg, weights, numa_nodes, nthread, nodeid, opts)
 * (src/gibbs_sampler.cc:5-18) incl. the InferenceResult it owns
 * (src/inference_result.cc:24-42). */
int dwx_sampler_create(const dwx_graph *g, const dwx_options *opts, dwx_sampler **out);
/* Optional: pay the HIP runtime's start-up (context creation on `device`) now -- e.g. on a
 * helper thread while dwx_graph_create, which is host-only, runs.  dwx_sampler_create does
 * the same on its own if this was never called.  (No reference counterpart: the reference
 * has no device.) */
int dwx_device_init(int32_t device);
/* Number of usable HIP devices (0 without a GPU: not an error). */
int dwx_device_count(int32_t *count);
/* Frees the sampler's device buffers and hands the device builds' idle scratch blocks (sort buffers
 * kept in a cache inside the library: INTEGRATION.md, "Device memory a caller may notice") back to the runtime. */
void dwx_sampler_destroy(dwx_sampler *s);

/* GibbsSampler::sample(i_epoch) (src/gibbs_sampler.cc:20-25): one inference sweep. */
int dwx_sample_async(dwx_sampler *s);
/* The inference loop of DimmWitted::inference (src/dimmwitted.cc:131-156: `for i_epoch:
 * sample(i_epoch); wait()`), n_sweeps of its iterations in one call: state, tallies and sweep
 * counter afterwards are bit for bit those of n_sweeps calls of dwx_sample_async.  On a graph
 * whose factors are all unary (no variable reads another, so nothing a sweep reads changes
 * between sweeps) the sweeps share ONE launch: every record is read once, every variable draws
 * n_sweeps times with the uniforms its separate sweeps would have used.  Any other graph runs
 * the n_sweeps sweeps one after the other. */
int dwx_sample_n_async(dwx_sampler *s, uint32_t n_sweeps);
/* GibbsSampler::sample_sgd(stepsize) (src/gibbs_sampler.cc:27-33): one learning
 * sweep = dwx_sgd_plan + (accumulate, apply)* + dwx_sgd_finish. */
int dwx_sample_sgd_async(dwx_sampler *s, double stepsize);
/* GibbsSampler::wait() (src/gibbs_sampler.cc:35-38). */
int dwx_wait(dwx_sampler *s);

/* A learning sweep in pieces, for drivers that put a collective between accumulation and
 * update (multi-GPU: all-reduce DWX_BUF_GRAD; replaces the dormant
 * InferenceResult::merge_gradients_from, src/inference_result.cc:57-62).
 *
 * The reference applies every factor's SGD update immediately; the device accumulates a
 * mini-batch and applies it in one step.  Two things keep that step faithful to the
 * reference's sequential updates:
 *  (1) the step of every weight SATURATES at the inverse of its own curvature bound h[w]
 *      (dwx_sgd_apply_async: w -= (1 - exp(-c stepsize)) / c * (G + reg T w), c = h[w] + reg T
 *      -- the end point of the gradient flow the T sequential updates follow).  A weight tied
 *      to millions of factors can therefore never overshoot, whatever the step size; a weight
 *      with few factors takes the reference's own step.  h is a static table (Gershgorin row
 *      sums of the batch's curvature), part of DWX_BUF_TSTATIC*.
 *  (2) dwx_sgd_plan sizes the mini-batches for the given step size: with R = the (estimated)
 *      largest eigenvalue of a batch's curvature in weight space (how strongly all updates of
 *      one batch interact), every colour launch is cut into `batches` runs of tiles carrying
 *      equal SGD work, batches = the first power of two >= stepsize * R(1) / step_cap with
 *      stepsize * R(batches) <= step_cap (1 for configs 2-3 of BASELINE.json at their quoted
 *      step; dozens for heavily tied weights with a large step; never more than 64).  Inside a
 *      batch all draws see the weights of its start, so the cut decides how closely the run
 *      follows the reference from epoch to epoch -- not whether it is stable.
 * effective_stepsize reports the SMALLEST step any weight takes under the plan (== stepsize
 * unless a weight's bound saturates it).  force_batches != 0 overrides the cut (all ranks of a
 * multi-GPU run must use the same value).  A plan is a list of chunks (consecutive device-order
 * runs of variables, never crossing a colour; n_chunks <= batches * colours -- tiles that learn
 * nothing ride along with a neighbour); with batches == 1 the update is applied once after
 * the last chunk, otherwise after every chunk.
 *   dwx_sgd_plan -> n_chunks;  for c in chunks: dwx_sgd_accumulate_async(c) [+ collective,
 *   + dwx_sgd_apply_async where due];  dwx_sgd_finish.
 * DWX_E_LIMIT (dwx_sgd_plan and dwx_sample_sgd_async, before anything is sampled; state untouched, no plan
 * left): a mini-batch of the plan could take a weight's int64 sums -- gradient 2^30 x sum t |g|, update count,
 * curvature bound 2^10 x sum kappa d S -- past 2^63 - 1 in the worst case over all assignments (DESIGN.md 4,
 * "Learning domain"; 65 536 visits of a +-1 factor with feature value 65 536 on one weight).  The text names
 * the weight.  A finer plan (force_batches, a smaller step_cap) whose mini-batches fit is accepted.  Sums a
 * driver all-reduces over ranks are the driver's to bound. */
int dwx_sgd_plan(dwx_sampler *s, double stepsize, uint32_t force_batches, uint32_t *batches,
                 uint32_t *n_chunks, double *effective_stepsize);
/* The curvature estimate R(batches) dwx_sgd_plan works with (cached per batch count).  A
 * multi-GPU driver takes the maximum over ranks once per batch count and can then derive
 * the common plan for any step size without a per-sweep agreement round. */
int dwx_sgd_curvature(dwx_sampler *s, uint32_t batches, double *lambda);
/* Multi-GPU only: make the current split plan's static-count table n_rows tall (rows
 * beyond this rank's own chunks are zero), so that all ranks can sum equally sized tables
 * and every rank can apply the update of a chunk it idles through. */
int dwx_sgd_plan_rows(dwx_sampler *s, uint32_t n_rows);
/* Multi-GPU only: run the CURRENT split plan with per-record gradient atomics and dynamic
 * update counts (the T half of DWX_BUF_GRAD) although this rank has per-chunk tables --
 * because some other rank has none (its chunk count exceeds the table limit) and all ranks
 * must put the same vector through the collective.  No effect on an un-split plan; reset by
 * the next dwx_sgd_plan. */
int dwx_sgd_plan_force_dynamic(dwx_sampler *s, int on);
/* chunk_range[2 * n_chunks]: chunk c covers positions [chunk_range[2c], chunk_range[2c+1]) of
 * the schedule order (dwx_graph_get_schedule).  The chunks of a split plan go round-robin over
 * the colour launches (the reference's id-order scan meets the colours interleaved), so their
 * ranges are not ascending. */
int dwx_sgd_get_chunks(dwx_sampler *s, uint64_t *chunk_range);
int dwx_sgd_accumulate_async(dwx_sampler *s, uint32_t chunk);
int dwx_sgd_apply_async(dwx_sampler *s);
int dwx_sgd_finish(dwx_sampler *s);
/* Multi-GPU (shards), between dwx_sgd_accumulate_async and dwx_sgd_apply_async, when every rank's
 * dwx_graph_info.grad_shift allows it: the gradient sums G[0, W) of DWX_BUF_GRAD as 32-bit counts
 * (int32)(G[i] >> shift) in a device buffer of the library (*dev32, *n elements) for the caller's
 * all-reduce -- half the bytes of the int64 vector -- and back, G[i] = (int64)count << shift.
 * Replaces nothing in the reference (its replicas average weights once per epoch,
 * src/dimmwitted.cc:209-216); dwx_wait fails if a sum was not a multiple of 2^shift or its count was not
 * inside (-2^31, 2^31) -- (-2^15, 2^15) at 16 bits. */
int dwx_grad_pack32_async(dwx_sampler *s, uint32_t shift, void **dev32, uint64_t *n);
int dwx_grad_unpack32_async(dwx_sampler *s, uint32_t shift);
/* The general form: bits = 32 as above, or bits = 16 -- two counts per 32-bit word, word i =
 * c[2i] + 65536 c[2i+1] as arithmetic, *n_words = ceil(W / 2): the all-reduce's 32-bit sums of the
 * words are the packed sums of the counts while every SUMMED count stays inside (-2^15, 2^15), i.e.
 * while (sum over ranks of max_records_per_weight) x grad_unit_max < 2^15 -- a quarter of the int64
 * bytes (config 5a: 2 MB per mini-batch at W = 1 M).  RCCL has no 16-bit integer type, hence words.
 * The check dwx_wait makes covers the packs since the last dwx_wait: it reports their bad sums and starts from 0. */
int dwx_grad_pack_async(dwx_sampler *s, uint32_t shift, uint32_t bits, void **dev32, uint64_t *n_words);
int dwx_grad_unpack_async(dwx_sampler *s, uint32_t shift, uint32_t bits);

/* infrs.weight_values access (src/dimmwitted.cc:209-216 merge/average, :245-258 dump) */
int dwx_get_weights(dwx_sampler *s, double *out);
int dwx_set_weights(dwx_sampler *s, const double *in);
/* Replica averaging, the reference's n_datacopy semantics (DimmWitted::update_weights +
 * copy_weights_to, src/dimmwitted.cc:209-216,199; InferenceResult::merge_weights_from /
 * average_weights, src/inference_result.cc:68-79): every replica (one sampler per GPU on
 * the WHOLE graph, own seed) runs dwx_sample_sgd_async; the driver then sums
 * DWX_BUF_WEIGHTS over the replicas in place (RCCL all-reduce on dwx_stream) and calls this
 * on every replica: weights /= n_replicas (fixed weights are restored verbatim), f32
 * sampling copy refreshed.  Replaces SURVEY.md 8(b)'s dwx_allreduce_weights: the
 * collective itself stays with the caller's communicator. */
int dwx_average_weights_async(dwx_sampler *s, uint32_t n_replicas);
/* InferenceResult::clear_variabletally / sample_tallies + agg_nsamples
 * (src/inference_result.cc:107-127); arrays are in the REFERENCE numbering. */
int dwx_clear_tallies(dwx_sampler *s);
int dwx_get_tallies(dwx_sampler *s, uint64_t *tallies, uint64_t *nsamples);
/* Rao-Blackwellised marginals.  NO reference counterpart: the reference's only estimator counts the drawn
 * values (sample_single_variable, src/gibbs_sampler.h:160-167; dumped as tally / nsamples,
 * src/inference_result.cc:211-243).  Every inference draw first computes the exact conditional
 * P(x_v = d | all other variables) of the variable it samples -- 1 / (1 + exp(pn - pp)) for a boolean
 * variable (draw_sample, src/gibbs_sampler.h:198-215), exp(pot_d - m) / sum_j exp(pot_j - m), m = max_j
 * pot_j, for a categorical one (:217-246) -- from the very potentials the draw decides on.  While the switch
 * is on, every inference sweep (dwx_sample_async, dwx_sample_n_async; never a learning sweep) adds
 * llrint(2^32 * that probability), evaluated in f64, to an unsigned 64-bit sum per value row for every
 * variable it samples (the set whose nsamples grows).  sums / 2^32 / nsamples estimates the same marginal
 * as tallies / nsamples from the same chain (Gelfand & Smith 1990) with a smaller variance wherever a
 * variable's own evidence is informative; on an all-unary graph it is exact after one sweep.  The integer
 * sums do not depend on the kernels a graph takes, on dwx_sample_n_async against single sweeps, or on how
 * a graph without cross-shard factors is split over ranks.  Rows of variables that are not sampled stay 0.
 *   dwx_rb_enable(s, 1)  allocates and zeroes the sums on first use (8 bytes per value row; DWX_E_NOMEM
 *                        leaves the sampler usable, switch off); (s, 0) stops accumulating, keeps the sums.
 *   dwx_get_rb_sums      sums[num_values] and nsamples[num_variables] in the REFERENCE numbering, as
 *                        dwx_get_tallies (either may be null); DWX_E_INVALID when never enabled.
 *   dwx_clear_tallies    zeroes them with the tallies; DWX_BUF_RB is the device array. */
int dwx_rb_enable(dwx_sampler *s, int on);
int dwx_get_rb_sums(dwx_sampler *s, uint64_t *sums, uint64_t *nsamples);
/* Posterior sample trace.  NO reference counterpart: the reference overwrites every assignment with the next
 * sweep's and keeps counts only (sample_single_variable, src/gibbs_sampler.h:160-167), so neither a variable's
 * draws as a sequence (split-R-hat, effective sample size: sampler_amd/diagnostics.py) nor a joint sample
 * (co-occurrences, P(a and b)) can be had from it.  The trace is a ring, on the device, of the assignments of the
 * inference chain (chain 1, the one dwx_sample_async advances) after each of the last `capacity` INFERENCE
 * sweeps (dwx_sample_async, dwx_sample_n_async; never a learning sweep), packed: 1 bit per owned variable
 * when no owned variable is categorical, else 1 byte.  Ghost variables are not traced.
 *   dwx_trace_enable(s, capacity)  allocates the ring on first use (capacity x ceil(V_owned / 64) x 8 bytes, or
 *                        capacity x ceil(V_owned / 8) x 8; DWX_E_NOMEM leaves the sampler usable, trace off);
 *                        capacity 0 stops recording and keeps what is there; a different non-zero capacity
 *                        reallocates and empties the ring; DWX_E_LIMIT when max_cardinality > 256.
 *   dwx_trace_info       entries held, the capacity, and (sweep_ids[count], may be null) oldest first the
 *                        value of the sweep counter each entry was drawn at -- the Philox counter word of that
 *                        sweep (dwx_get_sweep before it ran): learning sweeps in between leave gaps.
 *   dwx_trace_read       out[e * n_vids + i] = the dense value of variable vids[i] (REFERENCE numbering) in
 *                        entry first_entry + e (0 = oldest), as dwx_get_assignments(s, 1, ...) would have
 *                        returned it right after that sweep -- also for a variable the sweep does not sample
 *                        (evidence without sample_evidence: the value it had).  vids == NULL: all owned variables,
 *                        n_vids ignored.  The selection is gathered and unpacked on the device: only
 *                        n_entries x n_vids bytes cross to the host.  DWX_E_INVALID when never enabled, on a
 *                        range outside the entries held, on a ghost or unknown id.
 *   dwx_clear_tallies    empties the trace with the tallies: while count <= capacity, the number of entries
 *                        with value d equals tallies[row0 + d] for every sampled variable.
 * With the trace off nothing is launched or allocated for it.  Both uses have a device path that reads the ring
 * where it lies: dwx_trace_diagnostics (the sequences) and dwx_trace_cooccurrence (the joint counts), below. */
int dwx_trace_enable(dwx_sampler *s, uint32_t capacity_sweeps);
int dwx_trace_info(dwx_sampler *s, uint64_t *count, uint64_t *capacity, uint64_t *sweep_ids);
int dwx_trace_read(dwx_sampler *s, uint64_t first_entry, uint64_t n_entries, const uint64_t *vids, uint64_t n_vids,
                   uint8_t *out);
/* Split-R-hat and effective sample size of EVERY value row, computed on the device from the ring where it lies.
 * NO reference counterpart: the reference only counts the drawn values (sample_single_variable,
 * src/gibbs_sampler.h:160-167) and keeps no sequence to judge.  dwx_trace_read + sampler_amd/diagnostics.py is
 * the route for a selection of variables and for several chains; this one reads the ring once (n x ceil(V / 64)
 * x 8 bytes at a bit per variable) and returns two doubles per row, or the summary alone.
 * Rows are value rows in the REFERENCE numbering, as in dwx_get_tallies and dwx_graph_get_values: a boolean
 * variable has one row, the indicator of value 1; a categorical variable one row per dense value d, the indicator
 * x == d.  Every owned variable gets its rows, sampled or not (an unsampled variable's series is whatever the
 * trace holds for it); ghost variables have none, their rows of the arrays are left as they were.
 * Definition (single chain).  x_0 .. x_{n-1}: a row's 0/1 series over the n entries held, oldest first; the
 * entries are taken as consecutive whatever their sweep ids (summary.contiguous tells).  Integer statistics:
 *   k = sum x_i;  h = n / 2 (integer);  k1 = sum_{i < h} x_i;  k2 = sum_{i >= n - h} x_i (the middle draw of an
 *   odd n is dropped);  for t = 0 .. max_lag:  c_t = sum_{i < n - t} x_i x_{i+t},  H_t = sum_{i < n - t} x_i,
 *   T_t = sum_{i >= t} x_i.
 * split-R-hat, in f64 as IEEE arithmetic has it:
 *   var_j = (k_j - k_j^2 / h) / (h - 1);  W_s = (var_1 + var_2) / 2;  B = (k1 / h - k2 / h)^2 / 2;
 *   rhat = sqrt(((h - 1) / h * W_s + B) / W_s):  nan when W_s = 0 and B = 0, +inf when W_s = 0 and B > 0 (halves
 *   that are constant and different) -- diagnostics.split_rhat of the same draws.
 * ESS: nan when k = 0 or k = n.  Otherwise m = k / n, W = (k - k^2 / n) / (n - 1), var+ = (k - k^2 / n) / n,
 *   a_t = (c_t - m (H_t + T_t) + (n - t) m^2) / n,  rho_t = 1 - (W - a_t) / var+,  and Geyer's initial positive
 *   sequence: t = 0, s = 0; while t + 1 < n: pair = rho_t + rho_{t+1}; stop if !(pair > 0); s += pair; t += 2.
 *   tau = 1 + 2 (s - rho_0) if t > 0 else 1;  ess = n / tau -- diagnostics.ess of that one chain.  Where the loop
 *   would need rho_{t+1} with t + 1 > max_lag it stops there instead: the row is flagged truncated and its ess,
 *   from the pairs summed so far, is an upper bound.
 * rhat, ess ([num_values] doubles) and flags ([num_values] bytes: bit 0 constant, bit 1 truncated) may each be
 * null; with all three null only the summary crosses to the host.  summary may be null, but not with all three.
 * DWX_E_INVALID: trace never enabled, fewer than 4 entries held, max_lag outside 1 .. 64, nothing to return.
 * DWX_E_NOMEM (the temporary device arrays: up to 17 bytes per row) leaves the sampler usable.  The call is
 * ordered after everything queued on the sampler's stream and returns when done, like dwx_trace_read; it changes
 * nothing of the sampler's state.  With the function never called nothing is launched or allocated for it. */
typedef struct dwx_trace_diag_summary {
  uint64_t n_entries;       /* entries the statistics are over (= dwx_trace_info's count)           */
  uint32_t max_lag;         /* as passed                                                            */
  uint32_t contiguous;      /* 1: the entries' sweep ids are consecutive (no learning sweep between) */
  uint64_t rows_finite;     /* rows whose rhat is finite                                            */
  uint64_t rows_constant;   /* rows whose series never changed: rhat and ess are nan                */
  uint64_t rows_truncated;  /* rows whose autocorrelation sum reached max_lag before Geyer's cut    */
  uint64_t rows_rhat_above; /* rows with rhat > rhat_threshold (inf counts, nan does not)           */
  double max_rhat;  uint64_t max_rhat_row;   /* over rows that are not nan; a row attaining it      */
  double min_ess;   uint64_t min_ess_row;    /* over rows that are not nan; a row attaining it      */
} dwx_trace_diag_summary;   /* (no row that is not nan: the value is nan, the row UINT64_MAX) */
int dwx_trace_diagnostics(dwx_sampler *s, uint32_t max_lag, double rhat_threshold, double *rhat, double *ess,
                          uint8_t *flags, dwx_trace_diag_summary *summary);
/* Joint counts of PAIRS of value rows over the sample trace, counted on the device from the ring where it lies.
 * NO reference counterpart: the reference keeps counts only (sample_single_variable, src/gibbs_sampler.h:160-167)
 * and overwrites every assignment with the next, so it cannot tell whether two things were true TOGETHER.
 * dwx_trace_read ships a byte per (entry, variable) to the host for that; this call ships the pairs up and three
 * integers per pair down.
 * Rows are value rows in the REFERENCE numbering, as in dwx_get_tallies, dwx_graph_get_values and
 * dwx_trace_diagnostics: a boolean variable has one row, the indicator of value 1; a categorical variable one row per
 * dense value d, the indicator x == d.  A row's series x_r(e) is exactly the series dwx_trace_diagnostics defines
 * for it; an unsampled owned variable has one too (whatever the trace holds for it).  A ghost variable has no value
 * rows at all (num_values counts the owned variables' rows), so none of its can be named.
 * Definition.  E = [first_entry, first_entry + n_entries), entry 0 the oldest held (as dwx_trace_read).  For pair i:
 *   n_ab[i] = #{e in E: x_{rows_a[i]}(e) = 1 and x_{rows_b[i]}(e) = 1},
 *   n_a[i]  = #{e in E: x_{rows_a[i]}(e) = 1},   n_b[i] = #{e in E: x_{rows_b[i]}(e) = 1}.
 * n_a and n_b may each be null; n_ab may not.  P(a and b) = n_ab / n_entries, P(a and not b) = (n_a - n_ab) /
 * n_entries, lift, phi and the like are the caller's (sampler_amd/diagnostics.py: cooccurrence_stats): the library
 * returns integers only.  Pairs may repeat; rows_a[i] == rows_b[i] is allowed (n_ab == n_a == n_b); two different
 * values of one categorical variable give n_ab == 0.  While count <= capacity after dwx_clear_tallies, n_a over all
 * entries equals tallies[rows_a[i]] for a sampled variable's row.
 * n_entries == 0 (a valid range) returns DWX_OK and zeroes every output; n_pairs == 0 returns DWX_OK and touches
 * nothing, whatever the pointers.
 * DWX_E_INVALID: trace never enabled; first_entry + n_entries > count (dwx_trace_info); n_ab, rows_a or rows_b null
 * with n_pairs > 0; a row >= num_values (a ghost variable has no rows: there is no other "ghost row" case).
 * DWX_E_LIMIT: n_entries > 2^31 - 1 or a ring of more than 2^31 - 1 sweeps (the kernel's counts and plane cursor are
 * 32-bit); n_pairs > 2^32 - 1 (a bound of the call, not of the kernel, whose pair index is 64-bit: the temporary
 * arrays of such a call would exceed 146 GB -- split the list).
 * DWX_E_NOMEM (the temporary device arrays: up to 34 bytes per pair) leaves the sampler usable.  After any error
 * return the output arrays are as they were.  Each row is translated to a (device position, dense value) once per
 * call on the host; only the translated pairs go up (8 or 10 bytes per pair) and 3 x 8 x n_pairs bytes come down.
 * The call is ordered after everything queued on the sampler's stream and returns when done, like dwx_trace_read;
 * it changes nothing of the sampler's state.  With the function never called nothing is launched or allocated for
 * it. */
int dwx_trace_cooccurrence(dwx_sampler *s, const uint64_t *rows_a, const uint64_t *rows_b, uint64_t n_pairs,
                           uint64_t first_entry, uint64_t n_entries, uint64_t *n_ab, uint64_t *n_a, uint64_t *n_b);
/* Joint log-score of a state under the model, computed on the device.  The reference has no counterpart beyond the
 * per-variable sum FactorGraph::potential (src/factor_graph.h:127-145), which this extends to ALL factors.
 * Definition.  For a joint assignment x (dense values, as dwx_get_assignments / dwx_trace_read give them):
 *   score(x) = sum over f of  w[weight_id_f] * (sign_f(x) * feature_value_f)
 * over ALL factors of the graph (those on fixed weights and on evidence variables included); sign_f is the factor
 * function of src/factor.h:112-299 with no variable proposed; w is the f64 master weights (DWX_BUF_WEIGHTS) at the
 * time of the call -- the weights a run dumps.  score(x) is the log of the unnormalised probability; the partition
 * function is not estimated.
 * Numerics (independent of kernels, grid sizes and the order of atomics):  t_f = w * (s * fval), two f64
 * multiplications in that association, no contraction;  q_f = llrint(2^32 * t_f) (round-to-nearest-even);  the q_f are
 * summed EXACTLY (q >> 32 into a signed 64-bit sum, the low 32 bits into an unsigned one: F < 2^32, neither can
 * overflow);  the result is (double)(((__int128)hi << 32) + lo) * 2^-32: the correctly rounded value of the exact
 * integer sum over 2^32, also where that sum is beyond int64.  A term that is not finite or has |t_f| >= 2^30 makes the
 * call fail with DWX_E_LIMIT, the outputs left as they were.  (RATIO at arity >= 3 takes log2 of 3, 4, ... on the
 * device: its sign is the device's f64 log2, within 1 ulp of the true value.)
 *   dwx_score        the score of a live chain (chain as in dwx_get_assignments: 0 free, 1 evidence); deferred draws
 *                    (dwx_kernel_time, kind 7) are run first, exactly as dwx_get_assignments does; ghost variables'
 *                    assignments are read like any other.
 *   dwx_trace_score  scores[e] of entries [first_entry, first_entry + n_entries) of the sample trace, entry 0 the
 *                    oldest held (as dwx_trace_read); best_entry (may be null): the entry of the range with the largest
 *                    score, the OLDEST on a tie.  n_entries == 0 is DWX_OK, *best_entry = UINT64_MAX.
 * Both need a graph compiled with dwx_compile_opts.keep_factors; the device copy of its factor table is uploaded by
 * the first call and freed by dwx_sampler_destroy (DWX_E_NOMEM there, or for the call's few temporary bytes, leaves
 * the sampler usable).  Both are ordered after everything queued on the sampler's stream, return when done and change
 * nothing of the sampler's state (sweep counter, chains, tallies, RB sums, trace).  A graph without factors scores 0.
 * DWX_E_INVALID: the graph was compiled without keep_factors; a null output; a chain other than 0 / 1;
 * dwx_trace_score: trace never enabled, a range outside the entries held, a graph with ghost variables (they are not
 * traced).  With neither function ever called nothing is allocated or launched. */
int dwx_score(dwx_sampler *s, int chain, double *score);
int dwx_trace_score(dwx_sampler *s, uint64_t first_entry, uint64_t n_entries, double *scores, uint64_t *best_entry);
/* Per-weight feature sums -- the model's sufficient statistics -- of a state or of a range of traced states, computed
 * on the device.  The reference has no counterpart: its learning sweep forms the gradient one variable at a time
 * and never reports the sums.
 * Definition.  For a joint assignment x,  u_f = sign_f(x) * feature_value_f  (one f64 product, no contraction; sign_f
 * exactly as in dwx_score: the factor function with no variable proposed) and  q_f = llrint(2^32 * u_f)
 * (round-to-nearest-even), over ALL factors, those on fixed weights and on evidence variables included.
 *   dwx_weight_stats        stats[w] = the correctly rounded value of (sum over the factors f on weight w of q_f) / 2^32
 *                           for a live chain (0 free, 1 evidence); deferred draws are run first, as dwx_score does.
 *   dwx_trace_weight_stats  sums[w] = the correctly rounded value of (sum over the entries e of [first_entry,
 *                           first_entry + n_entries) and over the factors f on w of q_f(x_e)) / 2^32, entry 0 the
 *                           oldest held (as dwx_trace_read).  The caller divides by n_entries for the mean: for the
 *                           +-1 functions that is 2 * (satisfied fraction) - 1 of the rule under the posterior.
 * Both arrays have num_weights entries; a weight that no factor names reads 0.0.  The weights' VALUES take no part:
 * after dwx_set_weights the result is bit for bit the same.  stats(evidence chain) - stats(free chain) is the
 * one-sample estimate of d log-likelihood / d w.
 * Numerics.  The per-weight sums are integers and exact: q >> 32 into a signed 64-bit sum, the low 32 bits into an
 * unsigned one, the result (double)(((__int128)hi << 32) + lo) * 2^-32; it does not depend on the grid, on which lanes
 * combined their terms before the atomics or on the atomics' order.  A term that is not finite or has |u_f| >= 2^30
 * makes the call fail with DWX_E_LIMIT.  The two limbs hold fewer than 2^32 terms per weight: the call fails with
 * DWX_E_LIMIT -- before anything is launched, the error text naming the weight -- when n_entries * (factors on the
 * most-used weight) >= 2^32 (the count is taken once, when the first of these calls runs); the caller splits the
 * entry range and adds.  (RATIO at arity >= 3: as for dwx_score.)
 * Both need a graph compiled with dwx_compile_opts.keep_factors and share the device copy of the factor table with
 * dwx_score / dwx_trace_score (whichever call comes first uploads it).  Temporary device memory: 16 bytes per weight
 * (the per-weight factor counts stay on the host); DWX_E_NOMEM leaves the sampler usable.  Both are ordered after
 * everything queued on the sampler's stream, return when done and change nothing of the sampler's state (sweep
 * counter, chains, tallies, RB sums, trace, weights, the pack check).  n_entries == 0 is DWX_OK and all zeros; so is a
 * graph without factors.  After any error return the output array is as it was.
 * DWX_E_INVALID: the graph was compiled without keep_factors; a null output; a chain other than 0 / 1;
 * dwx_trace_weight_stats: trace never enabled, a range outside the entries held, a graph with ghost variables (they
 * are not traced).  With neither function ever called nothing is allocated or launched. */
int dwx_weight_stats(dwx_sampler *s, int chain, double *stats /* [num_weights] */);
int dwx_trace_weight_stats(dwx_sampler *s, uint64_t first_entry, uint64_t n_entries, double *sums /* [num_weights] */);
/* assignments_free (chain 0) / assignments_evid (chain 1), original variable order */
int dwx_get_assignments(dwx_sampler *s, int chain, uint64_t *out);
int dwx_set_assignments(dwx_sampler *s, int chain, const uint64_t *in);
/* sweep counter (the Philox counter word); starts at 0, +1 per sweep */
int dwx_get_sweep(dwx_sampler *s, uint64_t *out);
int dwx_set_sweep(dwx_sampler *s, uint64_t sweep);

/* Raw device buffers, so the caller's collective library (RCCL via
 * torch.distributed or rccl.h) can reduce / exchange in place. */
enum {
  DWX_BUF_WEIGHTS = 0,      /* double[W]                                            */
  DWX_BUF_GRAD = 1,         /* int64[2W]: fixed-point (2^-30) gradient sums G[W],
                               then update counts T[W]                             */
  DWX_BUF_ASSIGN_FREE = 2,  /* uint32[V] in device order                           */
  DWX_BUF_ASSIGN_EVID = 3,  /* uint32[V] in device order                           */
  DWX_BUF_TALLIES = 4,      /* uint32[num_values] in device order                  */
  DWX_BUF_TSTATIC = 5,      /* int64[2W]: per-sweep update counts T[W] of boolean variables
                               (fixed point 2^-30), then the curvature bounds h[W] of
                               all variables (fixed point 2^-10); static; a multi-GPU
                               driver sums it across shards once after create      */
  DWX_BUF_TSTATIC_PLAN = 6, /* int64[rows][2W]: the same pair per chunk of the current
                               SPLIT plan (valid between dwx_sgd_plan and dwx_sgd_finish;
                               null / 0 bytes when the plan counts dynamically).  A
                               multi-GPU driver calls dwx_sgd_plan_rows(n_chunks of the
                               slowest rank) and sums the table across shards ONCE per
                               batch count (the library caches it per batch count)   */
  DWX_BUF_SORTED_RECORDS = 7,      /* test hooks: the weight-sorted record copy of the graph's default  */
  DWX_BUF_SORTED_RECORDS_PLAN = 8, /* layout / of the current plan level's own (8 bytes per record;
                                      null / 0 bytes when there is none): the device build
                                      (device_build.hip) is checked against the host builder's bytes  */
  DWX_BUF_RB = 9,           /* uint64[num_values] in device order, like DWX_BUF_TALLIES: the
                               Rao-Blackwellised sums (2^-32 fixed point; dwx_rb_enable); null / 0
                               bytes when never enabled.  Replicas sum it with a 64-bit integer sum  */
  DWX_BUF_TRACE = 10        /* the sample trace's ring (dwx_trace_enable), in the library's OWN device
                               layout (packed planes in device order, a ring) -- not for interpretation,
                               read it through dwx_trace_read; here so that its footprint can be seen:
                               capacity x ceil(V_owned / 64) x 8 bytes on an all-boolean graph, no
                               other padding.  Null / 0 bytes when never enabled  */
};
int dwx_device_buffer(dwx_sampler *s, int which, void **dev_ptr, uint64_t *nbytes);
/* Copy between host memory and a device pointer obtained from dwx_device_buffer /
 * dwx_halo_buffer (to_device != 0: host -> device), ordered after everything already queued
 * on the sampler's stream; returns when the copy is done.  For drivers without a device
 * runtime of their own (the host-staged test communicator of `dw gibbs --comm host`). */
int dwx_buffer_copy(dwx_sampler *s, void *dst, const void *src, uint64_t nbytes, int to_device);
/* Halo exchange support (multi-GPU with factors that cross the shard boundary; SURVEY.md 8e:
 * "exchange halo assignments ... grouped in one ncclGroupStart/End").  A halo list is one side
 * of the exchange with one peer: `vids` = local variable ids (owned variables a peer ghosts:
 * a SEND list; ghost variables a peer owns: a RECEIVE list, dwx_graph_desc.num_ghost_variables)
 * and a device buffer for both chains.  dwx_halo_pack_async gathers the listed variables'
 * assignments of the selected chains (bit 0: free chain, bit 1: evidence chain; selected
 * chains back to back, see dwx_halo_message_bytes) into the buffer; the caller moves buffers between
 * ranks with its collective library on dwx_stream (ncclSend / ncclRecv); dwx_halo_unpack_async
 * scatters a received buffer into the ghosts.  All on the sampler's stream, no host
 * synchronisation.  (No reference counterpart: the reference's threads share one address
 * space and read each other's assignments directly, src/gibbs_sampler.h:198-215.) */
typedef struct dwx_halo dwx_halo;
int dwx_halo_create(dwx_sampler *s, const uint64_t *vids, uint64_t n, dwx_halo **out);
void dwx_halo_destroy(dwx_halo *h);
int dwx_halo_buffer(dwx_halo *h, void **dev_ptr, uint64_t *nbytes);
/* Bytes at the start of the buffer that dwx_halo_pack_async(h, chains) fills and
 * dwx_halo_unpack_async(h, chains) reads -- what to send / receive.  Values travel as 1 bit
 * (every listed variable boolean), 8 bits (every listed cardinality <= 256) or 32 bits each,
 * the selected chains' blocks back to back, each padded to 8 bytes; the peer's list of the same
 * variables gives the same number. */
int dwx_halo_message_bytes(dwx_halo *h, int chains, uint64_t *nbytes);
int dwx_halo_pack_async(dwx_halo *h, int chains);
int dwx_halo_unpack_async(dwx_halo *h, int chains);

/* The HIP stream (hipStream_t) the sampler enqueues on. */
int dwx_stream(dwx_sampler *s, void **stream);

/* Device time of the sweep kernels only, measured with HIP events on the sampler's
 * stream around every launch since the last reset: total milliseconds, number of
 * kernel launches and number of sweeps (a learning sweep of several colours or
 * mini-batches is ONE sweep of several launches).  kind: 0 = inference sweep kernels, 1 = learning
 * sweep kernels, 2 = the pull-based gradient kernel of learning sweeps, 3 = no time: launches =
 * sweeps = the split learning sweeps dwx_sample_sgd_async handed over as ONE graph launch since
 * the sampler was created (DWX_GRAPH=n in the environment: a sweep of >= n mini-batches is
 * captured and replayed as a hipGraph from the plan level's second sweep on, never while timing
 * is enabled; off by default -- measured, it buys nothing: DESIGN.md section 3.5); 4 = no time:
 * launches = sweeps = the split learning sweeps that ran as ONE persistent launch (DWX_PERSIST=1 in the
 * environment at dwx_sampler_create; all-unary graphs with at most 128 weights, >= 8 mini-batches:
 * chunk loop, grid barrier and update inside the kernel; off by default -- measured, it is slower
 * than the launches it replaces: sampler_amd/csrc/persist_kernels.h); 5 = no time: launches = sweeps =
 * the split learning sweeps that ran with ONE launch per mini-batch -- the update of a mini-batch as the
 * prologue of the next one's sweep kernel (all-unary graphs with at most 1024 weights and no
 * degree-binned variable; the default for them, DWX_NO_MERGED_APPLY=1 at dwx_sampler_create disables it); 6 = no
 * time: launches = the weight-sorted super-tiles of learning sweeps that took their potentials from the
 * potential cache instead of streaming their records, sweeps = the learning sweeps that read it, since the
 * sampler was created (all-unary graphs with weight-sorted learning sweeps, an un-split learning sweep right
 * after an inference sweep on the same weights; DWX_NO_POT_CACHE=1 at the first inference sweep disables it); 7 = the
 * deferred draws: ms = device time of the flushes since the last reset, launches = the flushes and
 * sweeps = the learning sweeps that deferred since the sampler was created.  An un-split learning sweep of an
 * all-unary graph (learn_non_evidence and noise_aware off) launches over its evidence tiles only; the draws of its
 * query variables, which nothing reads while sweeps follow each other, are run -- with that sweep's counter and
 * weights, the same values bit for bit -- only when dwx_get_assignments, dwx_set_assignments, dwx_set_sweep, a halo
 * exchange or dwx_device_buffer(DWX_BUF_ASSIGN_*) asks before a later sweep has overwritten them.
 * dwx_device_buffer(DWX_BUF_ASSIGN_*) also ends deferral for the rest of the sampler's life (the caller keeps the
 * pointer); DWX_NO_DEFER=1 at dwx_sampler_create disables it. */
int dwx_kernel_time(dwx_sampler *s, int kind, double *ms, uint64_t *launches, uint64_t *sweeps);
int dwx_kernel_time_reset(dwx_sampler *s, int enable);

/* Test hook: evaluate one factor function on the device.  sat[i] = whether the
 * predicate of position i holds; mirrors test/factor_test.cc's truth tables. */
int dwx_test_factor_sign(int device, int func, uint64_t arity, const uint8_t *sat, double *out);
/* Test hook: the device's random number generator (the reference draws with erand48,
 * src/gibbs_sampler.h:177,204,230; the device with the counter-based Philox4x32-10 of Salmon
 * et al., SC'11).  out = philox(key, ctr), the raw block function (Random123's known-answer
 * vectors apply); uniforms = the two 53-bit uniforms the sweep kernels draw for
 * (seed = key, variable id = ctr[0..1], sweep = ctr[2..3]). */
int dwx_test_philox(int device, const uint32_t key[2], const uint32_t ctr[4], uint32_t out[4],
                    double uniforms[2]);
/* Test hook: the wave-level primitives of the kernels (sampler_amd/csrc/device_intrinsics.h: the gfx950 forms; the
 * tests' host emulation: its stand-ins), called by ONE workgroup of 256 lanes on the caller's per-lane inputs; every
 * lane's result comes back.  `in` and `out` are arrays of 8-byte words; n is the number of input words.
 *   DWX_WAVE_OP_SEG_SUM   in[512]: 256 keys (low 32 bits), 256 int64 addends.  out[512]: per lane the sum from the
 *                         lane to the end of its run of equal keys inside its wave, then 1 where the lane heads a run
 *   DWX_WAVE_OP_SUM_F64   in[256] doubles.  out[256]: per lane the sum over its wave (xor-butterfly association)
 *   DWX_WAVE_OP_BALLOT    in[256] predicates (non-zero = true).  out[256]: the wave's ballot as every lane sees it
 *   DWX_WAVE_OP_PAIR_SWAP in[256] values (low 32 bits).  out[256]: the value lane ^ 1 passed
 *   DWX_WAVE_OP_LOAD16 / LOAD8   in[0] = n_rec records of 16 / 8 bytes, in[1 ..]: their bytes (exactly n_rec records
 *                         are allocated on the device).  K = 12 loads per lane: out[(k * 256 + t) * 2 .. + 2] / out[k *
 *                         256 + t] = the record lane t got for slot k (record t + 256 k; zeros past the end)
 *   DWX_WAVE_OP_LOAD_SORTED      in[0] = n_rec, in[1] = first, in[2 ..] the 8-byte records.  K = 4 loads per lane, the
 *                         workgroup's lanes standing for lanes t < 256 of the sorted sweep: out[k * 256 + t] = record
 *                         first + t + k * SORT_THREADS (1024), zeros past n_rec
 * DWX_E_INVALID on an unknown op or a length that does not match. */
enum {
  DWX_WAVE_OP_SEG_SUM = 0, DWX_WAVE_OP_SUM_F64 = 1, DWX_WAVE_OP_BALLOT = 2, DWX_WAVE_OP_PAIR_SWAP = 3,
  DWX_WAVE_OP_LOAD16 = 4, DWX_WAVE_OP_LOAD8 = 5, DWX_WAVE_OP_LOAD_SORTED = 6
};
int dwx_test_wave_ops(int device, int op, const uint64_t *in, uint64_t n, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* DWX_H_ */
