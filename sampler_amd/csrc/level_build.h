// level_build.h -- the host builders of a learning plan level: pure functions of a CompiledGraph and the
// options, host data in and out.  They are the checker of the device build (device_build.h), the builders
// DWX_HOST_BUILD=1 selects and the only ones the tests' host emulation runs; dwx_api.cc uploads their results.
#ifndef DWX_LEVEL_BUILD_H_
#define DWX_LEVEL_BUILD_H_

#include <stdint.h>
#include <vector>

#include "graph_compile.h"

namespace dwx {

// a variable with these v_meta bits runs SGD in a learning sweep (sgd_on_variable)
bool triggers_sgd(const dwx_options &o, uint32_t meta);

// Tile boundaries of colour launch l cut into at most nb runs of (nearly) equal SGD work
// (records visited by sgd_on_variable; query variables sample but do not learn, so a cut
// by tile count would put all the learning of an evidence-after-query launch in half of the batches).
// sgd_work: [tiles + 1] prefix sums of that work, sgd_work_max_launch: that of the colour launch with the
// most.  Returns strictly increasing boundaries from the launch's first tile to its last.
std::vector<uint32_t> cut_launch(const CompiledGraph &c, const std::vector<uint64_t> &sgd_work, uint64_t sgd_work_max_launch,
                                 size_t l, uint32_t nb);

// The domain of the learning sums: per group of variables that share an update
// (`groups`: device-order position ranges) and per weight, the worst case of the int64 sums G, T and h
// over any assignment.  -> empty, or the text of the DWX_E_LIMIT error, naming the weight.
std::string learning_range_error(const CompiledGraph &c, const dwx_options &o,
                                 const std::vector<std::pair<uint32_t, uint32_t>> &groups);

namespace hostb {
struct TileGroup { uint32_t t0, t1; };   // the tiles whose variables share an update: a chunk, or the whole un-split sweep

// A plan level's static tables, one row pair per group: table[groups][T[W] | h[W]] -- the update counts
// of the boolean variables (a boolean variable that triggers SGD visits every factor of its row once
// with t = 1, src/factor_graph.cc:265-273, whatever the samples drawn; fixed point 2^-30) and the
// curvature bounds of all variables (apply_kernel's saturating step; 2^-10); *t_max / *h_max: the largest
// entries, the fixed-point integers devb::build_static_tables reports.
void build_static_tables(const CompiledGraph &c, const dwx_options &o, const std::vector<TileGroup> &groups,
                         RawArray<long long> &table, long long *t_max, long long *h_max);

// A plan level's pull-gradient structures: devb::Incidence with host arrays where that has device
// pointers.  The incidence list of every (variable, non-fixed record with a non-zero delta) pair of the
// pull tiles, sorted by (group, weight) (two stable parallel counting sorts: by weight, then by group),
// every group padded to whole runs of PULL_RUN; and -- graphs with >= block_pull_min_w weights and few
// distinct deltas -- per group the block-pull table, with only what did not fit a row left on the list.
// Throws std::invalid_argument when the list exceeds 2^32 - 1 entries.
struct Incidence {
  RawArray<uint32_t> inc_wid, inc_slot;          // the padded columns
  RawArray<float> inc_d;
  std::vector<uint32_t> inc_begin, inc_end;      // per group: its part of the columns
  struct BlockTable {
    RawArray<unsigned long long> ell;            // [blocks][depth][wp] rows as 8-byte words (a U32x4 row is two)
    std::vector<uint32_t> tile0;                 // [blocks] first tile of every variable block
    std::vector<uint64_t> ov_start;              // [W + 1]: where each weight's leftovers start in the group's list
    uint32_t blocks = 0, depth = 0;              // blocks == 0: the group keeps its whole list
    uint32_t tiles = 0;                          // tiles per block (bp_block_tiles)
    bool one_plane = false;                      // the rows are one-plane packed words (device_types.h: bp1_pack_entry)
    uint64_t total = 0, on_list = 0;             // the group's entries; those left on the list
  };
  std::vector<BlockTable> bp;                    // [groups], or empty: no block pull
  std::vector<uint32_t> dvals;                   // ascending f32 bit patterns of the distinct deltas
  uint64_t max_blocks = 0, wp = 0;
};
// bp_tiles: tiles per block, 0 = the row format's default; allow_one_plane: groups that qualify (bp_one_plane) take
// the one-plane rows
void build_incidence(const CompiledGraph &c, const dwx_options &o, const std::vector<TileGroup> &groups,
                     uint64_t block_pull_min_w, uint64_t bp_tiles, bool allow_one_plane, Incidence &out);

// Curvature of the SGD mini-batch of variables [p0, p1) in weight space: max(power-iteration estimate,
// largest diagonal entry), WITHOUT row_sum_bound's 1.1 safety factor -- the contract of
// devb::batch_curvature, whose arithmetic is the dense branch's term for term.  A batch that touches a
// good part of the weight table (batch_is_dense) takes dense passes over it on all host threads, any
// other a serial sparse walk.  `sc`: scratch vectors kept between calls.
struct CurvatureScratch {
  std::vector<double> x, y, diag;
  std::vector<uint8_t> seen;
  std::vector<uint32_t> touched;
};
inline bool batch_is_dense(const CompiledGraph &c, uint32_t p0, uint32_t p1) {
  return (uint64_t)(p1 - p0) * 8 >= c.W && p1 - p0 >= 65536;
}
double batch_curvature(const CompiledGraph &c, const dwx_options &o, uint32_t p0, uint32_t p1, CurvatureScratch &sc);

}  // namespace hostb
}  // namespace dwx
#endif
