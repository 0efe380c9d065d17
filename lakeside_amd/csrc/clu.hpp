// The name-clustered value copy's tile rule, stated once and pinned on the CPU (tests/test_clu_rule_cpu.py through
// clu_sim.cpp).  Plain C++ with no engine header, like bucket.hpp: scan_clu inlines clu_classify per tile, the host
// (eval.cpp) decides with clu_segment_taken which segments scan_clu takes whole.
//
// scan_clu gives a tile's rows their bucket without a timestamp per row, by scan_lean's two rules (lean_kernel.hpp):
// the zone map pins the tile to one bucket, or the tile is a split tile -- its timestamps never decrease and it meets
// at most CLU_SPLIT_MAX - 1 buckets, so the rows' classes (0 before the window, 1 .. span its buckets, span + 1 after
// the window) follow from a few boundary rows.  Metrics queries (rows checked on the step grid) are never taken.
#pragma once
#include <stdint.h>

#include "bucket.hpp"
#include "layout.hpp"

namespace lk {

constexpr uint32_t CLU_SPLIT_MAX = 4;   // class boundaries of a split tile at most (scan_lean's LEAN_SPLIT_MAX)

// A tile block's layout (layout.hpp, CluTile), stated once for Engine::build_cluster, clu_build and scan_clu and pinned
// on the CPU (tests/test_clu_layout_cpu.py through clu_sim.cpp): [cpref + NaN mask | cagg | cvals | crows].
// dict_n is taken as 1 .. 64, as the builder takes it.
LK_BK_HD inline uint32_t clu_dict_n(uint32_t dict_n) { return dict_n < 1u ? 1u : (dict_n > 64u ? 64u : dict_n); }
LK_BK_HD inline uint32_t clu_vals_off(uint32_t dict_n) { return CLU_AGG_OFF + clu_dict_n(dict_n) * uint32_t(sizeof(CluAgg)); }
LK_BK_HD inline uint64_t clu_rows_off(uint32_t nrows, uint32_t dict_n) { return clu_vals_off(dict_n) + uint64_t(nrows) * 8u; }
LK_BK_HD inline uint64_t clu_block_bytes(uint32_t nrows, uint32_t dict_n) {
  const uint64_t b = clu_rows_off(nrows, dict_n) + uint64_t(nrows) * 2u;
  return (b + (CLU_BLOCK_ALIGN - 1u)) / CLU_BLOCK_ALIGN * CLU_BLOCK_ALIGN;
}

enum CluKind : uint32_t {
  CLU_NONE = 0,     // outside the glob window: no row of the tile counts
  CLU_PINNED,       // every row in bucket b0
  CLU_SPLIT,        // nsb boundaries, classes 1 .. nsb - 1 are buckets b0 .. b0 + nsb - 2
  CLU_UNTAKEN       // inside the window, but neither rule gives the rows' buckets
};

struct CluClass {
  CluKind kind;
  int64_t b0;
  uint32_t nsb;
};

LK_BK_HD inline CluClass clu_classify(int64_t ts_min, int64_t ts_max, int64_t win_lo, int64_t win_hi, int64_t step,
                                      int64_t base, uint64_t nbuckets, bool sorted, bool split_ok) {
  if (ts_max < win_lo || ts_min >= win_hi) return CluClass{CLU_NONE, 0, 0u};
  if (ts_min >= win_lo && ts_max < win_hi) {
    const int64_t b0 = bucket_mono(ts_min, step, base, false);
    const int64_t b1 = bucket_mono(ts_max, step, base, false);
    if (b0 == b1 && b0 >= 0 && uint64_t(b0) < nbuckets) return CluClass{CLU_PINNED, b0, 0u};
  }
  if (sorted && split_ok) {
    const int64_t lo_ts = ts_min > win_lo ? ts_min : win_lo;
    const int64_t hi_ts = ts_max < win_hi - 1 ? ts_max : win_hi - 1;
    const int64_t bl = bucket_mono(lo_ts, step, base, false), bh = bucket_mono(hi_ts, step, base, false);
    if (lo_ts <= hi_ts && bl >= 0 && bh < int64_t(nbuckets) && bh - bl + 2 <= int64_t(CLU_SPLIT_MAX))
      return CluClass{CLU_SPLIT, bl, uint32_t(bh - bl + 2)};
  }
  return CluClass{CLU_UNTAKEN, 0, 0u};
}

// The host's rule for a whole segment: every tile has a copy and sorted timestamps, and the widest tile's
// ts_max - ts_min is below two steps.  Such a range meets at most three buckets, so every tile that meets a window
// lying inside the call's bucket space [base, base + nbuckets * step) is pinned or split (split tiles allowed).
inline bool clu_segment_taken(bool all_copies_sorted, int64_t widest, int64_t step) {
  return all_copies_sorted && step > 0 && widest >= 0 && widest < 2 * step;
}

}  // namespace lk
