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

// A tile's sub-block area (a second area per segment, beside the blocks: nothing inside a block moves).  The tile is
// cut into sub-blocks of CLU_SUB_ROWS rows; per chunk-dictionary code c (indexed like cagg):
//   sagg : at 0, CLU_SUB_MAX CluAgg per code: code c's elements of sub-block j reduced with clu_reduce_pinned
//          (32-B entries from a 128-B-aligned start: none straddles a 128-B line)
//   csub : at clu_sub_csub_off, CLU_SUB_MAX + 1 uint32 per code: the element index, within the tile, of code c's first
//          element whose row is >= CLU_SUB_ROWS * j (entries past the tile's sub-blocks repeat cpref[c + 1])
//   snan : at clu_sub_nan_off, one uint16 per code: bit j = a NaN among code c's elements of sub-block j
// A segment's tiles lie at a fixed stride, clu_sub_bytes of the segment's largest dict_n; a tile's offsets use its own.
constexpr uint32_t CLU_SUB_ROWS = 4096;
constexpr uint32_t CLU_SUB_MAX = TILE_ROWS / CLU_SUB_ROWS;   // 16
constexpr uint32_t CLU_SUB_STRADDLE = ~0u;
LK_BK_HD inline uint32_t clu_nsub(uint32_t nrows) { return (nrows + CLU_SUB_ROWS - 1u) / CLU_SUB_ROWS; }
LK_BK_HD inline uint32_t clu_sub_sagg_off(uint32_t c, uint32_t j) { return (c * CLU_SUB_MAX + j) * uint32_t(sizeof(CluAgg)); }
LK_BK_HD inline uint32_t clu_sub_csub_off(uint32_t dict_n) { return clu_dict_n(dict_n) * CLU_SUB_MAX * uint32_t(sizeof(CluAgg)); }
LK_BK_HD inline uint32_t clu_sub_nan_off(uint32_t dict_n) { return clu_sub_csub_off(dict_n) + clu_dict_n(dict_n) * (CLU_SUB_MAX + 1u) * 4u; }
LK_BK_HD inline uint32_t clu_sub_bytes(uint32_t dict_n) {
  const uint32_t b = clu_sub_nan_off(dict_n) + clu_dict_n(dict_n) * 2u;
  return (b + (CLU_BLOCK_ALIGN - 1u)) / CLU_BLOCK_ALIGN * CLU_BLOCK_ALIGN;
}

// A tile's timestamp sample table: CLU_SAMP_N raw 8-B timestamps, entry s the one of row clu_samp_row(s, nrows) -- the
// rows the first round of scan_clu's boundary search samples, 2 KB apart in a full tile's timestamp stream and here 16
// consecutive 128-B lines a wave loads in four coalesced rounds beside its filter chain.  A property of the segment's
// timestamp column (every tile sorted, PLAIN64), not of the copy: the tables form an area of their own, tile t's at
// clu_samp_tile_off(t), allocated in front of the sub-block area where the segment has one, so scan_clu finds it
// QSeg::clu_samp_back bytes below QSeg::clu_sub (0: the segment has no tables and the search samples the column).
constexpr uint32_t CLU_SAMP_N = 256;
constexpr uint32_t CLU_SAMP_BYTES = CLU_SAMP_N * 8u;   // a multiple of CLU_BLOCK_ALIGN
LK_BK_HD inline uint32_t clu_samp_row(uint32_t s, uint32_t nrows) { return uint32_t((uint64_t(s) * nrows) >> 8); }   // s = 256: nrows
LK_BK_HD inline uint64_t clu_samp_tile_off(uint32_t t) { return uint64_t(t) * CLU_SAMP_BYTES; }

// Sub-block j of a split tile of nrows rows, rows [lo, hi) = [CLU_SUB_ROWS * j, min(CLU_SUB_ROWS * (j + 1), nrows)),
// against the tile's boundary rows sb[0 .. nsb) (ascending; sb[k] is the first row of class k + 1): the sub-block is
// whole when no boundary lies strictly inside (lo, hi) -- one exactly on its first row leaves it whole -- and then
// every row has the class returned, the number of boundaries at or below lo.  CLU_SUB_STRADDLE: its rows' classes
// differ, so its elements are streamed.
LK_BK_HD inline uint32_t clu_sub_class(uint32_t j, uint32_t nrows, const uint32_t* sb, uint32_t nsb) {
  const uint32_t lo = j * CLU_SUB_ROWS, hi = lo + CLU_SUB_ROWS < nrows ? lo + CLU_SUB_ROWS : nrows;
  uint32_t c = 0u;
  bool whole = true;
  for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++) {
    if (k >= nsb) continue;
    c += sb[k] <= lo ? 1u : 0u;
    whole = whole && !(sb[k] > lo && sb[k] < hi);
  }
  return whole ? c : CLU_SUB_STRADDLE;
}

// COUNT over a split tile (scan_clu<AGG_COUNT>, clu_kernel.hpp) needs no value: the per-class counts of one code, stated
// here once and pinned on the CPU (tests/test_clu_count_cpu.py through clu_sim.cpp, lk_clu_count_sim).
//
// A row's class: the number of boundary rows at or below it.  sb holds CLU_SPLIT_MAX entries, those past the tile's
// nsb boundaries set to ~0 (no row reaches them).
LK_BK_HD inline uint32_t clu_split_class(uint32_t r, const uint32_t* sb) {
  uint32_t c = 0u;
  for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++) c += r >= sb[k] ? 1u : 0u;
  return c;
}
// A code's elements [a, b) of one sub-block (two neighbouring csub entries) clamped to the code's range [s, e) of the
// tile, as cpref is clamped to the tile's rows: s <= a <= b <= e afterwards.
LK_BK_HD inline void clu_sub_clamp(uint32_t& a, uint32_t& b, uint32_t s, uint32_t e) {
  b = b < e ? b : e;
  b = b > s ? b : s;
  a = a > s ? a : s;
  a = a < b ? a : b;
}
// One code of a split tile of nrows rows: its elements [s, e) of the tile, rows[i] the row within the tile of element
// s + i (ascending: crows + s), csub[0 .. clu_nsub(nrows)] its entries of the sub-block area (element indices within
// the tile; read only when use_sub), the boundary rows sb[0 .. nsb).  cnt[0 .. CLU_SPLIT_MAX] += the elements of each
// class (scan_clu merges the in-window classes 1 .. nsb - 1 and drops class 0 and class nsb).  With the area a whole
// sub-block (clu_sub_class) adds b - a to its class without looking at a row, the elements of a straddling one are
// classed one by one; without it every element is.  scan_clu<AGG_COUNT> mirrors this line for line: lane j is the
// iteration j of the sub-block loop, the element loops are spread over the wave's lanes.
LK_BK_HD inline void clu_count_split(const uint16_t* rows, uint32_t s, uint32_t e, const uint32_t* csub, uint32_t nrows,
                                     const uint32_t* sb, uint32_t nsb, bool use_sub, uint32_t* cnt) {
  uint32_t sbp[CLU_SPLIT_MAX];
  for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++) sbp[k] = k < nsb ? sb[k] : 0xffffffffu;
  if (s >= e) return;
  if (!use_sub) {
    for (uint32_t i = s; i < e; i++) cnt[clu_split_class(uint32_t(rows[i - s]), sbp)] += 1u;
    return;
  }
  const uint32_t nsub = clu_nsub(nrows);
  for (uint32_t j = 0; j < nsub; j++) {
    uint32_t a = csub[j], b = csub[j + 1u];
    clu_sub_clamp(a, b, s, e);
    if (a >= b) continue;
    const uint32_t subc = clu_sub_class(j, nrows, sbp, nsb);
    if (subc != CLU_SUB_STRADDLE) {
      cnt[subc] += b - a;
      continue;
    }
    for (uint32_t i = a; i < b; i++) cnt[clu_split_class(uint32_t(rows[i - s]), sbp)] += 1u;
  }
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
