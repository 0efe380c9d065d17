// Query evaluation: PushDownRequest -> plan (eval_plan.cpp) -> scan kernel -> (RCCL merge) -> finalize -> rows
// (labelled in eval_rows.cpp).
//
// Semantics (the globs' and buckets' in eval_plan.cpp): sum/min/max/count ignore NULL values, a
// group whose values are all NULL reads back 0.0 (Commons.scala:427); tags drop NULL/"null"/"" (Commons.scala:433) and
// fall back to the glob head's queryTags (450-452).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "comm.hpp"
#include "ddsketch.hpp"
#include "engine.hpp"
#include "eval_plan.hpp"
#include "evalutil.hpp"
#include "hll.hpp"
#include "hostutil.hpp"
#include "kernels.hpp"
#include "layout.hpp"
#include "plan.hpp"

namespace lk {

namespace {
// Large dense results cross the host link without their timestamp column: finalize_write records the first row of
// every bucket (FParams::bucket_pos) and the timestamps are expanded here, rows being in bucket-major order.
constexpr unsigned long long kTsRunsMinKeys = 1ull << 18;   // output key spaces this large (C5: 10M keys)
constexpr uint64_t kTsRunsMaxBuckets = 1u << 16;            // bucket_pos entries (mapped pinned memory)

void expand_ts_runs(Engine& E, int64_t* ts, size_t nrows, const FParams& F) {
  if (!nrows) return;
  const uint32_t* bp = F.bucket_pos;
  const uint64_t nb = F.nbuckets;
  const size_t piece = size_t(1) << 19;
  const size_t npieces = (nrows + piece - 1) / piece;
  E.host_parallel(npieces, [&](size_t p) {
    const size_t lo = p * piece, hi = std::min(nrows, lo + piece);
    // the bucket of row lo: the last bucket starting at or before it
    uint64_t b = uint64_t(std::upper_bound(bp, bp + nb, uint32_t(lo)) - bp);
    b = b ? b - 1 : 0;
    for (size_t r = lo; r < hi;) {
      const size_t end = std::min<size_t>(hi, b + 1 < nb ? bp[b + 1] : nrows);
      const int64_t t = F.bucket_base + int64_t(b) * F.step;
      for (; r < end; r++) ts[r] = t;
      b++;
    }
  });
}

// Rows of a large result from its output keys' existence bits (FParams::key_bits): rows are the existing keys in key
// order, so row r's key -- and from it the timestamp, group id and glob -- follow from the bits alone.  Pieces of 2^20
// keys: counts, a prefix, then every piece expanded on its own thread.
void expand_rows_from_keys(Engine& E, int64_t* ts, uint32_t* gid, uint32_t* glob, const unsigned long long* bits,
                           const FParams& F, bool per_glob) {
  const uint64_t words = (F.nkeys + 63) / 64;
  constexpr uint64_t kPiece = uint64_t(1) << 14;   // words per piece
  const size_t np = size_t((words + kPiece - 1) / kPiece);
  std::vector<size_t> base(np + 1, 0);
  E.host_parallel(np, [&](size_t p) {
    size_t c = 0;
    for (uint64_t w = p * kPiece; w < std::min(words, (p + 1) * kPiece); w++) c += size_t(__builtin_popcountll(bits[w]));
    base[p + 1] = c;
  });
  for (size_t p = 0; p < np; p++) base[p + 1] += base[p];
  const uint64_t ng = F.ngroups, ns = F.nglob_slots ? F.nglob_slots : 1;
  E.host_parallel(np, [&](size_t p) {
    size_t r = base[p];
    for (uint64_t w = p * kPiece; w < std::min(words, (p + 1) * kPiece); w++) {
      unsigned long long x = bits[w];
      if (!x) continue;
      const uint64_t k0 = w * 64;
      uint64_t t0 = k0 / ng, g0 = k0 - t0 * ng;   // key = t * ngroups + g
      while (x) {
        const uint64_t b = uint64_t(__builtin_ctzll(x));
        x &= x - 1;
        uint64_t g = g0 + b, t = t0;
        if (g >= ng) {
          t += g / ng;
          g %= ng;
        }
        const uint64_t bucket = per_glob ? t / ns : t;
        ts[r] = F.bucket_base + int64_t(bucket) * F.step;
        gid[r] = uint32_t(g);
        if (glob) glob[r] = uint32_t(t % ns);
        r++;
      }
    }
  });
}
}  // namespace

namespace {
// Percentiles: one DDSketch per (glob, step, group-key tags) -- the groupBys' values, or {"_cardinalhq.name": ""}
// without groupBys (PushDownAggregatorStage.getGroupByKeyTags, 188-197: see sketch_rows); NULL / "null" / "" values drop
// out of the tags (Commons.scala:433).  Merged: per (step, tags).
struct SkRow {
  int64_t ts;
  uint32_t glob;
  unsigned long long gid;
  dd::Sketch sk;
};
struct CesRow {
  int64_t ts;
  uint32_t glob;
  hll::Sketch h;
};

// The device half's state: what the upload, scan, reduce and finalize functions share and change.
struct DevState {
  QParams P{};
  hipStream_t st = nullptr;
  int kagg = 0;                   // the kernels' aggregate (avg scans as sum, rows / sketch / ces as count)
  float scan_ms = 0;
  double plan_ms = 0, launch_ms = 0, scan_agreed_ms = 0, reduce_ms = 0, sync_ms = 0, alloc_ms = 0, copy_ms = 0;
  // staging: one pinned buffer + one device workspace, offsets into both
  uint8_t* hbuf = nullptr;
  uint8_t* dbuf = nullptr;
  size_t o_gsegs = 0, o_truth_x = 0, o_rank = 0, o_fval = 0, o_fok = 0, o_tail = 0, o_bpos = 0, o_kbits = 0;
  std::vector<size_t> map_off;    // per column: its fold map's offset in d_maps (SIZE_MAX: none)
  const uint32_t* d_maps = nullptr;
  bool ftext_tab = false, ts_runs_ok = false, key_rows_ok = false;
  uint64_t okeys = 0, out_keys = 0;
  bool keep_dev = false, fast_final = false, dense_shape = false;
  uint32_t fexist = 0;
  int local_err = 0;              // distributed: a rank-local failure, agreed on with the other ranks after the scan
  std::string local_msg;
  // scan
  uint64_t cap = 0;               // hash table slots (grown by the scan loop)
  size_t nc = 0;                  // table cells
  bool fast_done = false;         // rows already written by the speculative finalize
  uint32_t fast_rows = 0;
  unsigned long long plan_bytes = 0;
  uint32_t clu_tiles = 0;         // tiles scan_clu took (counted with the plan bytes: flags[1])
  uint32_t hflags = 0;
  int attempts = 0;
  // multi-GPU reduce
  bool keyrange = false;
  int W = 1;
  std::vector<uint64_t> kb;       // key-range bounds: rank j owns cells [kb[j], kb[j+1])
  size_t kr_len = 0;
  uint32_t nrows_out = 0;
  bool rows_done = false;         // key-range path: rank 0's result rows are already in place
  const char* emit_mode = "local";
  bool emit = false;
  // finalize
  FParams F{};
  SParams S{};
  uint32_t nfb = 0;
  uint32_t* d_counts = nullptr;
  void* sws = nullptr;
  unsigned long long nocc = 0;
  std::vector<SkRow> sk_rows;
  std::vector<CesRow> ces_rows;
};

// The table's planes as finalize / sparse parameters read them.
template <class T, class Table>
void bind_table(T& t, const Table& P) { t.rows = P.rows, t.cnt = P.cnt, t.hi = P.hi, t.lo = P.lo, t.ext = P.ext; }

// ---- device: upload ----
void stage_upload(const EvalCall& C, const Plan& pl, DevState& dv) {
  dv.plan_ms = ms_since(C.t_start);
  dv.st = C.X.stream;
  dv.cap = pl.cs.cap;
  dv.local_err = pl.sg.local_err;
  dv.local_msg = pl.sg.local_msg;
  dv.P.nsegs = uint32_t(pl.sg.qsegs.size());
  dv.P.total_tiles = pl.sg.total_tiles;
  dv.P.max_tiles = pl.sg.max_tiles;
  dv.P.fast_div = (pl.gp.step > 0 && pl.gp.step < (int64_t(1) << 31) && pl.cs.nbuckets &&
                pl.cs.max_hi - pl.cs.bucket_base < (int64_t(1) << 32)) ? 1 : 0;
  dv.P.inv_step = 1.0 / double(pl.gp.step > 0 ? pl.gp.step : 1);
  dv.P.nstr = uint32_t(pl.fp.cols.size());
  dv.P.nleaves = uint32_t(pl.fp.leaves.size());
  dv.P.nprog = uint32_t(pl.fp.prog.size());
  dv.P.metrics = pl.qs.metrics ? 1 : 0;
  dv.P.step = pl.gp.step > 0 ? pl.gp.step : 1;
  dv.P.bucket_base = pl.cs.bucket_base;
  dv.P.nbuckets = pl.cs.nbuckets;
  dv.P.ngroups = pl.dp.ngroups;
  dv.P.ncells = pl.cs.ncells;
  std::vector<StrParam> strp(pl.fp.cols.size());
  for (size_t s = 0; s < pl.fp.cols.size(); s++) {
    StrParam& sp = strp[size_t(pl.fp.dev_of[s])];   // device order (query column 2 + dev_of[s])
    sp.dim_null = pl.dp.dims[s].dim_null;
    sp.dim_stride = pl.dp.dims[s].is_dim ? uint32_t(pl.dp.dims[s].stride) : 0u;
    sp.lbase = pl.fp.cols[s].lbase;
    sp.lmask = pl.fp.cols[s].lmask;
    sp.hmask = pl.fp.cols[s].hmask;
  }
  memcpy(dv.P.prog, pl.fp.prog.data(), pl.fp.prog.size());
  if (const char* ab = getenv("LK_ABLATE")) dv.P.ablate = uint32_t(atoi(ab));   // diagnostics only

  // staging layout in one pinned buffer + one device workspace
  size_t off = 0;
  auto reserve = [&](size_t n) { size_t o = (off + 255) / 256 * 256; off = o + n; return o; };
  const size_t o_segs = reserve(pl.sg.qsegs.size() * sizeof(QSeg));
  dv.o_gsegs = reserve(pl.sg.gsegs.size() * sizeof(QSeg));
  const size_t o_truth = reserve(pl.fp.truth.size() * 4);
  dv.o_truth_x = reserve(pl.fp.truth_x.size() * 4);
  const size_t o_truth_e = reserve(pl.fp.truth_early.size() * 4);
  const size_t o_truth_l = reserve(pl.fp.truth_late.size() * 4);
  std::vector<size_t> o_tab(pl.fp.cols.size());
  for (size_t s = 0; s < pl.fp.cols.size(); s++) o_tab[s] = pl.dp.need_tab[s] ? reserve(pl.dp.tabs[s].size() * 4) : 0;
  const size_t o_flags = reserve(sizeof(uint32_t) * 4);
  const size_t o_strp = reserve(strp.size() * sizeof(StrParam));
  dv.o_rank = reserve(pl.dp.name_rank.size() * 4);
  // null-like group values folded after per-glob aggregation (merged min/max over NULL-able values)
  std::vector<uint32_t> flat;
  dv.map_off.assign(pl.dp.dims.size(), SIZE_MAX);
  if (pl.cs.rekey)
    for (size_t s = 0; s < pl.dp.dims.size(); s++)
      if (!pl.cs.fold_maps[s].empty()) {
        dv.map_off[s] = flat.size();
        flat.insert(flat.end(), pl.cs.fold_maps[s].begin(), pl.cs.fold_maps[s].end());
      }
  const size_t o_maps = reserve(flat.size() * 4);
  // field chart over a VARCHAR field: per dictionary id the double and a validity bit (XParams::ftab / fok)
  dv.ftext_tab = pl.gp.ftext_any && pl.gp.ftab;
  dv.o_fval = reserve(dv.ftext_tab ? size_t(pl.gp.ftab_n) * 8 : 0);
  dv.o_fok = reserve(dv.ftext_tab ? (size_t(pl.gp.ftab_n) + 31) / 32 * 4 : 0);
  const size_t stage_bytes = off;
  dv.o_tail = reserve(64);   // host side only: the small-table epilogue's flags and row count (mapped)
  // host side only (mapped): the first row of every bucket, when a large result's timestamps are expanded on the host
  dv.ts_runs_ok = pl.cs.nbuckets <= kTsRunsMaxBuckets && !getenv("LK_NO_TS_RUNS");
  dv.o_bpos = reserve(dv.ts_runs_ok ? (size_t(pl.cs.nbuckets) + 1) * 4 : 0);
  // host side only (mapped): the existence bit of every output key of a large grouped result (FParams::key_bits)
  dv.okeys = pl.qs.per_glob_rows ? pl.cs.ncells : (pl.cs.collapse ? pl.cs.nbuckets : pl.cs.nbuckets * pl.dp.ngroups);
  // default since r06 (LK_NO_KEY_ROWS=1 for A/B): with the row expansion on the job's whole thread share it runs while
  // the values cross the host link -- C5 eval 2.64 -> 1.93 ms (profiles/r06_ab_c5_*); r05's 8-thread expansion measured
  // slower (2.28 vs 2.13 ms)
  dv.key_rows_ok = !pl.cs.collapse && dv.okeys >= kTsRunsMinKeys && !getenv("LK_NO_KEY_ROWS");
  dv.o_kbits = reserve(dv.key_rows_ok ? size_t((dv.okeys + 2047) / 2048) * 2048 / 8 : 0);
  // staging buffers: a rank-local failure here is agreed on after the scan stage (no scan runs on this rank)
  try {
    HIP_TRY(hipSetDevice(C.E.device));
    dv.hbuf = static_cast<uint8_t*>(C.X.pinned_buf(off + 64));
    dv.dbuf = static_cast<uint8_t*>(C.X.workspace("query", stage_bytes));
  } catch (const PlanError& e) {
    if (!C.dist) throw;
    if (!dv.local_err) {
      dv.local_err = e.code;
      dv.local_msg = e.what();
    }
  }
  if (dv.hbuf && dv.dbuf) {
  memcpy(dv.hbuf + o_segs, pl.sg.qsegs.data(), pl.sg.qsegs.size() * sizeof(QSeg));
  memcpy(dv.hbuf + dv.o_gsegs, pl.sg.gsegs.data(), pl.sg.gsegs.size() * sizeof(QSeg));
  if (!pl.fp.truth.empty()) memcpy(dv.hbuf + o_truth, pl.fp.truth.data(), pl.fp.truth.size() * 4);
  if (!pl.fp.truth_x.empty()) memcpy(dv.hbuf + dv.o_truth_x, pl.fp.truth_x.data(), pl.fp.truth_x.size() * 4);
  if (pl.fp.late_mask) {
    memcpy(dv.hbuf + o_truth_e, pl.fp.truth_early.data(), pl.fp.truth_early.size() * 4);
    memcpy(dv.hbuf + o_truth_l, pl.fp.truth_late.data(), pl.fp.truth_late.size() * 4);
  }
  for (size_t s = 0; s < pl.fp.cols.size(); s++)
    if (pl.dp.need_tab[s]) {
      memcpy(dv.hbuf + o_tab[s], pl.dp.tabs[s].data(), pl.dp.tabs[s].size() * 4);
      strp[size_t(pl.fp.dev_of[s])].strtab = reinterpret_cast<const uint32_t*>(dv.dbuf + o_tab[s]);
    } else if (pl.dp.dims[s].exchanged) {
      strp[size_t(pl.fp.dev_of[s])].strtab = pl.dp.dims[s].uni->d_dim_of_gid;   // resident (dims.cpp)
    }
  memcpy(dv.hbuf + o_strp, strp.data(), strp.size() * sizeof(StrParam));
  memset(dv.hbuf + o_flags, 0, 16);
  if (!pl.dp.name_rank.empty()) memcpy(dv.hbuf + dv.o_rank, pl.dp.name_rank.data(), pl.dp.name_rank.size() * 4);
  if (!flat.empty()) memcpy(dv.hbuf + o_maps, flat.data(), flat.size() * 4);
  if (dv.ftext_tab && pl.gp.ftab_n) {
    memcpy(dv.hbuf + dv.o_fval, pl.gp.ftab->val.data(), size_t(pl.gp.ftab_n) * 8);
    uint32_t* ok = reinterpret_cast<uint32_t*>(dv.hbuf + dv.o_fok);
    memset(ok, 0, (size_t(pl.gp.ftab_n) + 31) / 32 * 4);
    for (uint32_t id = 0; id < pl.gp.ftab_n; id++)
      if (pl.gp.ftab->cls[id] == 1) ok[id >> 5] |= 1u << (id & 31u);
  }
  const hipError_t up = hipMemcpyAsync(dv.dbuf, dv.hbuf, stage_bytes, hipMemcpyHostToDevice, dv.st);
  if (up != hipSuccess) {
    (void)hipGetLastError();
    if (!C.dist) throw PlanError(LK_ERR_DEVICE, std::string("HIP: query upload: ") + hipGetErrorString(up));
    if (!dv.local_err) {
      dv.local_err = LK_ERR_DEVICE;
      dv.local_msg = std::string("HIP: query upload: ") + hipGetErrorString(up);
    }
  }
  }
  dv.P.segs = reinterpret_cast<const QSeg*>(dv.dbuf + o_segs);
  dv.P.flags = reinterpret_cast<uint32_t*>(dv.dbuf + o_flags);
  dv.P.truth = pl.fp.truth.empty() ? nullptr : reinterpret_cast<const uint32_t*>(dv.dbuf + o_truth);
  dv.P.late_mask = getenv("LK_NO_LATE") ? 0u : pl.fp.late_mask;   // env: diagnostics only (A/B of the late path)
  dv.P.truth_early = pl.fp.late_mask ? reinterpret_cast<const uint32_t*>(dv.dbuf + o_truth_e) : nullptr;
  dv.P.truth_late = pl.fp.late_mask ? reinterpret_cast<const uint32_t*>(dv.dbuf + o_truth_l) : nullptr;
  dv.P.strp = reinterpret_cast<const StrParam*>(dv.dbuf + o_strp);
  dv.d_maps = reinterpret_cast<const uint32_t*>(dv.dbuf + o_maps);
}

void setup_scan(const EvalCall& C, const Plan& pl, DevState& dv) {
  dv.kagg = pl.qs.agg == AGG_AVG ? AGG_SUM : ((pl.qs.agg == AGG_ROWS || pl.qs.agg == AGG_SKETCH || pl.qs.agg == AGG_CES) ? AGG_COUNT : pl.qs.agg);
  // lean tables: no NULL value anywhere in the value column -> cnt == rows; min/max also imply rows
  if (!pl.gp.value_nulls && !pl.qs.no_value_col && !getenv("LK_NO_LEAN"))
    dv.P.lean = (dv.kagg == AGG_MIN || dv.kagg == AGG_MAX) ? LEAN_NO_ROWS : LEAN_NO_CNT;
  // dense SUM (not AVG, which needs the row counts): existence from the -0.0 marker, no rows atomics at all
  if (dv.P.lean == LEAN_NO_CNT && pl.qs.agg == AGG_SUM && !pl.cs.hash_mode && !pl.qs.sketch && !pl.qs.ces && !getenv("LK_NO_SUM_EXISTS"))
    dv.P.lean |= LEAN_SUM_EXISTS;
  // single string column (filter and group dim on `name` only), or name early with every other string column late
  // (<= 2 of them): NULL-free tiles with a small name dictionary go to scan_lean (lean_kernel.hpp), the rest to
  // scan_tiles
  const bool lean_shape = dv.P.nstr == 1 || (dv.P.nstr <= 3 && dv.P.late_mask == ((1u << dv.P.nstr) - 2u));
  dv.P.rows_only = pl.qs.no_value_col ? 1u : 0u;   // COUNT(*) / metrics ces: no value column is bound (lean tiles need none)
  // late columns decoded per chunk (scan_lean<..., EARLY>) where a late filter leaf exists: the late filter then runs
  // before the rows are listed, and a listed row waits only on its value.  Opt-in (LK_LATE_CHUNK=1): measured slower
  // than the per-row late stage on C3 (3.47 vs 1.97 ms) and the tag query (2.28 vs 1.06 ms) -- every chunk pays a
  // run search and a window load per late column before its filter outcome is known
  {
    bool late_leaves = false;
    for (size_t s = 0; s < pl.fp.cols.size(); s++)
      if (((pl.fp.late_mask >> pl.fp.dev_of[s]) & 1u) && !pl.fp.cols[s].leaves.empty()) late_leaves = true;
    dv.P.late_chunk = (late_leaves && pl.dp.ngroups <= 65536u && getenv("LK_LATE_CHUNK")) ? 1u : 0u;
    // one string column whose eq / in filter passes a quarter or more of its values (the dense query): the 5-wave
    // per-lane scan_lean<..., 0, EARLY> -- its dense-code tiles lose ~0.3 ms in C2's 4-wave listed shape
    // (LK_NO_DENSE_SHAPE=1: A/B).  Against the dictionary's live ids (values some cached segment references), not
    // its size, which also counts ids evicted segments left behind; the pick is in stats.lean_dense_shape.
    if (dv.P.nstr == 1 && !pl.dp.dims[0].cand.empty() && !getenv("LK_NO_DENSE_SHAPE")) {
      GlobalDict& gd = C.E.dict(pl.fp.cols[0].name);
      size_t nv = 0;
      {
        std::lock_guard<std::mutex> g(gd.mu);
        nv = gd.live;
      }
      if (pl.dp.dims[0].cand.size() * 4 >= nv) {
        dv.P.late_chunk = 1u;
        dv.dense_shape = true;
      }
    }
  }
  dv.P.lean_split = (lean_shape && dv.P.truth && (pl.qs.agg != AGG_ROWS || pl.qs.tagq) && !pl.qs.sketch && (!pl.qs.numeric || pl.fp.vleaf) && !getenv("LK_NO_LEAN_SPLIT"))
                    ? (pl.sg.all_lean ? 2u : 1u) : 0u;
  if (pl.qs.numeric && !(pl.fp.vleaf && pl.sg.gsegs.empty())) dv.P.lean = 0;   // the general row scan accumulates every table field
  if (dv.P.lean && getenv("LK_NO_DENSE_DIRECT")) dv.P.lean |= LEAN_NO_DENSE_DIRECT;   // env: A/B only
  // exact integer sums: every partial sum of <= vals_rows integers of magnitude <= vals_abs_max is <= 2^52 (a margin for
  // the FLOAT cast of union_by_name integer columns), so it is
  // exact in any order and the compensated sum equals the plain one bit for bit (LK_NO_EXACT_SUM=1: A/B)
  dv.P.exact_sum = (dv.kagg == AGG_SUM && !pl.qs.sketch && !pl.qs.ces && pl.sg.vals_integral && pl.sg.vals_abs_max * pl.sg.vals_rows <= 4503599627370496.0 &&
                 !getenv("LK_NO_EXACT_SUM")) ? 1u : 0u;
  // a group space far beyond scan_lean's LDS hash table (1M+ cells): register cells go straight to the global table
  dv.P.global_cells = (uint64_t(pl.dp.ngroups) * pl.cs.nbuckets >= (1ull << 20) && !getenv("LK_LDS_CELLS")) ? 1u : 0u;
  dv.P.split_ok = getenv("LK_NO_SPLIT") ? 0u : 1u;   // env: A/B only
  // LK_NO_CLU_AGG=1 (read per call: A/B and the tests' proof of the path): scan_clu streams its pinned tiles
  if (dv.P.split_ok && getenv("LK_NO_CLU_AGG")) dv.P.split_ok |= SPLIT_OK_NO_CLU_AGG;
  // LK_NO_CLU_SUB=1 (read per call, independent of the above): scan_clu streams its split tiles' ranges whole
  if (dv.P.split_ok && getenv("LK_NO_CLU_SUB")) dv.P.split_ok |= SPLIT_OK_NO_CLU_SUB;
  // LK_NO_CLU_SAMP=1 (read per call, independent of the above): scan_clu's boundary search samples the timestamp column
  // instead of loading the tile's sample table
  if (dv.P.split_ok && getenv("LK_NO_CLU_SAMP")) dv.P.split_ok |= SPLIT_OK_NO_CLU_SAMP;
  // scan_lean (and, in COUNT / p<NN> / ces calls, scan_tiles) tests the value leaves of every row its string conjuncts pass
  if (pl.fp.vleaf && !pl.sg.qsegs.empty()) {
    dv.P.nvl = uint32_t(pl.fp.nleaves.size());
    dv.P.vtab = pl.fp.vtab;
    for (size_t k = 0; k < pl.fp.nleaves.size(); k++) {
      const NumLeaf& nl = pl.fp.nleaves[k];
      dv.P.vl[k] = vleaf_of(nl);
    }
  }
  // scan_lean: a dense table whose group space fits LDS for the few buckets a tile spans is aggregated in the tile's
  // direct table (lean_kernel.hpp) instead of the LDS hash table: dir_span = the most buckets it holds
  if (dv.P.lean_split && !pl.cs.hash_mode && !getenv("LK_NO_DIRECT")) {
    const uint64_t words = lean_dir_words(dv.P.nstr - 1);
    const bool rows_plane = dv.kagg != AGG_COUNT && !(dv.P.lean & (LEAN_SUM_EXISTS | LEAN_NO_ROWS));
    const uint32_t cw = (dv.kagg == AGG_SUM ? 2u : 1u) + (rows_plane ? 1u : 0u);
    // the most replicas per cell (spreading lanes that add into the same cells over more LDS addresses) that still
    // leave room for a tile spanning two buckets
    const uint32_t rep_max = getenv("LK_DIRECT_REPMAX") ? uint32_t(atoi(getenv("LK_DIRECT_REPMAX"))) : 4u;   // env: A/B
    for (uint32_t rep = rep_max >= 64 ? 64u : rep_max >= 16 ? 16u : rep_max >= 8 ? 8u : 4u; rep >= 1; rep /= 2) {
      const uint64_t w = std::min<uint64_t>(LEAN_DIR_MAXSPAN, words / (uint64_t(cw) * rep * std::max<uint64_t>(pl.dp.ngroups, 1)));
      if (w >= 2 || (rep == 1 && w >= 1)) {
        dv.P.dir_span = uint32_t(w);
        dv.P.dir_planes = cw;
        dv.P.dir_rep = getenv("LK_DIRECT_REP1") ? 1u : rep;   // env: A/B only
        if (dv.P.dir_rep == 1u && rep != 1u)
          dv.P.dir_span = uint32_t(std::min<uint64_t>(LEAN_DIR_MAXSPAN, words / (uint64_t(cw) * std::max<uint64_t>(pl.dp.ngroups, 1))));
        break;
      }
    }
  }
  if (pl.qs.sketch) {
    dv.P.sketch = 1;
    dv.P.dd_mult = dd::mapping().multiplier;
    dv.P.dd_min = dd::mapping().min_indexable;
    dv.P.dd_max = dd::mapping().max_indexable;
  }

  // Single-GPU dense tables with a bounded output: the finalize is enqueued right behind the scan -- rows written by
  // the kernel into the (pinned) result block sized for every output key -- so the flags, the row count and the rows
  // come back with one stream synchronization instead of three (scan flags, row count, rows).  A re-run (metrics off
  // the step grid, MIN over NaN) discards the speculative rows.
  dv.out_keys = pl.cs.ncells == 0 ? 0 : (pl.qs.per_glob_rows ? pl.cs.ncells : (pl.cs.collapse ? pl.cs.nbuckets : pl.cs.nbuckets * pl.dp.ngroups));
  dv.keep_dev = (C.flags & kEvalKeepDevice) != 0;
  if (dv.keep_dev && (pl.qs.per_glob_rows || pl.qs.sketch || pl.qs.ces || pl.qs.tagq))
    throw PlanError(LK_ERR_DEVICE, "internal: rows kept on the device are merged aggregate rows");
  dv.fast_final = !dv.keep_dev && !C.dist && !pl.cs.hash_mode && !pl.qs.sketch && !pl.qs.ces && !pl.cs.rekey && pl.cs.ncells && dv.out_keys <= (uint64_t(1) << 20) &&
                          !getenv("LK_NO_FAST_FINAL");
  // field charts: `<field> IS NOT NULL` drops a row, so a cell exists iff a row with a field reached it.  The row
  // scan applies the conjunct per row (rows != 0 says so); the fused kernels count every passing row, and a numeric
  // field's rows with a field are its cnt -- a call with a VARCHAR glob runs on the row scan alone (plan_segments)
  dv.fexist = (pl.qs.fchart && !pl.gp.ftext_any) ? 1u : 0u;
  // Multi-GPU reduce shape (decided before the scan: its receive buffers are placed before the scan's agreement
  // point, so no rank can fail alone between that agreement and the first point-to-point transfer).
  const char* kr_env = getenv("LK_KEYRANGE_MIN_CELLS");
  const uint64_t kr_min = kr_env ? uint64_t(atoll(kr_env)) : (uint64_t(1) << 20);
  dv.keyrange = C.dist && (comm_world(C.E) > 1 || comm_loopback(C.E)) && !pl.cs.hash_mode && !pl.qs.per_glob_rows && !pl.cs.collapse && !pl.cs.rekey && !pl.qs.sketch &&
                        !pl.qs.ces && pl.cs.nslots == 1 && pl.cs.ncells >= std::max<uint64_t>(kr_min, 1);
  dv.W = C.dist ? comm_world(C.E) : 1;
  dv.kb.resize(size_t(dv.W) + 1);   // key-range bounds: rank j owns cells [kb[j], kb[j+1])
  for (int j = 0; j <= dv.W; j++) dv.kb[size_t(j)] = j == dv.W ? pl.cs.ncells : (pl.cs.ncells * uint64_t(j) / uint64_t(dv.W)) & ~63ull;
  dv.kr_len = size_t(dv.kb[size_t(pl.gp.rank) + 1] - dv.kb[size_t(pl.gp.rank)]);
}

void setup_final(const Plan& pl, const DevState& dv, FParams& Fp, uint32_t fslots) {
  Fp.ngroups = pl.dp.ngroups;
  Fp.nbuckets = pl.cs.nbuckets;
  Fp.nglob_slots = fslots;
  Fp.agg = pl.qs.agg;
  Fp.per_glob = pl.qs.per_glob_rows ? 1 : 0;
  Fp.collapse = pl.cs.collapse ? 1 : 0;
  Fp.name_stride = pl.dp.dims[0].stride ? pl.dp.dims[0].stride : 1;
  Fp.name_rank = pl.dp.name_rank.empty() ? nullptr : reinterpret_cast<const uint32_t*>(dv.dbuf + dv.o_rank);
  Fp.bucket_base = pl.cs.bucket_base;
  Fp.step = dv.P.step;
  Fp.nkeys = dv.out_keys;
  Fp.exist_cnt = dv.fexist;
  Fp.scale = pl.qs.fscale;
}

// Zero the table (SoA [rows | cnt | hi | lo | ext (| keys)]) and the scan flags.
void zero_table(const EvalCall& C, DevState& dv, size_t ncl, bool hashed) {
  uint8_t* tb = static_cast<uint8_t*>(C.X.workspace("table", ncl * 8 * (hashed ? 6 : 5) + 4 * 256));
  dv.P.rows = reinterpret_cast<unsigned long long*>(tb);
  dv.P.cnt = reinterpret_cast<unsigned long long*>(tb + ncl * 8);
  dv.P.hi = reinterpret_cast<double*>(tb + ncl * 16);
  dv.P.lo = reinterpret_cast<double*>(tb + ncl * 24);
  dv.P.ext = reinterpret_cast<unsigned long long*>(tb + ncl * 32);
  dv.P.hkeys = hashed ? reinterpret_cast<unsigned long long*>(tb + ncl * 40) : nullptr;
  dv.P.hmask = hashed ? ncl - 1 : 0;
  // one launch: the planes this aggregate reads, and the scan flags + plan-bytes counter (4 x u32)
  FillList F{};
  auto add = [&](void* p, size_t n, unsigned long long v) {
    F.p[F.count] = static_cast<unsigned long long*>(p);
    F.n[F.count] = n;
    F.v[F.count] = v;
    F.count++;
  };
  add(tb, ncl * 2, 0ull);                                           // rows | cnt
  if (dv.kagg == AGG_SUM) {
    add(dv.P.hi, ncl, (dv.P.lean & LEAN_SUM_EXISTS) ? NEG_ZERO_BITS : 0ull);
    add(dv.P.lo, ncl, 0ull);
  }
  if (dv.kagg == AGG_MIN) add(dv.P.ext, ncl, ~0ull);
  if (dv.kagg == AGG_MAX) add(dv.P.ext, ncl, 0ull);
  if (hashed) add(dv.P.hkeys, ncl, ~0ull);
  add(dv.P.flags, 2, 0ull);                                            // flags + the 64-bit plan-bytes counter
  HIP_TRY(launch_fill_many(F, dv.st));
}

// The general row scan's parameters over the staged query (gsegs): XMODE_AGG into dv.P's table, or the numeric group
// dimensions' discovery (XMODE_NUMDIM), which reads the same rows.
XParams general_scan_params(const Plan& pl, const DevState& dv, uint32_t mode) {
  XParams XG{};
  XG.segs = reinterpret_cast<const QSeg*>(dv.dbuf + dv.o_gsegs);
  XG.nsegs = uint32_t(pl.sg.gsegs.size());
  XG.max_tiles = pl.sg.gmax_tiles;
  XG.strp = dv.P.strp;
  XG.nstr = dv.P.nstr;
  XG.nleaves = dv.P.nleaves;
  XG.nprog = dv.P.nprog;
  memcpy(XG.prog, dv.P.prog, sizeof(XG.prog));
  XG.truth = pl.fp.truth_x.empty() ? dv.P.truth : reinterpret_cast<const uint32_t*>(dv.dbuf + dv.o_truth_x);
  XG.mode = mode;
  XG.nnum = uint32_t(pl.qs.nums.size());
  XG.nnl = uint32_t(pl.fp.nleaves.size());
  for (size_t i = 0; i < pl.fp.nleaves.size(); i++) XG.nl[i] = pl.fp.nleaves[i];
  XG.agg = dv.kagg;
  XG.hash = pl.cs.hash_mode ? 1 : 0;
  XG.q = dv.P;
  if (pl.qs.fchart) {   // `<field> IS NOT NULL` as a conjunct; a VARCHAR field's values from the staged table
    XG.field = 1;
    XG.ftab = dv.ftext_tab ? reinterpret_cast<const double*>(dv.dbuf + dv.o_fval) : nullptr;
    XG.fok = dv.ftext_tab ? reinterpret_cast<const uint32_t*>(dv.dbuf + dv.o_fok) : nullptr;
  }
  // numeric group dimensions: query column, stride and NULL id per dimension; the discovered tables
  XG.nnd = uint32_t(pl.qs.numgbs.size());
  for (size_t k = 0; k < pl.qs.numgbs.size(); k++) {
    const DimCol& dc = pl.dp.dims[pl.fp.cols.size() + k];
    const size_t n = size_t(std::find(pl.qs.nums.begin(), pl.qs.nums.end(), pl.qs.numgbs[k]) - pl.qs.nums.begin());
    XG.nd[k] = NumDim{uint32_t(2 + pl.fp.cols.size() + n), uint32_t(dc.stride), dc.dim_null, 0u};
    XG.ndmask |= 1u << XG.nd[k].qc;
  }
  XG.seg_glob = pl.dp.nd.d_seg_glob;
  XG.ndcap = pl.dp.nd.cap;
  XG.ndkeys = pl.dp.nd.d_keys;
  XG.ndids = pl.dp.nd.d_ids;
  XG.ndones = pl.dp.nd.d_ones;
  XG.ndflags = pl.dp.nd.d_flags;
  return XG;
}

// Numeric group dimensions, the discovery pass: one XMODE_NUMDIM launch over the staged query lists the
// canonical keys of every numeric group column per glob (tables regrown x8 while one overflows, as TAGNUM's); the host
// prints each (glob union type, key) as JDBC getString does, orders the distinct texts of all globs -- a dimension's
// ids depend on the set of texts alone -- and uploads the id of every slot for the aggregate scan's lookup.
// Distributed: every rank discovers over its own segments, one all-gather carries every rank's text sets with its
// status, and the sorted union over the ranks is the dimension on every rank (ids never depend on a rank, a slot or
// timing).  The rank-local steps run inside comm_local: a failure travels with the next agreement, no rank unwinds alone.
void discover_numdims(const EvalCall& C, Plan& pl, const DevState& dv) {
  const auto t0 = std::chrono::steady_clock::now();
  NumDimTables& nd = pl.dp.nd;
  const size_t nnd = pl.qs.numgbs.size(), ng = pl.gp.globs.size(), nseg = pl.sg.gsegs.size();
  const size_t first = pl.fp.cols.size();
  auto pow2 = [](uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
  };
  std::vector<unsigned long long> keys;
  std::vector<uint32_t> ones(ng * nnd, 0);
  std::vector<std::vector<std::string>> mine(nnd);   // per column: this process's distinct texts, sorted
  hipStream_t st = dv.st;
  auto text_of = [&](size_t k, size_t gi, unsigned long long key) { return numdim_key_text(pl.gp.num_ut[k][gi], key); };
  // run a rank-local step: alone it throws; distributed, its failure is kept for the next agreement
  auto local = [&](auto&& f) {
    if (C.dist) comm_local(C.X, f);
    else f();
  };
  local([&] {
    if (C.dist) fault_point(C.E, "numdim");
    if (dv.local_err) throw PlanError(dv.local_err, dv.local_msg);   // (distributed: the staging failed on this rank)
    std::vector<uint64_t> grows(ng, 0);
    for (size_t gi = 0; gi < ng; gi++)
      for (int si : pl.gp.globs[gi].segs)
        if (pl.gp.segs[si]) grows[gi] += uint64_t(pl.gp.segs[si]->num_rows);
    const uint64_t cap_max = std::max<uint64_t>(1 << 12, pow2(2 * *std::max_element(grows.begin(), grows.end())));
    uint64_t cap = std::min<uint64_t>(cap_max, pow2(env_u64("LK_NUMDIM_INIT_SLOTS", uint64_t(1) << 12, 64)));
    if (nseg && pl.cs.ncells && (!dv.hbuf || !dv.dbuf)) throw PlanError(LK_ERR_DEVICE, "internal: numeric groupBy without a staged query");
    for (;;) {
      nd.attempts++;
      const size_t nslots = ng * nnd * size_t(cap);
      // [keys | ids | all-ones words | flags | segment -> glob]
      const size_t o_ids = nslots * 8, o_ones = o_ids + nslots * 4, o_flags = o_ones + ng * nnd * 4, o_sg = o_flags + 16;
      uint8_t* tb = static_cast<uint8_t*>(C.X.workspace("numdim", o_sg + nseg * 4 + 64));
      nd.cap = cap;
      nd.d_keys = reinterpret_cast<unsigned long long*>(tb);
      nd.d_ids = reinterpret_cast<uint32_t*>(tb + o_ids);
      nd.d_ones = reinterpret_cast<uint32_t*>(tb + o_ones);
      nd.d_flags = reinterpret_cast<uint32_t*>(tb + o_flags);
      nd.d_seg_glob = reinterpret_cast<const uint32_t*>(tb + o_sg);
      HIP_TRY(hipMemsetAsync(tb, 0xff, nslots * 8, st));
      HIP_TRY(hipMemsetAsync(tb + o_ids, 0, o_sg - o_ids, st));
      if (nseg) HIP_TRY(hipMemcpyAsync(tb + o_sg, pl.sg.gseg_glob.data(), nseg * 4, hipMemcpyHostToDevice, st));
      if (pl.cs.ncells && nseg) HIP_TRY(launch_ex_scan_numdim(general_scan_params(pl, dv, XMODE_NUMDIM), st));
      uint32_t fl = 0;
      HIP_TRY(hipMemcpyAsync(&fl, nd.d_flags, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (!(fl & FLAG_HASH_FULL)) break;
      if (cap >= cap_max) throw PlanError(LK_ERR_MEMORY, "numeric groupBy: value table full at its bound");
      cap = std::min(cap_max, cap * 8);
    }
    const size_t nslots = ng * nnd * size_t(nd.cap);
    keys.resize(nslots);
    HIP_TRY(hipMemcpyAsync(keys.data(), nd.d_keys, nslots * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ones.data(), nd.d_ones, ones.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < nnd; k++) {
      std::vector<std::string> texts;
      for (size_t gi = 0; gi < ng; gi++) {
        const unsigned long long* tk = keys.data() + (gi * nnd + k) * size_t(nd.cap);
        for (size_t s2 = 0; s2 < nd.cap; s2++)
          if (tk[s2] != TAG_EMPTY) texts.push_back(text_of(k, gi, tk[s2]));
        if (ones[gi * nnd + k]) texts.push_back(text_of(k, gi, TAG_EMPTY));
      }
      mine[k] = numdim_text_union({texts});
    }
  });
  // the dimensions: the sorted union of every rank's texts, dim id = position
  std::vector<std::vector<std::vector<std::string>>> sets(nnd);   // [column][rank]
  if (C.dist) {
    const auto t1 = std::chrono::steady_clock::now();
    std::string blob;
    for (size_t k = 0; k < nnd; k++) put_texts(blob, mine[k]);
    // (a rank whose discovery failed sends its pending status: every rank throws it here)
    const std::vector<std::string> all = comm_allgather_status(C.E, C.X, 0, std::string(), blob);
    for (const std::string& b : all) {
      size_t at = 0;
      for (size_t k = 0; k < nnd; k++) sets[k].push_back(get_texts(b, at));
    }
    nd.exchange_bytes = blob.size();
    nd.exchange_ms = ms_since(t1);
  } else {
    for (size_t k = 0; k < nnd; k++) sets[k].push_back(std::move(mine[k]));
  }
  for (size_t k = 0; k < nnd; k++) {   // (the bounds are checked on the union: every rank fails alike)
    DimCol& dc = pl.dp.dims[first + k];
    dc.cand = numdim_text_union(sets[k]);
    if (dc.cand.size() + 1 > DIM_MASK) throw PlanError(LK_ERR_UNSUPPORTED, "group dimension too large");
    dc.ndim = uint32_t(dc.cand.size()) + 1;
    dc.dim_null = uint32_t(dc.cand.size());
  }
  local([&] {
    if (C.dist) fault_point(C.E, "numdim_ids");
    const size_t nslots = ng * nnd * size_t(nd.cap);
    std::vector<uint32_t> ids(nslots, 0);
    for (size_t k = 0; k < nnd; k++) {
      const DimCol& dc = pl.dp.dims[first + k];
      for (size_t gi = 0; gi < ng; gi++) {
        const size_t base = (gi * nnd + k) * size_t(nd.cap);
        for (size_t s2 = 0; s2 < nd.cap; s2++)
          if (keys[base + s2] != TAG_EMPTY) ids[base + s2] = numdim_id_of(dc.cand, text_of(k, gi, keys[base + s2]));
        ones[gi * nnd + k] = ones[gi * nnd + k] ? numdim_id_of(dc.cand, text_of(k, gi, TAG_EMPTY)) : dc.dim_null;
      }
    }
    HIP_TRY(hipMemcpyAsync(nd.d_ids, ids.data(), nslots * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(nd.d_ones, ones.data(), ones.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
  });
  nd.ms = ms_since(t0);
}

// Zero the table and scan; returns the kernel's flags.
uint32_t run_scan(const EvalCall& C, const Plan& pl, DevState& dv) {
  dv.nc = pl.cs.hash_mode ? size_t(dv.cap) : size_t(std::max<uint64_t>(pl.cs.ncells, 1));
  if (C.dist && !pl.cs.hash_mode) {   // the reduce stage's buffers
    fault_point(C.E, "reduce");
    if (dv.keyrange) {
      (void)C.X.workspace("kr_parts", size_t(dv.W) * 5 * dv.kr_len * 8 + 64);
      (void)C.X.workspace("kr_counts", (size_t(finalize_blocks(dv.kr_len)) + 2) * 4);
    } else {
      comm_reduce_prepare(C.E, C.X, dv.nc);
    }
  }
  zero_table(C, dv, dv.nc, pl.cs.hash_mode);   // (and the flags)
  dv.P.plan_bytes = (C.flags & LK_PLAN_BYTES) ? reinterpret_cast<unsigned long long*>(dv.P.flags + 2) : nullptr;
  HIP_TRY(hipEventRecord(C.X.ev_scan0, dv.st));
  const size_t nstamp = size_t(dv.P.max_tiles) * dv.P.nsegs * LK_NSTAMP;
  if (getenv("LK_STAMPS") && nstamp) {   // diagnostics only: per-block phase cycle totals
    dv.P.stamps = static_cast<unsigned long long*>(C.X.workspace("stamps", nstamp * 8));
    HIP_TRY(hipMemsetAsync(dv.P.stamps, 0, nstamp * 8, dv.st));
  }
  dv.launch_ms = ms_since(C.t_start);   // host staging done, scan enqueued
  if (pl.cs.ncells && !pl.sg.qsegs.empty()) {
    // scan_clu's segments are the last n_clu of the staged descriptors (plan_cluster); the other fused kernels see the
    // rest (none: not launched)
    QParams Po = dv.P;
    Po.nsegs -= pl.sg.n_clu;
    HIP_TRY(launch_scan(Po, dv.kagg, dv.st));
    if (pl.sg.n_clu) {
      QParams Pc = dv.P;
      Pc.segs += Po.nsegs;
      Pc.nsegs = pl.sg.n_clu;
      HIP_TRY(launch_scan_clu(Pc, dv.kagg, dv.st));
    }
  }
  if (pl.cs.ncells && !pl.sg.gsegs.empty()) {   // general row scan (numeric comparison leaves, union_by_name promotion)
    const XParams XG = general_scan_params(pl, dv, XMODE_AGG);
    HIP_TRY(XG.nnd ? launch_ex_scan_numdim(XG, dv.st) : launch_ex_scan(XG, dv.st));
  }
  HIP_TRY(hipEventRecord(C.X.ev_scan1, dv.st));
  // small dense single-GPU tables: fixup, rows and flags in one single-workgroup launch (launch_epilogue_small),
  // read after one synchronization from mapped pinned memory -- no fixup / count / scan / write launches, no copies
  const bool epilogue = dv.fast_final && !dv.fast_done && !dv.P.stamps && dv.nc <= kEpilogueMax && dv.out_keys <= kEpilogueMax &&
                        !getenv("LK_NO_EPILOGUE");
  if (epilogue) {
    C.res->alloc_rows(size_t(dv.out_keys), pl.qs.per_glob_rows);
    if (C.res->blk.pinned) {
      FParams Fs{};
      bind_table(Fs, dv.P);
      setup_final(pl, dv, Fs, pl.cs.nslots);
      uint32_t* tail = reinterpret_cast<uint32_t*>(dv.hbuf + dv.o_tail);
      memset(tail, 0, 32);
      HIP_TRY(launch_epilogue_small(dv.P, Fs, dv.nc, dv.kagg, C.res->ts, C.res->val, C.res->gid, pl.qs.per_glob_rows ? C.res->glob : nullptr,
                                    dv.P.flags, tail, dv.st));
      HIP_TRY(hipStreamSynchronize(dv.st));
      dv.fast_rows = tail[4];
      dv.fast_done = true;
      memcpy(&dv.plan_bytes, tail + 2, 8);
      dv.clu_tiles = tail[1];
      return tail[0];
    }
  }
  if (pl.cs.ncells) HIP_TRY(launch_fixup_table(dv.P, dv.nc, dv.kagg, dv.st));
  if (dv.P.stamps) {
    std::vector<unsigned long long> h(nstamp);
    HIP_TRY(hipMemcpyAsync(h.data(), dv.P.stamps, nstamp * 8, hipMemcpyDeviceToHost, dv.st));
    HIP_TRY(hipStreamSynchronize(dv.st));
    static const char* names[LK_NSTAMP] = {"prologue", "defs", "decode", "fold", "filter", "compact", "prefetch", "stream"};
    double sm[LK_NSTAMP] = {};
    size_t n = 0;
    for (size_t i = 0; i < nstamp; i += LK_NSTAMP) {
      if (!(h[i] >> 63)) continue;   // block exited early (zone map / past the segment's tiles)
      h[i] &= ~(1ull << 63);
      for (int k = 0; k < LK_NSTAMP; k++) sm[k] += double(h[i + k]);
      n++;
    }
    if (n) {
      double tot = 0;
      std::string line;
      for (int k = 0; k < LK_NSTAMP; k++) {
        tot += sm[k] / n;
        line += std::string(" ") + names[k] + "=" + std::to_string(long(sm[k] / n));
      }
      fprintf(stderr, "[lk stamps] blocks=%zu mean cycles:%s total=%.0f\n", n, line.c_str(), tot);
    }
  }
  uint32_t fl[4] = {0, 0, 0, 0};
  if (dv.fast_final && !dv.fast_done) {
    C.res->alloc_rows(size_t(dv.out_keys), pl.qs.per_glob_rows);
    if (C.res->blk.pinned) {
      FParams Fs{};
      bind_table(Fs, dv.P);
      setup_final(pl, dv, Fs, pl.cs.nslots);
      const uint32_t nb = finalize_blocks(Fs.nkeys);
      uint32_t* cnts = static_cast<uint32_t*>(C.X.workspace("counts", (size_t(nb) + 2) * 4));
      if (dv.ts_runs_ok && dv.out_keys >= kTsRunsMinKeys) Fs.bucket_pos = reinterpret_cast<uint32_t*>(dv.hbuf + dv.o_bpos);
      HIP_TRY(launch_finalize_count(Fs, cnts, dv.st));
      if (Fs.bucket_pos) {
        HIP_TRY(launch_finalize_bucket_pos(Fs, cnts, dv.st));
        HIP_TRY(hipEventRecord(C.X.ev_rows, dv.st));
      }
      HIP_TRY(launch_finalize_write(Fs, cnts, Fs.bucket_pos ? nullptr : C.res->ts, C.res->val, C.res->gid,
                                    pl.qs.per_glob_rows ? C.res->glob : nullptr, dv.st));
      HIP_TRY(hipMemcpyAsync(&dv.fast_rows, cnts + nb, 4, hipMemcpyDeviceToHost, dv.st));
      dv.fast_done = true;
      if (Fs.bucket_pos) {   // timestamps expanded here while finalize_write's rows cross the host link
        HIP_TRY(hipMemcpyAsync(fl, dv.P.flags, 16, hipMemcpyDeviceToHost, dv.st));
        HIP_TRY(hipEventSynchronize(C.X.ev_rows));
        expand_ts_runs(C.E, C.res->ts, Fs.bucket_pos[pl.cs.nbuckets], Fs);
        HIP_TRY(hipStreamSynchronize(dv.st));
        memcpy(&dv.plan_bytes, fl + 2, 8);
        dv.clu_tiles = fl[1];
        return fl[0];
      }
    }
  }
  HIP_TRY(hipMemcpyAsync(fl, dv.P.flags, 16, hipMemcpyDeviceToHost, dv.st));
  HIP_TRY(hipStreamSynchronize(dv.st));
  memcpy(&dv.plan_bytes, fl + 2, 8);
  dv.clu_tiles = fl[1];
  return fl[0];
}

void scan_agreed(const EvalCall& C, const Plan& pl, DevState& dv) {
  // Every rank reports (error, flags); a failure anywhere fails every rank (no rank is left in a collective),
  // and every rank sees the OR of the flags (so they re-run a too-small hash table together).
  auto agree = [&](int err, const std::string& msg, uint32_t fl) -> uint32_t {
    if (!C.dist) {
      if (err) throw PlanError(err, msg);
      return fl;
    }
    uint32_t all_fl = 0;
    const std::vector<std::string> all =
        comm_allgather_status(C.E, C.X, err, msg, std::string(reinterpret_cast<const char*>(&fl), 4));
    for (const std::string& b : all) {
      uint32_t f = 0;
      memcpy(&f, b.data(), std::min<size_t>(4, b.size()));
      all_fl |= f;
    }
    return all_fl;
  };
  for (;;) {
    dv.attempts++;
    int err = dv.local_err;
    std::string msg = dv.local_msg;
    uint32_t fl = 0;
    if (!err) {
      try {
        fl = run_scan(C, pl, dv);
      } catch (const PlanError& e) {
        if (!C.dist) throw;
        err = e.code;
        msg = e.what();
      }
    }
    // A full hash table is reported as "full, can grow" or "full at its bound" (cap and cap_max are rank-local):
    // the ranks agree on both, re-run together while any rank can grow -- each growing only its own full table --
    // and fail together when any table is full at its bound (a rank must not leave while another
    // re-runs into the next collective).
    const bool my_full = pl.cs.hash_mode && (fl & FLAG_HASH_FULL);
    if (my_full && dv.cap < pl.cs.cap_max) fl = (fl & ~uint32_t(FLAG_HASH_FULL)) | FLAG_HASH_GROW;
    dv.hflags = agree(err, msg, fl);
    if (pl.cs.hash_mode && !(dv.hflags & FLAG_HASH_FULL) && (dv.hflags & FLAG_HASH_GROW)) {
      if (my_full) dv.cap = std::min<uint64_t>(pl.cs.cap_max, dv.cap * 4);
      continue;
    }
    break;
  }
  dv.scan_agreed_ms = ms_since(C.t_start);   // every rank's scan done and its status agreed
  if (dv.hflags & FLAG_METRICS_UNALIGNED) {
    if (pl.gp.step == 1) throw PlanError(LK_ERR_DEVICE, "internal: metrics timestamp off a 1 ms grid");
    throw MetricsUnaligned{};
  }
  if ((dv.hflags & FLAG_MIN_NAN) && pl.qs.agg == AGG_MIN && pl.qs.merged && !pl.cs.min_max_nulls) throw MinNanApart{};
  if (dv.hflags & FLAG_CELL_RANGE)   // (scan_clu raises the same flag for a tile of its segments that its rule does not take)
    throw PlanError(LK_ERR_DEVICE, pl.sg.n_clu ? "internal: bucket outside the table, or a tile of a clustered segment outside scan_clu's "
                                                 "rule (LK_NO_CLUSTER=1 evaluates without the clustered copy)"
                                               : "internal: bucket outside the table");
  if (dv.hflags & FLAG_NUMDIM_MISS) throw PlanError(LK_ERR_DEVICE, "internal: a numeric groupBy value the discovery pass did not list");
  if (dv.hflags & FLAG_HASH_FULL) throw PlanError(LK_ERR_MEMORY, "aggregation hash table full at its bound");
  // DDSketch.accept on NaN / a magnitude beyond the mapping's range throws in the worker's stream stage: the
  // stream fails (Commons.scala:331-335) and query-api sees an empty source
  if (dv.hflags & FLAG_SKETCH_RANGE) throw PlanError(LK_ERR_ARG, "DDSketch: value outside the trackable range");
}

void reduce_tables(const EvalCall& C, const Plan& pl, DevState& dv) {
  // ---- multi-GPU: reduce partial tables to rank 0 over RCCL ----
  const double t_reduce0 = ms_since(C.t_start);
  if (C.dist) {
    if (pl.cs.hash_mode) {
      unsigned long long cap0 = dv.cap;
      comm_reduce_hash(C.E, C.X, dv.P, dv.kagg, cap0);
      dv.cap = cap0;
      dv.nc = size_t(dv.cap);
    } else if (dv.keyrange) {
      // Large dense tables (C5: 10M-key group dims), SURVEY §8(e): the merged output key is the cell index, so the
      // key space is cut into one contiguous range per rank.  All-to-all: every rank sends range j of its partial
      // table to rank j (grouped send/recv: all xGMI links at once, 7/8 of a table per rank instead of every table
      // into rank 0); rank j folds the W slices in rank order (merge_tables: the same deterministic fold) and
      // finalizes its range; the ranges' rows, already in key order, are concatenated on rank 0 in rank order.
      // (buffers placed before the scan's agreement: nothing between it and the exchange fails on one rank)
      const size_t len = dv.kr_len;
      uint8_t* tb = reinterpret_cast<uint8_t*>(dv.P.rows);   // [rows | cnt | hi | lo | ext], nc cells each
      uint8_t* parts = static_cast<uint8_t*>(C.X.workspace("kr_parts", size_t(dv.W) * 5 * len * 8 + 64));
      std::vector<Piece> sends, recvs;
      for (int p2 = 0; p2 < dv.W; p2++)
        for (int a = 0; a < 5; a++) {
          const size_t l2 = size_t(dv.kb[size_t(p2) + 1] - dv.kb[size_t(p2)]);
          sends.push_back(Piece{p2, tb + (size_t(a) * dv.nc + dv.kb[size_t(p2)]) * 8, l2 * 8});
          recvs.push_back(Piece{p2, parts + (size_t(p2) * 5 + size_t(a)) * len * 8, len * 8});
        }
      comm_exchange(C.E, C.X, sends, recvs);
      TableRef T{reinterpret_cast<unsigned long long*>(parts), reinterpret_cast<unsigned long long*>(parts + len * 8),
                 reinterpret_cast<double*>(parts + 2 * len * 8), reinterpret_cast<double*>(parts + 3 * len * 8),
                 reinterpret_cast<unsigned long long*>(parts + 4 * len * 8)};
      FParams Fk{};
      bind_table(Fk, T);
      setup_final(pl, dv, Fk, 1);   // (merged, uncollapsed rows: the key-range shape)
      Fk.key_base = dv.kb[size_t(pl.gp.rank)];
      Fk.cell_base = dv.kb[size_t(pl.gp.rank)];
      Fk.nkeys = len;
      const uint32_t nfk = finalize_blocks(len);
      uint32_t* kc = static_cast<uint32_t*>(C.X.workspace("kr_counts", (size_t(nfk) + 2) * 4));
      uint32_t mine_n = 0;
      // fold + count this rank's range; a failure travels with the row-count all-gather (every rank fails there)
      comm_local(C.X, [&] {
        fault_point(C.E, "keyrange_merge");
        if (!len) return;
        HIP_TRY(launch_merge_tables(T, reinterpret_cast<const unsigned long long*>(parts), dv.W, len, dv.kagg, dv.st));
        HIP_TRY(launch_finalize_count(Fk, kc, dv.st));
        HIP_TRY(hipMemcpyAsync(&mine_n, kc + nfk, 4, hipMemcpyDeviceToHost, dv.st));
        HIP_TRY(hipStreamSynchronize(dv.st));
      });
      const uint64_t n64 = mine_n;
      std::vector<uint64_t> ncnt(static_cast<size_t>(dv.W)), noff(static_cast<size_t>(dv.W));
      uint64_t total_rows = 0;
      {
        const std::vector<std::string> all =
            comm_allgather_status(C.E, C.X, 0, std::string(), std::string(reinterpret_cast<const char*>(&n64), 8));
        for (int j = 0; j < dv.W; j++) {
          memcpy(&ncnt[size_t(j)], all[size_t(j)].data(), 8);
          noff[size_t(j)] = total_rows;
          total_rows += ncnt[size_t(j)];
        }
      }
      if (total_rows >= (uint64_t(1) << 32)) throw PlanError(LK_ERR_UNSUPPORTED, "more than 2^32 result rows");
      // Parallel emission: every rank's GPU writes its range's rows straight into rank 0's result -- a shared host
      // block, columns [ts | value | group id] of total_rows each -- at the range's row offset, so the rows cross
      // every PCIe link of the node at once (otherwise: all rows into rank 0's device, then over its one link).
      const char* se = getenv("LK_SHM_EMIT");
      EmitTarget ET;
      // (a formula's kept operand: the rows are gathered into rank 0's device below and never touch the host block)
      if (total_rows && !dv.keep_dev && !(se && *se == '0')) ET = comm_emit_begin(C.E, C.X, size_t(total_rows) * 20);
      if (ET.ok) {
        const size_t N = size_t(total_rows), o = size_t(noff[size_t(pl.gp.rank)]);
        int wst = ET.mapped ? 0 : LK_ERR_DEVICE;
        if (ET.mapped && mine_n) {
          if (launch_finalize_write(Fk, kc, reinterpret_cast<int64_t*>(ET.dev) + o,
                                    reinterpret_cast<double*>(ET.dev + N * 8) + o,
                                    reinterpret_cast<uint32_t*>(ET.dev + N * 16) + o, nullptr, dv.st) != hipSuccess)
            wst = LK_ERR_DEVICE;
        }
        if (hipStreamSynchronize(dv.st) != hipSuccess) wst = LK_ERR_DEVICE;
        std::string wmsg = "shared result block: mapping or write failed";
        if (!wst && getenv("LK_FAULT")) {   // tests only: an injected failure of the row write
          try {
            fault_point(C.E, "emit");
          } catch (const PlanError& e) {
            wst = LK_ERR_DEVICE;
            wmsg = e.what();
          }
        }
        try {
          comm_agree(C.E, C.X, wst, wmsg);   // every range written
        } catch (...) {
          comm_emit_end(C.E, ET, false);     // rank 0: retire the block (a rank may not have mapped it)
          throw;
        }
        comm_emit_end(C.E, ET, true);   // every rank holds its mapping: this block's name can go
        if (pl.gp.rank == 0) {
          dv.nrows_out = uint32_t(total_rows);
          C.res->adopt_rows(ET.host, N, ET.lease);
          dv.rows_done = true;
        }
        dv.emit_mode = "shared_host_block";
      } else {
      uint8_t* ob = nullptr;
      uint8_t* rb = nullptr;
      comm_local(C.X, [&] {   // this rank's rows (and rank 0's receive buffer), agreed on before they move
        ob = static_cast<uint8_t*>(C.X.workspace("kr_rows_mine", size_t(mine_n) * 20 + 64));
        if (mine_n)
          HIP_TRY(launch_finalize_write(Fk, kc, reinterpret_cast<int64_t*>(ob), reinterpret_cast<double*>(ob + size_t(mine_n) * 8),
                                        reinterpret_cast<uint32_t*>(ob + size_t(mine_n) * 16), nullptr, dv.st));
        HIP_TRY(hipStreamSynchronize(dv.st));   // rows complete before they are sent
        if (pl.gp.rank == 0) rb = static_cast<uint8_t*>(C.X.workspace("kr_rows_all", size_t(total_rows) * 20 + 64));
      });
      comm_agree(C.E, C.X, 0, std::string());
      std::vector<Piece> s2, r2;   // [ts 8 B | value 8 B | group id 4 B] per row, column by column
      const size_t wcol[3] = {8, 8, 4};
      for (int a = 0; a < 3; a++) s2.push_back(Piece{0, ob + size_t(a) * mine_n * 8, size_t(mine_n) * wcol[a]});
      if (pl.gp.rank == 0)
        for (int j = 0; j < dv.W; j++)
          for (int a = 0; a < 3; a++)
            r2.push_back(Piece{j, rb + size_t(a) * total_rows * 8 + noff[size_t(j)] * wcol[a], size_t(ncnt[size_t(j)]) * wcol[a]});
      comm_exchange(C.E, C.X, s2, r2);
      comm_throw_pending(C.X);   // (host transport) a failed unpacking of the last round; no collective follows
      if (pl.gp.rank == 0 && dv.keep_dev) {   // the rows stay on the device: out of the call's workspace, device to device
        dv.nrows_out = uint32_t(total_rows);
        if (dv.nrows_out) {
          HIP_TRY(hipMalloc(&C.res->dev_rows, size_t(dv.nrows_out) * 20 + 64));
          HIP_TRY(hipMemcpyAsync(C.res->dev_rows, rb, size_t(dv.nrows_out) * 20, hipMemcpyDeviceToDevice, dv.st));
          HIP_TRY(hipStreamSynchronize(dv.st));
        }
        dv.rows_done = true;
      } else if (pl.gp.rank == 0) {
        dv.nrows_out = uint32_t(total_rows);
        C.res->alloc_rows(dv.nrows_out, false);
        if (dv.nrows_out) {
          HIP_TRY(hipMemcpyAsync(C.res->ts, rb, size_t(dv.nrows_out) * 8, hipMemcpyDeviceToHost, dv.st));
          HIP_TRY(hipMemcpyAsync(C.res->val, rb + size_t(dv.nrows_out) * 8, size_t(dv.nrows_out) * 8, hipMemcpyDeviceToHost, dv.st));
          HIP_TRY(hipMemcpyAsync(C.res->gid, rb + size_t(dv.nrows_out) * 16, size_t(dv.nrows_out) * 4, hipMemcpyDeviceToHost, dv.st));
        }
        HIP_TRY(hipStreamSynchronize(dv.st));
        dv.rows_done = true;
      }
      dv.emit_mode = "gather_to_root";
      }
    } else {
      comm_reduce_table(C.E, C.X, dv.P, dv.kagg, dv.nc);
    }
    comm_throw_pending(C.X);   // past the last collective: a rank-local failure unwinds this rank alone
  }
  dv.reduce_ms = ms_since(C.t_start) - t_reduce0;   // dist: table reduce (+ key-range emission)
  dv.emit = (!C.dist || pl.gp.rank == 0) && !dv.rows_done;
}

// The occupied slots of the hash table: their keys (and counts), copied to the host; sets dv.nocc.
void occupied_records(const EvalCall& C, DevState& dv, const char* ws, std::vector<unsigned long long>& keys,
                      std::vector<unsigned long long>* cnts) {
  SParams S2{};
  S2.keys = dv.P.hkeys;
  bind_table(S2, dv.P);
  S2.cap = dv.cap;
  const uint32_t nsb = sparse_blocks(dv.cap);
  uint32_t* occ = static_cast<uint32_t*>(C.X.workspace("occ_counts", (size_t(nsb) + 2) * 4));
  HIP_TRY(launch_sparse_count(S2, occ, dv.st));
  uint32_t n32 = 0;
  HIP_TRY(hipMemcpyAsync(&n32, occ + nsb, 4, hipMemcpyDeviceToHost, dv.st));
  HIP_TRY(hipStreamSynchronize(dv.st));
  dv.nocc = n32;
  keys.resize(dv.nocc);
  if (cnts) cnts->resize(dv.nocc);
  if (dv.nocc) {
    auto* recs = static_cast<unsigned long long*>(C.X.workspace(ws, size_t(dv.nocc) * 48 + 64));
    HIP_TRY(launch_table_records(dv.P, dv.cap, occ, recs, dv.nocc, dv.st));
    HIP_TRY(hipMemcpyAsync(keys.data(), recs, dv.nocc * 8, hipMemcpyDeviceToHost, dv.st));
    if (cnts) HIP_TRY(hipMemcpyAsync(cnts->data(), recs + dv.nocc, dv.nocc * 8, hipMemcpyDeviceToHost, dv.st));
    HIP_TRY(hipStreamSynchronize(dv.st));
  }
}

// ces: occupied cells -> (glob, step) -> the set of group-key strings, one HLL each
void ces_rows(const EvalCall& C, const Plan& pl, DevState& dv) {
  std::vector<unsigned long long> keys;
  occupied_records(C, dv, "ces_recs", keys, nullptr);
  // key string of each cell: groupBys.map(g => tags.getOrElse(g, "")).mkString(":") (Aggregator.scala:53-56)
  std::vector<std::string> kstr(dv.nocc);
  for (size_t gi2 = 0; gi2 < C.R.group_bys.size(); gi2++) {
    const size_t ci = size_t(pl.dim_index(C.R.group_bys[gi2]));
    const DimCol& sc = pl.dp.dims[ci];
    GlobalDict& gd = C.E.dict(pl.dim_name(ci));
    std::lock_guard<std::mutex> g(gd.mu);
    for (size_t i = 0; i < dv.nocc; i++) {
      const uint32_t d = uint32_t((keys[i] % pl.dp.ngroups) / (sc.stride ? sc.stride : 1) % sc.ndim);
      if (gi2) kstr[i] += ':';
      if (d != sc.dim_null && sc.stride) {
        const std::string_view v = sc.dim_value(d, gd);
        if (!null_like(v)) kstr[i] += v;
      }
    }
  }
  std::map<std::pair<uint64_t, uint32_t>, size_t> at;   // (step, glob) -> row
  for (size_t i = 0; i < dv.nocc; i++) {
    const unsigned long long cell = keys[i];
    const uint64_t b = (cell / pl.dp.ngroups) % pl.cs.nbuckets;
    const uint32_t slot = pl.qs.per_glob_rows ? uint32_t(cell / pl.dp.ngroups / pl.cs.nbuckets) : 0u;
    auto ins = at.emplace(std::make_pair(b, slot), dv.ces_rows.size());
    if (ins.second) dv.ces_rows.push_back(CesRow{pl.cs.bucket_base + int64_t(b) * dv.P.step, slot, hll::Sketch{}});
    dv.ces_rows[ins.first->second].h.update(kstr[i]);
  }
  std::vector<CesRow> sorted;   // std::map order: (step, glob) ascending
  sorted.reserve(dv.ces_rows.size());
  for (auto& kv : at) sorted.push_back(std::move(dv.ces_rows[kv.second]));
  dv.ces_rows.swap(sorted);
  dv.nrows_out = uint32_t(dv.ces_rows.size());
}

// percentiles: occupied (cell, bin) slots -> one DDSketch per (bucket, glob, key tags)
void sketch_rows(const EvalCall& C, const Plan& pl, DevState& dv) {
  std::vector<unsigned long long> keys, cnts;
  occupied_records(C, dv, "sketch_recs", keys, &cnts);
  // group term of each record's key tags
  std::vector<unsigned long long> kg(dv.nocc, 0);
  std::vector<unsigned long long> cellv(dv.nocc);
  for (size_t i = 0; i < dv.nocc; i++) cellv[i] = keys[i] / DD_NBINS;
  const bool by_name = pl.fp.gbs.empty();
  const bool name_grouped = std::find(pl.fp.gbs.begin(), pl.fp.gbs.end(), std::string(kName)) != pl.fp.gbs.end();
  for (size_t si = 0; si < pl.dp.dims.size(); si++) {
    const DimCol& sc = pl.dp.dims[si];
    if (!sc.is_dim || !sc.stride) continue;
    const bool drop = si == 0 && !by_name && !name_grouped;   // name is no key tag when groupBys exist
    if (drop) continue;   // the name is no key tag (its column is hidden): no group term
    if (si == 0 && by_name) {
      // no groupBys: getGroupByKeyTags reads `datapoint.tags.getOrElse(NAME, "")` with NAME = "_cardinalhq.name"
      // (PushDownAggregatorStage.scala:188-197, Commons.scala:45), but the row's name tag is labelled `name` (the
      // SQL's `"_cardinalhq.name" as name`): every row's key tags are {"_cardinalhq.name": ""} -- one sketch per
      // step, every name in it: no group term (the tag column reads "" for every row: label_rows' tcols[0]).
      continue;
    }
    GlobalDict& gd = C.E.dict(pl.dim_name(si));
    std::lock_guard<std::mutex> g(gd.mu);
    std::unordered_map<uint32_t, bool> nl;
    for (size_t i = 0; i < dv.nocc; i++) {
      uint32_t d = uint32_t((cellv[i] % pl.dp.ngroups) / sc.stride % sc.ndim);
      if (d != sc.dim_null) {
        auto it = nl.find(d);
        if (it == nl.end()) it = nl.emplace(d, null_like(sc.dim_value(d, gd))).first;
        if (it->second) d = sc.dim_null;
      }
      kg[i] += (unsigned long long)d * sc.stride;
    }
  }
  std::map<std::tuple<uint64_t, uint32_t, unsigned long long>, size_t> at;   // (bucket, glob, key) -> row
  for (size_t i = 0; i < dv.nocc; i++) {
    const unsigned long long cell = cellv[i];
    const uint64_t b = (cell / pl.dp.ngroups) % pl.cs.nbuckets;
    const uint32_t slot = uint32_t(cell / pl.dp.ngroups / pl.cs.nbuckets);
    auto ins = at.emplace(std::make_tuple(b, pl.qs.per_glob_rows ? slot : 0u, kg[i]), dv.sk_rows.size());
    if (ins.second)
      dv.sk_rows.push_back(SkRow{pl.cs.bucket_base + int64_t(b) * dv.P.step, pl.qs.per_glob_rows ? slot : 0u, kg[i], dd::Sketch{}});
    dv.sk_rows[ins.first->second].sk.add_bin(uint32_t(keys[i] % DD_NBINS), double(cnts[i]));
  }
  std::vector<size_t> ord(dv.sk_rows.size());
  for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
    const SkRow &x = dv.sk_rows[a], &y = dv.sk_rows[b];
    return x.ts != y.ts ? x.ts < y.ts : (x.glob != y.glob ? x.glob < y.glob : x.gid < y.gid);
  });
  std::vector<SkRow> sorted;
  sorted.reserve(ord.size());
  for (size_t i : ord) sorted.push_back(std::move(dv.sk_rows[i]));
  dv.sk_rows.swap(sorted);
  dv.nrows_out = uint32_t(dv.sk_rows.size());
}

void finalize_dense(const EvalCall& C, const Plan& pl, DevState& dv) {
  // ---- merged min/max with NULL-able values: fold null-like group values per glob-cell SQL value ----
  bind_table(dv.F, dv.P);
  uint32_t fslots = pl.cs.nslots;
  if (pl.cs.rekey && dv.emit && pl.cs.ncells) {
    const size_t n2 = size_t(pl.cs.nbuckets * pl.dp.ngroups);
    uint8_t* t2 = static_cast<uint8_t*>(C.X.workspace("table2", n2 * 24 + 256));
    RParams RP{};
    RP.in_rows = dv.P.rows;
    RP.in_cnt = dv.P.cnt;
    RP.in_ext = dv.P.ext;
    RP.ncells_in = pl.cs.ncells;
    RP.out_rows = reinterpret_cast<unsigned long long*>(t2);
    RP.out_cnt = reinterpret_cast<unsigned long long*>(t2 + n2 * 8);
    RP.out_ext = reinterpret_cast<unsigned long long*>(t2 + n2 * 16);
    RP.nbuckets = pl.cs.nbuckets;
    RP.ngroups = pl.dp.ngroups;
    RP.agg = dv.kagg;
    RP.exist_cnt = dv.fexist;
    for (size_t s = 0; s < pl.dp.dims.size(); s++) {
      if (!pl.dp.dims[s].is_dim) continue;
      if (RP.ndims >= MAXSTR) throw PlanError(LK_ERR_UNSUPPORTED, "too many group dimensions for merged min / max over NULL-able values");
      RP.stride[RP.ndims] = pl.dp.dims[s].stride;
      RP.ndim[RP.ndims] = pl.dp.dims[s].ndim;
      RP.map[RP.ndims] = dv.map_off[s] == SIZE_MAX ? nullptr : dv.d_maps + dv.map_off[s];
      RP.ndims++;
    }
    HIP_TRY(hipMemsetAsync(t2, 0, n2 * 16, dv.st));
    HIP_TRY(hipMemsetAsync(RP.out_ext, dv.kagg == AGG_MIN ? 0xff : 0, n2 * 8, dv.st));
    HIP_TRY(launch_rekey_minmax(RP, dv.st));
    dv.F.rows = RP.out_rows;
    dv.F.cnt = RP.out_cnt;
    dv.F.ext = RP.out_ext;
    fslots = 1;
  }

  // ---- finalize + compaction ----
  setup_final(pl, dv, dv.F, fslots);
  dv.nfb = finalize_blocks(dv.F.nkeys);
  dv.d_counts = static_cast<uint32_t*>(C.X.workspace("counts", (size_t(dv.nfb) + 2) * 4));
  if (dv.fast_done) {
    dv.nrows_out = dv.fast_rows;   // rows already in the result block (speculative finalize behind the scan)
  } else if (dv.emit && dv.F.nkeys) {
    if (!dv.keep_dev && dv.key_rows_ok && dv.F.nkeys == dv.okeys && !dv.F.key_base) dv.F.key_bits = reinterpret_cast<unsigned long long*>(dv.hbuf + dv.o_kbits);
    HIP_TRY(launch_finalize_count(dv.F, dv.d_counts, dv.st));
    HIP_TRY(hipMemcpyAsync(&dv.nrows_out, dv.d_counts + dv.nfb, 4, hipMemcpyDeviceToHost, dv.st));
  }
}

void finalize_sparse(const EvalCall& C, const Plan& pl, DevState& dv) {
  // ---- sparse finalize: occupied slots -> (output key, slot) -> radix sort -> one row per output key ----
  dv.S.keys = dv.P.hkeys;
  bind_table(dv.S, dv.P);
  dv.S.cap = dv.cap;
  dv.S.ngroups = pl.dp.ngroups;
  dv.S.nbuckets = pl.cs.nbuckets;
  dv.S.nslots = pl.cs.nslots;
  dv.S.agg = pl.qs.agg;
  dv.S.per_glob = pl.qs.per_glob_rows ? 1 : 0;
  dv.S.collapse = pl.cs.collapse ? 1 : 0;
  dv.S.rekey = pl.cs.rekey ? 1 : 0;
  for (size_t s = 0; s < pl.dp.dims.size() && pl.cs.rekey; s++) {
    if (!pl.dp.dims[s].is_dim) continue;
    if (dv.S.ndims >= MAXSTR) throw PlanError(LK_ERR_UNSUPPORTED, "too many group dimensions for merged min / max over NULL-able values");
    dv.S.stride[dv.S.ndims] = pl.dp.dims[s].stride;
    dv.S.ndim[dv.S.ndims] = pl.dp.dims[s].ndim;
    dv.S.map[dv.S.ndims] = dv.map_off[s] == SIZE_MAX ? nullptr : dv.d_maps + dv.map_off[s];
    dv.S.ndims++;
  }
  dv.S.name_stride = pl.dp.dims[0].stride ? pl.dp.dims[0].stride : 1;
  dv.S.name_rank = pl.dp.name_rank.empty() ? nullptr : reinterpret_cast<const uint32_t*>(dv.dbuf + dv.o_rank);
  dv.S.bucket_base = pl.cs.bucket_base;
  dv.S.step = dv.P.step;
  dv.S.exist_cnt = dv.fexist;
  dv.S.scale = pl.qs.fscale;
  const uint32_t nsb = sparse_blocks(dv.cap);
  uint32_t* occ = static_cast<uint32_t*>(C.X.workspace("occ_counts", (size_t(nsb) + 2) * 4));
  HIP_TRY(launch_sparse_count(dv.S, occ, dv.st));
  uint32_t n32 = 0;
  HIP_TRY(hipMemcpyAsync(&n32, occ + nsb, 4, hipMemcpyDeviceToHost, dv.st));
  HIP_TRY(hipStreamSynchronize(dv.st));
  dv.nocc = n32;
  const unsigned long long max_key =
      pl.qs.per_glob_rows ? pl.cs.nbuckets * pl.cs.nslots * pl.dp.ngroups : (pl.cs.collapse ? pl.cs.nbuckets : pl.cs.nbuckets * pl.dp.ngroups);
  int end_bit = 1;
  while (end_bit < 64 && (1ull << end_bit) < max_key) end_bit++;
  dv.sws = C.X.workspace("sparse", sparse_workspace_bytes(dv.nocc, end_bit));
  uint32_t* d_nrows = nullptr;
  HIP_TRY(launch_sparse_sort(dv.S, occ, dv.nocc, end_bit, dv.sws, &d_nrows, dv.st));
  HIP_TRY(hipMemcpyAsync(&dv.nrows_out, d_nrows, 4, hipMemcpyDeviceToHost, dv.st));
}

// The table's rows: sketch / ces rows assembled on the host, everything else finalized (and counted) on the device.
void finalize(const EvalCall& C, const Plan& pl, DevState& dv) {
  if (pl.qs.ces || pl.qs.sketch) {
    if (!dv.emit) return;
    if (pl.qs.ces) ces_rows(C, pl, dv);
    else sketch_rows(C, pl, dv);
  } else if (!pl.cs.hash_mode) {
    finalize_dense(C, pl, dv);
  } else if (dv.emit) {
    finalize_sparse(C, pl, dv);
  }
}

// Rows into the result: the host block, or (kEvalKeepDevice) a device buffer the result owns.
void write_rows(const EvalCall& C, const Plan& pl, DevState& dv) {
  if (!dv.fast_done) HIP_TRY(hipStreamSynchronize(dv.st));
  dv.sync_ms = ms_since(C.t_start);     // scan + merge + finalize done
  if (dv.fast_done) C.res->nrows = dv.nrows_out;       // the block holds out_keys rows' room; nrows_out of them are written
  else if (dv.keep_dev) C.res->nrows = dv.nrows_out;   // (the rows stay on the device)
  else if (!dv.rows_done) C.res->alloc_rows(dv.nrows_out, pl.qs.per_glob_rows);
  dv.alloc_ms = ms_since(C.t_start);
  if (pl.qs.ces) {
    for (size_t r = 0; r < dv.nrows_out; r++) {
      C.res->ts[r] = dv.ces_rows[r].ts;
      C.res->val[r] = dv.ces_rows[r].h.estimate();
      C.res->gid[r] = 0;
      if (pl.qs.per_glob_rows) C.res->glob[r] = dv.ces_rows[r].glob;
      if (C.res->keep_sketches) C.res->hll_objs.push_back(dv.ces_rows[r].h);
    }
  } else if (pl.qs.sketch) {
    C.res->sketches.reserve(dv.nrows_out);
    for (size_t r = 0; r < dv.nrows_out; r++) {
      const SkRow& k = dv.sk_rows[r];
      C.res->ts[r] = k.ts;
      C.res->val[r] = k.sk.quantile(pl.qs.quantile);
      C.res->gid[r] = uint32_t(k.gid);
      if (pl.qs.per_glob_rows) C.res->glob[r] = k.glob;
      C.res->sketches.push_back(k.sk.serialize());
      if (C.res->keep_sketches) C.res->dd_objs.push_back(k.sk);
    }
  } else if (dv.keep_dev) {
    if (dv.nrows_out && !dv.rows_done) {   // (rows_done: the key-range reduce left them in dev_rows)
      const size_t n = dv.nrows_out;
      HIP_TRY(hipMalloc(&C.res->dev_rows, n * 20 + 64));
      uint8_t* ob = static_cast<uint8_t*>(C.res->dev_rows);
      int64_t* o_ts = reinterpret_cast<int64_t*>(ob);
      double* o_val = reinterpret_cast<double*>(ob + n * 8);
      uint32_t* o_gid = reinterpret_cast<uint32_t*>(ob + n * 16);
      if (pl.cs.hash_mode) HIP_TRY(launch_sparse_write(dv.S, dv.nocc, dv.sws, o_ts, o_val, o_gid, nullptr, dv.st));
      else HIP_TRY(launch_finalize_write(dv.F, dv.d_counts, o_ts, o_val, o_gid, nullptr, dv.st));
      HIP_TRY(hipStreamSynchronize(dv.st));
    }
  } else if (dv.nrows_out && !dv.rows_done && !dv.fast_done) {
    // Rows written by the kernel straight into the mapped pinned result block when it is pinned: no device->host
    // copies (small async D2H copies cost ~1 ms of completion latency each call on this stack, measured in C4).
    const bool direct = C.res->blk.pinned;
    const size_t nk = direct ? 1 : dv.nrows_out;
    uint8_t* ob = static_cast<uint8_t*>(C.X.workspace("out", nk * (8 + 8 + 8 + 4) + 1024));
    int64_t* o_ts = direct ? C.res->ts : reinterpret_cast<int64_t*>(ob);
    double* o_val = direct ? C.res->val : reinterpret_cast<double*>(ob + nk * 8);
    uint32_t* o_gid = direct ? C.res->gid : reinterpret_cast<uint32_t*>(ob + nk * 16);
    uint32_t* o_glob = pl.qs.per_glob_rows ? (direct ? C.res->glob : reinterpret_cast<uint32_t*>(ob + nk * 24)) : nullptr;
    // large grouped results: values only; timestamps, group ids and globs from the key bits (finalize_count's, already
    // on the host) while the values cross the host link
    const bool key_rows = direct && !pl.cs.hash_mode && dv.F.key_bits;
    const bool ts_runs = direct && !pl.cs.hash_mode && !key_rows && dv.ts_runs_ok && dv.F.nkeys >= kTsRunsMinKeys;
    if (ts_runs) {
      dv.F.bucket_pos = reinterpret_cast<uint32_t*>(dv.hbuf + dv.o_bpos);
      HIP_TRY(launch_finalize_bucket_pos(dv.F, dv.d_counts, dv.st));
      HIP_TRY(hipEventRecord(C.X.ev_rows, dv.st));
    }
    if (pl.cs.hash_mode) HIP_TRY(launch_sparse_write(dv.S, dv.nocc, dv.sws, o_ts, o_val, o_gid, o_glob, dv.st));
    else if (key_rows) HIP_TRY(launch_finalize_write(dv.F, dv.d_counts, nullptr, o_val, nullptr, nullptr, dv.st));
    else HIP_TRY(launch_finalize_write(dv.F, dv.d_counts, ts_runs ? nullptr : o_ts, o_val, o_gid, o_glob, dv.st));
    if (!direct) {
      HIP_TRY(hipMemcpyAsync(C.res->ts, o_ts, size_t(dv.nrows_out) * 8, hipMemcpyDeviceToHost, dv.st));
      HIP_TRY(hipMemcpyAsync(C.res->val, o_val, size_t(dv.nrows_out) * 8, hipMemcpyDeviceToHost, dv.st));
      HIP_TRY(hipMemcpyAsync(C.res->gid, o_gid, size_t(dv.nrows_out) * 4, hipMemcpyDeviceToHost, dv.st));
      if (pl.qs.per_glob_rows) HIP_TRY(hipMemcpyAsync(C.res->glob, o_glob, size_t(dv.nrows_out) * 4, hipMemcpyDeviceToHost, dv.st));
    }
    if (ts_runs) {   // timestamps expanded here while finalize_write's rows cross the host link
      HIP_TRY(hipEventSynchronize(C.X.ev_rows));
      expand_ts_runs(C.E, C.res->ts, dv.nrows_out, dv.F);
    }
    if (key_rows)
      expand_rows_from_keys(C.E, C.res->ts, C.res->gid, pl.qs.per_glob_rows ? C.res->glob : nullptr, dv.F.key_bits, dv.F, pl.qs.per_glob_rows);
    HIP_TRY(hipStreamSynchronize(dv.st));
  }
  dv.copy_ms = ms_since(C.t_start);
  if (!dv.local_err && pl.cs.ncells) HIP_TRY(hipEventElapsedTime(&dv.scan_ms, C.X.ev_scan0, C.X.ev_scan1));
}

void write_stats(const EvalCall& C, const Plan& pl, const DevState& dv, const CommCounters& cc0) {
  const char* reduce = !C.dist ? "none" : (dv.keyrange ? "keyrange" : (pl.cs.hash_mode ? "records_to_root" : "gather_to_root"));
  C.res->scan_ms = double(dv.scan_ms);
  C.res->rows_scanned = (unsigned long long)pl.sg.rows_scanned;
  C.res->reduce = reduce;
  char buf[1280];
  snprintf(buf, sizeof(buf),
           "{\"scan_ms\":%.6f,\"total_ms\":%.6f,\"plan_ms\":%.6f,\"device_ms\":%.6f,\"launch_ms\":%.6f,"
           "\"sync_ms\":%.6f,\"alloc_ms\":%.6f,\"copy_ms\":%.6f,\"rows_scanned\":%llu,"
           "\"algorithmic_bytes\":%llu,\"tiles\":%u,\"cells\":%llu,\"segments\":%zu,\"general_segments\":%zu,"
           "\"failed_globs\":%zu,\"table\":\"%s\","
           "\"slots\":%llu,\"occupied\":%llu,\"attempts\":%d,\"plan_bytes\":%llu,\"reduce\":\"%s\","
           "\"dims_ms\":%.6f,\"dims_rebuilt\":%d,\"emit\":\"%s\",\"exact_sum\":%u,\"global_cells\":%u",
           double(dv.scan_ms), ms_since(C.t_start), dv.plan_ms, dv.copy_ms - dv.plan_ms, dv.launch_ms, dv.sync_ms, dv.alloc_ms, dv.copy_ms, (unsigned long long)pl.sg.rows_scanned,
           (unsigned long long)pl.sg.alg_bytes, pl.sg.total_tiles, (unsigned long long)pl.cs.ncells, pl.sg.qsegs.size() + pl.sg.gsegs.size(), pl.sg.gsegs.size(),
           pl.gp.nfailed, pl.cs.hash_mode ? "hash" : "dense", (unsigned long long)(pl.cs.hash_mode ? dv.cap : pl.cs.ncells), dv.nocc, dv.attempts, dv.plan_bytes,
           reduce, pl.dp.dims_ms,
           pl.dp.dims_rebuilt, dv.emit_mode, dv.P.exact_sum, dv.P.global_cells);
  C.res->stats = buf;
  if (C.dist) {   // the distributed call's stages and collectives (this rank)
    const CommCounters cc = comm_counters(C.E);
    char b2[384];
    snprintf(b2, sizeof(b2),
             ",\"reduce_ms\":%.6f,\"scan_agreed_ms\":%.6f,\"collectives\":%llu,\"allgathers\":%llu,"
             "\"allgather_bytes\":%llu,\"p2p_groups\":%llu,\"p2p_bytes\":%llu",
             dv.reduce_ms, dv.scan_agreed_ms, (unsigned long long)(cc.allgathers - cc0.allgathers + cc.p2p_groups - cc0.p2p_groups),
             (unsigned long long)(cc.allgathers - cc0.allgathers), (unsigned long long)(cc.allgather_bytes - cc0.allgather_bytes),
             (unsigned long long)(cc.p2p_groups - cc0.p2p_groups), (unsigned long long)(cc.p2p_bytes - cc0.p2p_bytes));
    C.res->stats += b2;
  }
  if (!pl.gp.bad_msg.empty()) C.res->stats += ",\"first_glob_error\":\"" + json_escape(pl.gp.bad_msg) + "\"";
  if (C.redo) C.res->stats += ",\"redo\":" + std::to_string(C.redo);   // 1: metrics at 1 ms, 2: MIN cells kept per glob
  if (dv.dense_shape) C.res->stats += ",\"lean_dense_shape\":1";
  C.res->stats += std::string(",\"clustered\":") + (pl.sg.n_clu && pl.cs.ncells ? "1" : "0");   // scan_clu was launched
  if (C.flags & LK_PLAN_BYTES) C.res->stats += ",\"clustered_tiles\":" + std::to_string(dv.clu_tiles);
  if (!pl.qs.numgbs.empty()) {
    std::string nd = ",\"numeric_dims\":[";
    for (size_t k = 0; k < pl.qs.numgbs.size(); k++)
      nd += std::string(k ? "," : "") + "{\"column\":\"" + json_escape(pl.qs.numgbs[k]) + "\",\"values\":" +
            std::to_string(pl.dp.dims[pl.fp.cols.size() + k].cand.size()) + "}";
    char b3[160];
    snprintf(b3, sizeof(b3), "],\"numdim_ms\":%.6f,\"numdim_attempts\":%d", pl.dp.nd.ms, pl.dp.nd.attempts);
    C.res->stats += nd + b3;
    if (C.dist) {
      snprintf(b3, sizeof(b3), ",\"numdim_exchange_ms\":%.6f,\"numdim_exchange_bytes\":%llu", pl.dp.nd.exchange_ms,
               (unsigned long long)pl.dp.nd.exchange_bytes);
      C.res->stats += b3;
    }
  }
  {   // which filter path ran: table (<= TT_MAX_LEAVES leaves) or interpreter, the early / late split, the lean kernels
    char b4[192];
    snprintf(b4, sizeof(b4),
             ",\"filter\":{\"leaves\":%zu,\"table\":%d,\"early\":%d,\"late_mask\":%u,\"vleaf\":%d},\"lean_split\":%u,"
             "\"late_chunk\":%u",
             pl.fp.leaves.size(), pl.fp.truth.empty() ? 0 : 1, pl.fp.early, pl.fp.late_mask, pl.fp.vleaf ? 1 : 0,
             dv.P.lean_split, dv.P.late_chunk);
    C.res->stats += b4;
  }
  C.res->stats += "}";
}
}  // namespace

// One evaluation: plan -> scan -> (RCCL merge) -> finalize -> rows.  Distributed calls issue their collectives in this
// order: the glob agreement (plan_globs; once more after the re-plan of a call with numeric groupBys), one dim union per
// unrestricted dim (plan_dims), the numeric group dimensions' value exchange (discover_numdims), the post-scan status
// all-gathers (scan_agreed), the reduce (reduce_tables).
static int evaluate_once(Engine& E, const std::shared_ptr<const Request>& Rp, const char* const* paths, size_t n_paths,
                         int glob_size, unsigned flags, const int32_t* shard, bool dist, lk_result* res, unsigned redo) {
  auto t_start = std::chrono::steady_clock::now();
  // Distributed calls issue collectives: one at a time per engine, in the same order on every rank.  Every call
  // runs on its own context (stream, workspaces), so local calls from several threads overlap.
  std::unique_lock<std::mutex> comm_lock;
  if (dist && !(flags & kEvalCommHeld)) comm_lock = std::unique_lock<std::mutex>(E.comm_mu);   // (a formula holds it over its operands)
  CtxLease X(E);
  X->pend_code = 0;
  X->pend_msg.clear();
  const CommCounters cc0 = dist ? comm_counters(E) : CommCounters{};
  static const bool plan_timing = getenv("LK_PLAN_TIMING") != nullptr;   // diagnostics: host planning stages
  auto stage = [&](const char* what) {
    if (plan_timing) fprintf(stderr, "[lk plan] %-10s %.3f ms\n", what, ms_since(t_start));
  };
  const Request& R = *Rp;
  stage("parse");
  if (!(flags & LK_PER_GLOB_ROWS) && !(flags & LK_MERGED)) throw PlanError(LK_ERR_ARG, "flags must be LK_PER_GLOB_ROWS or LK_MERGED");
  if (glob_size <= 0) glob_size = 10;
  if (n_paths != R.segments.size()) throw PlanError(LK_ERR_ARG, "paths must match segmentRequests");
  // Exemplar query (no chart, not a tag query): raw rows, ORDER BY timestamp LIMIT n (BaseExpr.scala:234-239)
  if (!R.is_tag_query && !R.has_chart)
    return evaluate_exemplar(E, *X, R, paths, n_paths, glob_size, flags, dist, res, std::string(), shard);
  // Tag-name query (isTagQuery without a tagDataType): SELECT * ... WHERE <filter> (BaseExpr.scala:231-232), each tag
  // name once (tagnames.cpp)
  if (R.is_tag_query && R.tag_name.empty())
    return evaluate_tagnames(E, *X, R, paths, n_paths, glob_size, flags, dist, res);

  const EvalCall C{E, *X, R, paths, n_paths, glob_size, flags, shard, dist, redo, res, t_start};
  Plan pl;   // owns the segments and the FieldTab lock until the call returns
  shape_gate(C, pl.qs);
  if (answer_without_segments(C, pl.qs)) return LK_OK;
  load_segments(C, pl.qs, pl.gp);
  plan_numeric_group_bys(C, pl.qs, pl.gp);   // (before the filter's string columns are listed)
  plan_filter(C, pl.qs, pl.fp);
  if (!pl.gp.tag_numeric || dist) {
    stage("segments");
    plan_globs(C, pl.qs, pl.fp, pl.gp);
  }
  // Distributed numeric groupBys: which groupBys are numeric was agreed on with the glob unions, after the filter was
  // planned from the request alone -- every rank plans again from the shape with the agreed classes (the decision comes
  // from agreed data, so every rank takes this branch, refuses alike and issues the second glob agreement)
  if (dist_numeric_replan(C, pl.qs, pl.gp)) {
    const std::vector<std::string> cands = std::move(pl.gp.gb_cands);
    const std::vector<GbClass> agreed = std::move(pl.gp.gb_class);
    pl.qs = QueryShape{};
    pl.fp = FilterPlan{};
    reset_glob_plan(pl.gp);
    shape_gate(C, pl.qs);
    decide_numeric_group_bys(C, pl.qs, cands, agreed);
    plan_filter(C, pl.qs, pl.fp);
    plan_globs(C, pl.qs, pl.fp, pl.gp);
    stage("replan");
  }
  // A tag query over a numeric tag column (agreed among the ranks): every rank takes the TAGNUM row scan (exemplar.cpp)
  if (pl.gp.tag_numeric) {
    pl.gp.segs.clear();
    return evaluate_exemplar(E, *X, R, paths, n_paths, glob_size, flags, dist, res, R.tag_name, dist ? shard : nullptr);
  }
  stage("globs");
  cell_policy(C, pl.qs, pl.gp, pl.cs);
  plan_dims(C, pl.qs, pl.fp, pl.dp);
  stage("dims");
  plan_tables(C, pl.qs, pl.fp, pl.gp, pl.cs, pl.dp);
  stage("tables");
  plan_cells(C, pl.qs, pl.fp, pl.gp, pl.dp, pl.cs);
  plan_truth(C, pl.qs, pl.fp);
  sketch_leaf_check(pl.qs, pl.fp);   // (a numeric groupBy found in the files: the value leaves' route is gone)
  plan_segments(C, pl.qs, pl.fp, pl.gp, pl.cs, pl.sg);
  stage("qsegs");
  plan_table_mode(pl.qs, pl.sg, pl.cs);
  plan_cluster(pl.cs, pl.sg);
  stage("truth");

  DevState dv;
  stage_upload(C, pl, dv);
  if (!pl.qs.numgbs.empty()) {
    // numeric group dimensions: their values from a discovery pass over the staged query; the group space, cells and
    // table mode then follow from the dimensions' sizes, and the query is staged again with the final strides
    discover_numdims(C, pl, dv);
    plan_strides(pl.dp);
    plan_cells(C, pl.qs, pl.fp, pl.gp, pl.dp, pl.cs);
    plan_table_mode(pl.qs, pl.sg, pl.cs);
    dv = DevState{};
    stage_upload(C, pl, dv);
    // distributed: a rank whose ids did not reach its tables scans nothing; the scan's agreement fails every rank
    if (C.X.pend_code && !dv.local_err) {
      dv.local_err = C.X.pend_code;
      dv.local_msg = C.X.pend_msg;
      C.X.pend_code = 0;
      C.X.pend_msg.clear();
    }
    stage("numdims");
  }
  if (pl.gp.ftab_guard.owns_lock()) pl.gp.ftab_guard.unlock();   // the table is staged: other calls may extend it
  setup_scan(C, pl, dv);
  scan_agreed(C, pl, dv);   // throws the re-runs (MetricsUnaligned / MinNanApart) before anything is written to *res
  reduce_tables(C, pl, dv);
  finalize(C, pl, dv);
  write_rows(C, pl, dv);
  label_rows(C, pl, dv.nrows_out);
  write_stats(C, pl, dv, cc0);
  return LK_OK;
}

int evaluate_req(Engine& E, const std::shared_ptr<const Request>& Rp, const char* const* paths, size_t n_paths,
                        int glob_size, unsigned flags, const int32_t* shard, bool dist, lk_result* res) {
  // Both re-runs are thrown before anything is written to *res, and every rank throws them together (agreed flags).
  unsigned redo = 0;
  for (;;) {
    try {
      return evaluate_once(E, Rp, paths, n_paths, glob_size, flags, shard, dist, res, redo);
    } catch (const MetricsUnaligned&) {
      if (redo & REDO_METRICS_RAW) throw PlanError(LK_ERR_DEVICE, "internal: metrics re-run flagged again");
      redo |= REDO_METRICS_RAW;
    } catch (const MinNanApart&) {
      if (redo & REDO_MIN_APART) throw PlanError(LK_ERR_DEVICE, "internal: min re-run flagged again");
      redo |= REDO_MIN_APART;
    }
  }
}

// Metrics: the worker groups by the raw timestamp (`GROUP BY "_cardinalhq.timestamp"`, BaseExpr.scala:376-394); the
// segment index picks segments whose frequency equals the step (`metric_seg.frequency_ms = ?`,
// QueryEngineV2.scala:746-752), so timestamps normally sit on the step grid and a bucket per step is exact.  When a
// row's timestamp is off that grid (the kernel flags it; every rank sees the flag), the evaluation runs again with
// one bucket per millisecond: the cell key is then the raw timestamp (a sparse key space: the hash table).
int evaluate(Engine& E, const std::string& json, const char* const* paths, size_t n_paths, int glob_size,
             unsigned flags, const int32_t* shard, bool dist, lk_result* res) {
  const std::shared_ptr<const Request> Rp = E.parse_cached(json);
  if (Rp->dataset == "metrics" && Rp->has_chart && !Rp->is_tag_query && Rp->aggregation.size() > 1 &&
      Rp->aggregation[0] == 'p' && !Rp->field_chart() && !Rp->has_extract && !Rp->has_compute)
    return evaluate_metrics_pct(E, json, *Rp, paths, n_paths, glob_size, flags, shard, dist, res);
  if (n_paths == Rp->segments.size() && mixed_steps(*Rp, glob_size <= 0 ? 10 : glob_size))
    return evaluate_mixed_steps(E, json, *Rp, paths, n_paths, glob_size <= 0 ? 10 : glob_size, flags, shard, dist, res);
  return evaluate_req(E, Rp, paths, n_paths, glob_size, flags, shard, dist, res);
}

// Operand of a formula (formula_eval.cpp): one merged evaluation whose rows stay on the device (kEvalKeepDevice).
// Distributed (lk_eval_formula_dist, which holds comm_mu): the sharded evaluation, rank 0's rows kept on its device.
int evaluate_keep_device(Engine& E, const std::shared_ptr<const Request>& Rp, const char* const* paths, size_t n_paths,
                         int glob_size, const int32_t* shard, bool dist, lk_result* res) {
  return evaluate_req(E, Rp, paths, n_paths, glob_size, LK_MERGED | kEvalKeepDevice | (dist ? kEvalCommHeld : 0u), shard,
                      dist, res);
}

// Operand of a distributed formula whose values are assembled on the host (`p<NN>`, ces): the sharded merged
// evaluation, its parts included, under the comm_mu its caller holds.
int evaluate_comm_held(Engine& E, const std::string& json, const char* const* paths, size_t n_paths, int glob_size,
                       const int32_t* shard, lk_result* res) {
  return evaluate(E, json, paths, n_paths, glob_size, LK_MERGED | kEvalCommHeld, shard, true, res);
}

}  // namespace lk
