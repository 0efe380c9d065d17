// Tag-name queries: a PushDownRequest with isTagQuery and no tagDataType -- which tags exist under a filter
// (POST /api/v1/tags/{dataset} without a tagName; QueryEngineV2.evaluateTagQuery, QueryEngineV2.scala:419-491).
//
// Reference (per glob, Commons.scala:343-462): SELECT * FROM (SELECT * FROM read_parquet([...], union_by_name=True)
// WHERE <window>) WHERE <filter>, no ORDER BY, no LIMIT (BaseExpr.scala:231-235).  With the union's first column the
// timestamp (branch T, the only one evaluated), a row becomes DataPoint(getLong(1), getDouble(2) (NULL: 0.0), tags =
// the columns from the third on whose getString is non-NULL, non-empty and not "null"); TagNameCompressionStage then
// drops every tag whose name this call has emitted before and the row when no tag is left; NoisyTagsDropper is not
// applied; PushDownAggregatorStage passes the rows through.
//
// Two stand-ins where the reference is not reproducible:
//   1. rows of a glob arrive in file-list order and, within a file, in row order (DuckDB's default
//      preserve_insertion_order; assumed, not verified against DuckDB);
//   2. the seen-set, which the reference shares among globs that run concurrently, sees the globs in request order, as if
//      they ran one after another.
// With both, column k is emitted on the row f(k) = the smallest (glob, file position, tile, row) among the passing rows
// where k is keepable; the rows returned are the distinct f(k), each with the tags {k : f(k) = row}.
//
// Here: per glob, ex_scan_mask writes one pass bit per row and col_first reduces, per column of the call's union, the
// smallest key of a passing keepable row into first[k] (ex_kernels.hip); first[] comes back as one small copy, tn_rows
// (tagnames.hpp) folds it into rows, and the exemplar route's ex_gather / value_text print them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "engine.hpp"
#include "eval_plan.hpp"
#include "evalutil.hpp"
#include "exemplar.hpp"
#include "hostutil.hpp"
#include "kernels.hpp"
#include "layout.hpp"
#include "parquet.hpp"
#include "tagnames.hpp"

namespace lk {

namespace {

// The groups of segments one mask workspace serves: the open globs' segment ranges of sg.qsegs (staged in glob order).
struct TnGroup {
  uint32_t seg0 = 0, nsegs = 0, max_tiles = 0;
  uint64_t words = 0;   // bitmap words of the group
};

struct TnTiles {
  std::vector<uint32_t> mask_off;   // per call tile: word offset in its group's bitmap
  std::vector<TnGroup> groups;
  uint64_t max_words = 1;
};

// tile_begin per segment, the tiles' bitmap offsets and the groups.
TnTiles tn_tiles(XSegs& sg) {
  TnTiles tt;
  uint32_t tiles = 0;
  for (size_t q = 0; q < sg.qsegs.size(); q++) {
    if (q == 0 || sg.meta[q].glob != sg.meta[q - 1].glob) tt.groups.push_back(TnGroup{uint32_t(q), 0, 0, 0});
    TnGroup& g = tt.groups.back();
    g.nsegs++;
    g.max_tiles = std::max(g.max_tiles, sg.qsegs[q].ntiles);
    sg.qsegs[q].tile_begin = tiles;
    for (const TileDesc& td : sg.meta[q].seg->tiles) {
      if (g.words > 0xffffffffull - 1024) throw PlanError(LK_ERR_UNSUPPORTED, std::string(kTnPrefix) + "a glob beyond 2^38 rows");
      tt.mask_off.push_back(uint32_t(g.words));
      g.words += (uint64_t(td.nrows) + 63) / 64;
    }
    tiles += sg.qsegs[q].ntiles;
    tt.max_words = std::max(tt.max_words, g.words);
  }
  return tt;
}

void tagnames_local(const EvalCall& C) {
  lk_result* res = C.res;
  const Request& R = C.R;
  tn_gate_request(R, C.dist);
  XShape qs;
  qs.star = true;
  qs.limit = 1;   // (no LIMIT: every open glob is scanned)
  qs.per_glob_rows = (C.flags & LK_PER_GLOB_ROWS) != 0;
  x_leaves(R, qs);
  res->exemplar = true;
  res->no_group_ids = true;
  res->per_glob = true;
  if (R.segments.empty()) return sentinel_row(C, qs);
  const XFilter fp = x_filter(C, qs);
  XGlobs gp = x_globs(C, qs, fp);
  // the schemas' part of the gate, over the globs whose files could all be read (the others are empty)
  for (size_t gi = 0; gi < gp.globs.size(); gi++) {
    const XGlob& g = gp.globs[gi];
    if (std::any_of(g.segs.begin(), g.segs.end(), [&](int si) { return gp.seg_bad[si] != 0; })) continue;
    TnGlob files;
    for (int si : g.segs) files.push_back(gp.segs[si]->schema);
    if (tn_gate_glob(files, gi) != g.cols) throw PlanError(LK_ERR_DEVICE, "internal: union order disagrees");
  }
  const std::vector<std::vector<uint32_t>> tabs = x_tables(C.E, fp);
  XSegs sg = x_segments(qs, fp, gp);
  const TnTiles tt = tn_tiles(sg);
  const size_t ng = gp.globs.size(), nq = sg.qsegs.size();
  XDev D = x_stage(C, qs, fp, tabs, sg, ng);
  hipStream_t st = D.st;

  // the call's union: every open glob's columns in first-seen order (column k of first[])
  std::vector<std::string> cols;
  for (auto& g : gp.globs) {
    if (g.skip) continue;
    for (auto& c : g.cols)
      if (std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
  }
  const size_t ncols = cols.size();
  if (ncols > 65535) throw PlanError(LK_ERR_UNSUPPORTED, std::string(kTnPrefix) + "more than 65535 columns in one call");
  // per (segment, column): the streams, and the column dictionary's ids of "" and "null"
  std::vector<TnCol> tcols(nq * ncols);
  for (size_t k = 0; k < ncols; k++) {
    uint32_t id_empty = TN_NO_ID, id_null = TN_NO_ID;
    bool looked = false;
    for (size_t q = 0; q < nq; q++) {
      const Segment& S = *sg.meta[q].seg;
      const XGlob& g = gp.globs[sg.meta[q].glob];
      if (cols[k] == g.cols[0] || cols[k] == g.cols[1]) continue;   // the glob's timestamp and value: no tags
      const int c = S.col_index(cols[k]);
      if (c < 0) continue;   // absent from the file: NULL (an unloaded column was refused by x_segments)
      const HostCol& hc = S.cols[size_t(c)];
      if (hc.is_string && !looked) {
        GlobalDict& gd = C.E.dict(cols[k]);
        std::lock_guard<std::mutex> dg(gd.mu);
        id_empty = gd.ids.find("");
        id_null = gd.ids.find("null");
        looked = true;
      }
      tcols[q * ncols + k] = TnCol{S.d_data, hc.d_runs, hc.d_tcols, hc.d_remap, 1u, hc.is_string ? id_empty : TN_NO_ID,
                                   hc.is_string ? id_null : TN_NO_ID, 0u};
    }
  }

  unsigned long long nfound = 0, stats[2] = {0, 0};
  std::vector<unsigned long long> first(ncols, TN_NONE);
  if (nq && ncols) {
    const size_t ntiles = tt.mask_off.size();
    const size_t b_cols = tcols.size() * sizeof(TnCol), b_off = ntiles * 4;
    const size_t o_off = (b_cols + 255) / 256 * 256, o_first = (o_off + b_off + 255) / 256 * 256;
    const size_t o_stats = o_first + ncols * 8, o_cnt = o_stats + 16, total = o_cnt + ntiles * 4;
    PinnedTmp io(total + 64);
    uint8_t* h = static_cast<uint8_t*>(io.p());
    memcpy(h, tcols.data(), b_cols);
    memcpy(h + o_off, tt.mask_off.data(), b_off);
    uint8_t* d = static_cast<uint8_t*>(C.X.workspace("tnames", total + 64));
    unsigned long long* d_mask = static_cast<unsigned long long*>(C.X.workspace("tnmask", tt.max_words * 8));
    for (size_t gi = 0; gi < ng; gi++) {
      const XGlob& g = gp.globs[gi];
      D.rng.range(gi, g.open && g.win_lo < g.win_hi, g.win_lo, g.win_hi);
    }
    HIP_TRY(hipMemcpyAsync(D.dbuf, D.hbuf, D.stage_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d, h, o_off + b_off, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d + o_first, 0xff, ncols * 8, st));
    HIP_TRY(hipMemsetAsync(d + o_stats, 0, 16 + ntiles * 4, st));
    XParams& P = D.P;
    P.mode = XMODE_EMIT;
    P.mask = d_mask;
    P.mask_off = reinterpret_cast<const uint32_t*>(d + o_off);
    P.pass_cnt = reinterpret_cast<uint32_t*>(d + o_cnt);
    TnParams T{};
    T.segs = P.segs;
    T.ncols = uint32_t(ncols);
    T.cols = reinterpret_cast<const TnCol*>(d);
    T.mask = d_mask;
    T.mask_off = P.mask_off;
    T.pass_cnt = P.pass_cnt;
    T.first = reinterpret_cast<unsigned long long*>(d + o_first);
    T.stats = reinterpret_cast<unsigned long long*>(d + o_stats);
    const QSeg* all_segs = P.segs;
    // group by group on one stream: the mask workspace is the largest group's, and a later group finds most columns
    // already in first[] and prunes
    HIP_TRY(hipEventRecord(C.X.ev_scan0, st));
    for (const TnGroup& g : tt.groups) {
      P.segs = all_segs + g.seg0;
      P.nsegs = g.nsegs;
      P.max_tiles = g.max_tiles;
      HIP_TRY(launch_ex_scan_mask(P, st));
      T.seg0 = g.seg0;
      T.nsegs = g.nsegs;
      T.max_tiles = g.max_tiles;
      HIP_TRY(launch_col_first(T, st));
    }
    HIP_TRY(hipEventRecord(C.X.ev_scan1, st));
    HIP_TRY(hipMemcpyAsync(h + o_first, d + o_first, ncols * 8 + 16, hipMemcpyDeviceToHost, st));   // first[] and the stats
    HIP_TRY(hipStreamSynchronize(st));
    D.scanned(C.X);
    memcpy(first.data(), h + o_first, ncols * 8);
    memcpy(stats, h + o_stats, 16);
  }

  // rows: the distinct first keys; gathered in key order, then ordered by timestamp (ties keep key order)
  const std::vector<TnRow> trows = tn_rows(first.data(), ncols);
  for (auto& r : trows) nfound += r.cols.size();
  std::vector<Cand> cands(trows.size());
  for (size_t i = 0; i < trows.size(); i++) {
    const unsigned long long ref = trows[i].key;
    const uint32_t q = uint32_t(ref >> 48);
    if (q >= nq) throw PlanError(LK_ERR_DEVICE, "internal: tag-name key names no segment");
    cands[i] = Cand{0, q, sg.meta[q].pos, 0, ref};
  }
  std::vector<const Cand*> stream(cands.size());
  for (size_t i = 0; i < cands.size(); i++) stream[i] = &cands[i];
  XGathered G = gather_columns(C, gp, sg, st, stream);
  if (!stream.empty() && G.out_cols != cols) throw PlanError(LK_ERR_DEVICE, "internal: tag-name column order disagrees");
  for (size_t i = 0; i < cands.size(); i++) {
    const Segment& S = *sg.meta[cands[i].qseg].seg;
    const size_t k0 = size_t(std::find(cols.begin(), cols.end(), std::string(kTimestamp)) - cols.begin());
    const unsigned long long raw = G.val[i * ncols + k0];
    const int c = S.col_index(kTimestamp);
    cands[i].ts = (c >= 0 && S.cols[size_t(c)].ptype == pq::INT32) ? int64_t(int32_t(uint32_t(raw))) : int64_t(raw);
  }
  std::vector<size_t> order(cands.size());
  std::iota(order.begin(), order.end(), size_t(0));
  const bool rev = R.reverse_sort;   // as for exemplars (Commons.scala:127)
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return rev ? cands[a].ts > cands[b].ts : cands[a].ts < cands[b].ts;
  });
  XGathered Gs;
  Gs.out_cols = G.out_cols;
  Gs.val.resize(G.val.size());
  Gs.ok.resize(G.ok.size());
  std::vector<uint8_t> keep(cands.size() * ncols, 0);
  for (size_t i = 0; i < order.size(); i++) {
    const size_t o = order[i];
    stream[i] = &cands[o];
    std::copy_n(G.val.begin() + o * ncols, ncols, Gs.val.begin() + i * ncols);
    std::copy_n(G.ok.begin() + o * ncols, ncols, Gs.ok.begin() + i * ncols);
    for (uint32_t k : trows[o].cols) keep[i * ncols + k] = 1;
  }
  write_rows(C, gp, sg, stream, Gs, true, &keep);
  if (!qs.per_glob_rows)
    for (size_t i = 0; i < res->nrows; i++) res->glob[i] = 0;
  char buf[384];
  snprintf(buf, sizeof buf,
           "{\"scan_ms\":%.4f,\"total_ms\":%.4f,\"rows_scanned\":%llu,"
           "\"tag_names\":{\"columns\":%zu,\"found\":%llu,\"rows\":%zu,\"tiles_walked\":%llu,\"tiles_pruned\":%llu},"
           "\"failed_globs\":%zu}",
           double(D.scan_ms), ms_since(C.t_start), (unsigned long long)sg.rows_scanned, ncols, nfound, trows.size(),
           stats[0], stats[1],
           size_t(std::count_if(gp.globs.begin(), gp.globs.end(), [](const XGlob& g) { return g.skip; })));
  res->stats = buf;
}

}  // namespace

int evaluate_tagnames(Engine& E, CallCtx& X, const Request& R, const char* const* paths, size_t n_paths, int glob_size,
                      unsigned flags, bool dist, lk_result* res) {
  const EvalCall C{E, X, R, paths, n_paths, glob_size <= 0 ? 10 : glob_size, flags, nullptr, dist, 0, res,
                   std::chrono::steady_clock::now()};
  tagnames_local(C);
  return LK_OK;
}

}  // namespace lk
