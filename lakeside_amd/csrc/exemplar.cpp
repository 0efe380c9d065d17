// Exemplar queries: a PushDownRequest whose baseExpr has no chart (and no tag query) -- raw rows.
//
// Reference (per glob of `glob_size` segments, Commons.scala:361-389):
//   SELECT "_cardinalhq.timestamp", "_cardinalhq.value", "_cardinalhq.name", "_cardinalhq.message", *     (logs)
//          "_cardinalhq.timestamp", "_cardinalhq.value", "span.name", "span.kind", *                      (traces)
//   FROM (SELECT * FROM read_parquet([...], union_by_name=True) WHERE <window>) WHERE <filter>
//   ORDER BY "_cardinalhq.timestamp" <order, default DESC> LIMIT <limit, default 1000>
// (BaseExpr.getBaseQuery, BaseExpr.scala:206-239; projections 41-45; defaults ASTUtils.scala:360-361).
// Each row becomes DataPoint(timestamp = col 1, value = getDouble(col 2), tags = every later column whose value is
// non-NULL, not "null" and not empty, keyed by column name, values as JDBC getString text) (Commons.toDataPoint,
// Commons.scala:428-459); PushDownAggregatorStage passes exemplar rows through (PushDownAggregatorStage.scala:42,
// 66-68); the globs' streams are folded with Akka mergeSorted under pushDownResponseOrdering (timestamp, reversed
// when reverseSort; Commons.scala:116-132, 391-392).
//
// Here: ex_scan HIST passes narrow each glob's window to the rows that can be in its top `limit`, one ex_scan EMIT
// pass lists them, the host sorts those few candidates, and ex_gather decodes every column of the selected rows
// (ex_kernels.hip).  Documented choices where the reference is unspecified: rows tied on the timestamp keep file
// order (segment position in the glob, then row), which DuckDB's ORDER BY leaves open; metrics exemplars (value =
// getDouble of the name column) fail like the reference's stream does (-> empty).
//
// The evaluation is a sequence of stages over the structs below (exemplar_local, in the style of eval_plan.hpp): a
// stage reads the earlier stages' structs and returns its own.  The selection arithmetic between the HIST passes is
// ex_select.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <set>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "comm.hpp"
#include "engine.hpp"
#include "eval_plan.hpp"
#include "evalutil.hpp"
#include "ex_select.hpp"
#include "exemplar.hpp"
#include "hostutil.hpp"
#include "kernels.hpp"
#include "layout.hpp"
#include "parquet.hpp"

namespace lk {

namespace {

const char* const kMessage = "_cardinalhq.message";   // Commons.scala:59
const char* const kSpanName = "span.name";            // Commons.scala:71
const char* const kSpanKind = "span.kind";            // Commons.scala:72

// union_by_name type of a column over a glob's files (DuckDB's common supertype for the physical types a segment
// writer produces): equal types stay; INT32/INT64 -> BIGINT; integers with FLOAT -> FLOAT; with DOUBLE -> DOUBLE.
// Anything else (strings mixed with numbers, BOOLEAN with numbers, INT96 / FIXED_LEN) is not decoded here.
int union_type(int a, int b) {
  if (a < 0) return b;
  if (a == b) return a;
  auto rank = [](int t) {
    switch (t) {
      case pq::INT32: return 1;
      case pq::INT64: return 2;
      case pq::FLOAT: return 3;
      case pq::DOUBLE: return 4;
      default: return 0;
    }
  };
  const int ra = rank(a), rb = rank(b);
  if (!ra || !rb) throw PlanError(LK_ERR_UNSUPPORTED, "union_by_name over incompatible column types");
  if ((ra <= 2 && rb <= 2)) return pq::INT64;
  if (ra == 4 || rb == 4) return pq::DOUBLE;
  return pq::FLOAT;
}

}  // namespace

// A test knob of the environment, read on every call (the tests change them between the calls of one process).
uint64_t env_u64(const char* name, uint64_t dflt, uint64_t floor) {
  const char* e = getenv(name);
  return e ? std::max<uint64_t>(floor, strtoull(e, nullptr, 10)) : dflt;
}

namespace {

// Rows summed per key, in first-seen order: the first row of a key is kept and `add` folds the later ones into it.
template <class Row, class Key, class Add>
std::vector<Row> sum_first_seen(std::vector<Row>& rows, Key key, Add add) {
  std::vector<Row> out;
  std::map<decltype(key(rows[0])), size_t> at;
  for (auto& r : rows) {
    const auto [it, fresh] = at.emplace(key(r), out.size());
    if (fresh) out.push_back(std::move(r));
    else add(out[it->second], r);
  }
  return out;
}

}  // namespace

// ---- the stages, in call order ----

static XShape x_gate(const EvalCall& C, const std::string& numtag) {
  const Request& R = C.R;
  XShape qs;
  qs.numtag = numtag;
  qs.tagnum = !numtag.empty();
  if (R.has_extract || R.has_compute)
    throw PlanError(LK_ERR_UNSUPPORTED, "extract / compute exemplar queries are not on the hot path");
  qs.logs = R.dataset == "logs";
  if (!qs.tagnum && !qs.logs && R.dataset != "traces") {
    // metrics: the projection's second column is "_cardinalhq.name" (BaseExpr.scala:41); getDouble of a metric
    // name fails the stream, which query-api turns into an empty source (QueryEngineV2.scala:141-145)
    if (R.dataset == "metrics") throw PlanError(LK_ERR_ARG, "metrics exemplar: getDouble of \"_cardinalhq.name\"");
    throw PlanError(LK_ERR_ARG, "Invalid dataset: " + R.dataset);
  }
  std::string order = R.order;
  for (auto& c : order) c = char(toupper(static_cast<unsigned char>(c)));
  if (qs.tagnum) order = "DESC";   // (a tag query has no ORDER BY / LIMIT)
  if (order != "DESC" && order != "ASC") throw PlanError(LK_ERR_ARG, "ORDER BY direction '" + R.order + "'");
  if (R.limit < 0 && !qs.tagnum) throw PlanError(LK_ERR_ARG, "negative LIMIT");
  qs.desc = order == "DESC";
  qs.limit = qs.tagnum ? 0 : uint64_t(R.limit);
  qs.per_glob_rows = (C.flags & LK_PER_GLOB_ROWS) != 0;

  x_leaves(R, qs);
  return qs;
}

void x_leaves(const Request& R, XShape& qs) {
  const std::string& numtag = qs.numtag;
  collect_leaves(R.filter.get(), qs.all_leaves);
  for (auto* l : qs.all_leaves) {
    if (l->extracted || l->computed) throw PlanError(LK_ERR_UNSUPPORTED, "extracted/computed filter fields");
    if (qs.tagnum && l->k == numtag && !numeric_op(l->op) && l->op != "exists" && l->op != "has")
      throw PlanError(LK_ERR_UNSUPPORTED, "string comparison '" + l->op + "' on the numeric tag column " + numtag);
    if (qs.num_col(l)) {
      if (std::find(qs.nums.begin(), qs.nums.end(), l->k) == qs.nums.end()) qs.nums.push_back(l->k);
      continue;
    }
    static const char* ok[] = {"eq", "!=", "in", "not_in", "regex", "contains", "has", "exists"};
    if (std::none_of(std::begin(ok), std::end(ok), [&](const char* o) { return l->op == o; }))
      throw PlanError(LK_ERR_ARG, "Invalid operator " + l->op);
  }
  if (qs.tagnum && std::find(qs.nums.begin(), qs.nums.end(), numtag) == qs.nums.end()) qs.nums.push_back(numtag);
}

// No segments: Commons.scala:393-396, the sentinel DataPoint(-1, -1, {}).
void sentinel_row(const EvalCall& C, const XShape& qs) {
  lk_result* res = C.res;
  if (qs.per_glob_rows) {
    res->alloc_rows(1);
    res->ts[0] = -1;
    res->val[0] = -1.0;
    res->glob[0] = 0;
    res->gid[0] = 0;
  }
  res->stats = "{\"scan_ms\":0,\"total_ms\":0,\"rows_scanned\":0,\"candidates\":0}";
}

XFilter x_filter(const EvalCall& C, const XShape& qs) {
  XFilter fp;
  std::vector<LeafCol>& strs = fp.strs;
  for (auto* l : qs.all_leaves) {
    if (qs.num_col(l)) continue;
    auto it = std::find_if(strs.begin(), strs.end(), [&](const LeafCol& s) { return s.name == l->k; });
    if (it == strs.end()) {
      strs.push_back(LeafCol{});
      strs.back().name = l->k;
      it = strs.end() - 1;
    }
    it->leaves.push_back(l);
  }
  if (2 + strs.size() + qs.nums.size() > size_t(MAXQCOL))
    throw PlanError(LK_ERR_UNSUPPORTED, "too many filter columns in one query");
  for (auto& nm : qs.nums)
    if (std::find_if(strs.begin(), strs.end(), [&](const LeafCol& sc) { return sc.name == nm; }) != strs.end())
      throw PlanError(LK_ERR_UNSUPPORTED, "column " + nm + " used both as a string and as a number");
  if (qs.all_leaves.size() > size_t(MAXLEAF)) throw PlanError(LK_ERR_UNSUPPORTED, "too many filter leaves");
  // (the numeric tag's `exists` / `has` leaves number as IS NOT NULL leaves: BaseExpr's "<tag>" IS NOT NULL)
  static_cast<LeafNumbering&>(fp) = number_leaves(
      C.R.filter.get(), qs.all_leaves, [&](const FilterNode* l) { return qs.num_col(l); }, qs.nums, strs);
  return fp;
}

// Segments and globs.  A segment that cannot be read (missing, corrupt, a shape the loader does not take) fails its
// glob's query only: that glob is empty, the others stream (Commons.scala:249-253, 338-340).
XGlobs x_globs(const EvalCall& C, const XShape& qs, const XFilter& fp) {
  const Request& R = C.R;
  const std::string& numtag = qs.numtag;
  XGlobs gp;
  gp.segs.resize(C.n_paths);
  gp.seg_bad.assign(C.n_paths, 0);
  for (size_t i = 0; i < C.n_paths; i++) {
    try {
      gp.segs[i] = C.E.get_segment(C.paths[i], true);
    } catch (const PlanError& e) {
      if (e.code != LK_ERR_IO) throw;   // capability gaps / evicted keys fail the call
      gp.seg_bad[i] = 1;
    }
  }
  const std::vector<std::string> proj = qs.star ? std::vector<std::string>{}
                                       : qs.tagnum ? std::vector<std::string>{kTimestamp, numtag}
                                       : qs.logs ? std::vector<std::string>{kTimestamp, kValue, kName, kMessage}
                                                 : std::vector<std::string>{kTimestamp, kValue, kSpanName, kSpanKind};
  const std::set<std::string> fset = field_set(R);
  for (size_t i = 0; i < C.n_paths; i += size_t(C.glob_size)) {
    XGlob g;
    for (size_t j = i; j < std::min(C.n_paths, i + size_t(C.glob_size)); j++) g.segs.push_back(int(j));
    g.win_lo = INT64_MAX;
    g.win_hi = INT64_MIN;
    std::vector<std::string> uni;
    for (int si : g.segs) {
      g.win_lo = std::min(g.win_lo, R.segments[si].start_ts);
      g.win_hi = std::max(g.win_hi, R.segments[si].end_ts);
      if (gp.seg_bad[si]) {
        g.skip = true;
        continue;
      }
      for (auto& [name, pt] : gp.segs[si]->schema) {
        if (!g.types.count(name)) uni.push_back(name);
        // a union this engine does not form (e.g. VARCHAR with a number, which DuckDB unifies to VARCHAR): the call
        // fails with LK_ERR_UNSUPPORTED so the caller can fall back, not an empty glob
        g.types[name] = union_type(g.type_or(name, -1), pt);
      }
    }
    for (auto& l : fp.leaves)   // nonExistentFields -> literal false (Commons.scala:224, BaseExpr.scala:462-464)
      if (fset.count(l.node->k) && !g.types.count(l.node->k)) g.leaf_false |= 1u << l.index;
    for (auto& p : proj)      // Binder Error -> empty glob (Commons.scala:249-253)
      if (!g.types.count(p)) g.skip = true;
    for (auto& l : fp.leaves)
      if (!(g.leaf_false >> l.index & 1u) && !g.types.count(l.node->k)) g.skip = true;
    for (auto& k : fp.bad_literal)   // normalizedValue failed for a field this glob has
      if (!(fset.count(k) && !g.types.count(k))) g.skip = true;
    if (qs.tagnum && g.type_or(numtag, -1) == pq::BYTE_ARRAY)   // VARCHAR in a glob of numbers
      throw PlanError(LK_ERR_UNSUPPORTED, "tag column " + numtag + " is text in some files and numeric in others");
    for (auto& nm : qs.nums)   // a VARCHAR compared with a number: Binder Error -> empty glob
      if (g.type_or(nm, -1) == pq::BYTE_ARRAY) g.skip = true;
    g.cols = proj;
    for (auto& u : uni)
      if (std::find(g.cols.begin(), g.cols.end(), u) == g.cols.end()) g.cols.push_back(u);
    gp.globs.push_back(std::move(g));
  }
  return gp;
}

// Per filter column: dictionary value -> leaf bits (cached per (column, leaves) like the aggregate path; a pattern
// RE2 rejects throws out of the call).
std::vector<std::vector<uint32_t>> x_tables(Engine& E, const XFilter& fp) {
  std::vector<std::vector<uint32_t>> tabs(fp.strs.size());
  for (size_t s = 0; s < fp.strs.size(); s++) {
    GlobalDict& gd = E.dict(fp.strs[s].name);
    std::lock_guard<std::mutex> dg(gd.mu);
    const uint32_t dict_n = uint32_t(gd.size());
    const LockedLeafBits cached = extend_leaf_bits(E, fp.strs[s], gd, dict_n);
    tabs[s].resize(std::max<uint32_t>(dict_n, 1));
    for (uint32_t gid = 0; gid < dict_n; gid++) tabs[s][gid] = uint32_t(cached.lb->hit[gid]) << 24;
  }
  return tabs;
}

// Query column qc of q = S's column `name`, when S has it.
static void bind_col(QSeg& q, int qc, const Segment& S, const std::string& name, bool want_string, const XShape& qs,
              const XFilter& fp, const XGlob& g) {
  const int c = S.col_index(name);
  if (c < 0) return;
  const HostCol& hc = S.cols[c];
  if (want_string != hc.is_string)
    throw PlanError(LK_ERR_UNSUPPORTED, "column " + name + " has an unexpected type for its role");
  if (qc == 0 && hc.ptype != pq::INT64 && hc.ptype != pq::INT32)
    throw PlanError(LK_ERR_UNSUPPORTED, "timestamp column must be INT64 or INT32");
  const bool is_tag = qs.tagnum && name == qs.numtag;
  if (qc >= 2 + int(fp.strs.size()) && hc.ptype != pq::INT64 && hc.ptype != pq::DOUBLE && hc.ptype != pq::INT32 &&
      hc.ptype != pq::FLOAT && !(is_tag && hc.ptype == pq::BOOLEAN))
    throw PlanError(LK_ERR_UNSUPPORTED, "numeric comparison on column " + name + " of an undecoded type");
  uint32_t pad = uint32_t(hc.ptype);
  if (is_tag) pad |= uint32_t(g.type_or(name, hc.ptype)) << 8;   // the glob's union type
  q.cols[qc] = QCol{hc.d_pages, hc.d_runs, hc.d_tcols, hc.d_remap, 1u, pad};
}

// Per-segment descriptors.  A referenced column this engine does not decode fails the call (LK_ERR_UNSUPPORTED: the
// caller falls back), where a column of a type the query cannot bind is DuckDB's Binder Error: the glob's descriptors
// go in together or not at all, an empty glob (Commons.scala:249-253) that leaves the other globs unaffected.
XSegs x_segments(const XShape& qs, const XFilter& fp, XGlobs& gp) {
  for (const XGlob& g : gp.globs) {
    if (g.skip) continue;
    for (int si : g.segs) {
      if (!gp.segs[si] || gp.segs[si]->unloaded.empty()) continue;
      const Segment& S = *gp.segs[si];
      std::vector<std::string> used{kTimestamp};
      for (auto& sc : fp.strs) used.push_back(sc.name);
      used.insert(used.end(), qs.nums.begin(), qs.nums.end());
      used.insert(used.end(), g.cols.begin(), g.cols.end());
      for (auto& c : used) {
        const auto u = S.unloaded.find(c);
        if (u != S.unloaded.end()) throw PlanError(LK_ERR_UNSUPPORTED, u->second + " (" + S.key + ")");
      }
    }
  }
  XSegs sg;
  for (size_t gi = 0; gi < gp.globs.size(); gi++) {
    XGlob& g = gp.globs[gi];
    if (g.skip || g.win_lo >= g.win_hi || (qs.limit == 0 && !qs.tagnum)) continue;
    std::vector<QSeg> gq;
    std::vector<XSegMeta> gm;
    try {
      for (size_t p = 0; p < g.segs.size(); p++) {
        const Segment& S = *gp.segs[g.segs[p]];
        QSeg q{};
        q.base = S.d_data;
        q.tiles = S.d_tiles;
        q.ntiles = uint32_t(S.tiles.size());
        q.glob_slot = uint32_t(gi);
        q.leaf_false = g.leaf_false;
        q.win_lo = g.win_lo;
        q.win_hi = g.win_hi;
        bind_col(q, 0, S, kTimestamp, false, qs, fp, g);
        if (!q.cols[0].present) continue;
        for (size_t s = 0; s < fp.strs.size(); s++) bind_col(q, int(2 + s), S, fp.strs[s].name, true, qs, fp, g);
        for (size_t n = 0; n < qs.nums.size(); n++)
          bind_col(q, int(2 + fp.strs.size() + n), S, qs.nums[n], false, qs, fp, g);
        gq.push_back(q);
        gm.push_back(XSegMeta{&S, uint32_t(p), uint32_t(gi)});
      }
    } catch (const PlanError& e) {
      if (e.code != LK_ERR_UNSUPPORTED) throw;
      g.skip = true;
      continue;
    }
    g.open = true;
    sg.qsegs.insert(sg.qsegs.end(), gq.begin(), gq.end());
    sg.meta.insert(sg.meta.end(), gm.begin(), gm.end());
  }
  for (size_t q = 0; q < sg.qsegs.size(); q++) {
    sg.rows_scanned += uint64_t(sg.meta[q].seg->num_rows);
    sg.max_tiles = std::max(sg.max_tiles, sg.qsegs[q].ntiles);
  }
  if (sg.qsegs.size() > 65535) throw PlanError(LK_ERR_UNSUPPORTED, "more than 65535 segments in one evaluation");
  return sg;
}

// Device staging: [segments | truth table | leaf-bit tables | string params | range words | counter], 256-aligned.
XDev x_stage(const EvalCall& C, const XShape& qs, const XFilter& fp, const std::vector<std::vector<uint32_t>>& tabs,
             const XSegs& sg, size_t ng) {
  HIP_TRY(hipSetDevice(C.E.device));
  XDev D;
  D.st = C.X.stream;
  const std::vector<LeafCol>& strs = fp.strs;
  std::vector<uint32_t> truth;
  if (fp.leaves.size() <= size_t(TT_MAX_LEAVES)) truth = truth_table(fp.prog, uint32_t(fp.leaves.size()));
  std::vector<StrParam> strp(strs.size());
  size_t off = 0;
  auto reserve = [&](size_t n) { size_t o = (off + 255) / 256 * 256; off = o + n; return o; };
  const size_t o_segs = reserve(sg.qsegs.size() * sizeof(QSeg));
  const size_t o_truth = reserve(truth.size() * 4);
  std::vector<size_t> o_tab(strs.size());
  for (size_t s = 0; s < strs.size(); s++) o_tab[s] = reserve(tabs[s].size() * 4);
  const size_t o_strp = reserve(strp.size() * sizeof(StrParam));
  D.o_rng = reserve(ng * 8 * 4);          // rlo, rhi, hbase, hwidth
  D.o_n = reserve(8);
  D.stage_bytes = off;
  const size_t o_hist = reserve(ng * XBINS * 4);   // host side only
  uint8_t* hbuf = D.hbuf = static_cast<uint8_t*>(C.X.pinned_buf(off));
  uint8_t* dbuf = D.dbuf = static_cast<uint8_t*>(C.X.workspace("xquery", D.stage_bytes));
  D.d_hist = static_cast<uint32_t*>(C.X.workspace("xhist", std::max<size_t>(ng * XBINS * 4, 4)));
  D.hist = reinterpret_cast<uint32_t*>(hbuf + o_hist);
  D.rng = XRanges{reinterpret_cast<int64_t*>(hbuf + D.o_rng), ng};
  memcpy(hbuf + o_segs, sg.qsegs.data(), sg.qsegs.size() * sizeof(QSeg));
  if (!truth.empty()) memcpy(hbuf + o_truth, truth.data(), truth.size() * 4);
  for (size_t s = 0; s < strs.size(); s++) {
    memcpy(hbuf + o_tab[s], tabs[s].data(), tabs[s].size() * 4);
    strp[s].strtab = reinterpret_cast<const uint32_t*>(dbuf + o_tab[s]);
    strp[s].lbase = strs[s].lbase;
    strp[s].lmask = strs[s].lmask;
    strp[s].hmask = strs[s].hmask;
  }
  memcpy(hbuf + o_strp, strp.data(), strp.size() * sizeof(StrParam));
  XParams& P = D.P;
  P.segs = reinterpret_cast<const QSeg*>(dbuf + o_segs);
  P.nsegs = uint32_t(sg.qsegs.size());
  P.max_tiles = sg.max_tiles;
  P.strp = reinterpret_cast<const StrParam*>(dbuf + o_strp);
  P.nstr = uint32_t(strs.size());
  P.nleaves = uint32_t(fp.leaves.size());
  P.nprog = uint32_t(fp.prog.size());
  memcpy(P.prog, fp.prog.data(), fp.prog.size());
  P.truth = truth.empty() ? nullptr : reinterpret_cast<const uint32_t*>(dbuf + o_truth);
  P.nnum = uint32_t(qs.nums.size());
  P.nnl = uint32_t(fp.nleaves.size());
  for (size_t i = 0; i < fp.nleaves.size(); i++) P.nl[i] = fp.nleaves[i];
  const XRanges d_rng{reinterpret_cast<int64_t*>(dbuf + D.o_rng), ng};
  P.rlo = &d_rng.rlo(0);
  P.rhi = &d_rng.rhi(0);
  P.hbase = &d_rng.hbase(0);
  P.hwidth = &d_rng.hwidth(0);
  P.out_n = reinterpret_cast<uint32_t*>(dbuf + D.o_n);
  P.tag_qc = ~0u;
  return D;
}

namespace {

// ---- tag query over a numeric tag: SELECT "<tag>", COUNT(*) ... GROUP BY "<tag>" per glob (BaseExpr.scala:127-138):
// one TAGNUM pass counts passing rows per (glob, canonical tag value); the host prints each value as JDBC getString
// does for the glob's union_by_name type (Long / Integer / Double / Float / Boolean .toString) ----

struct TagTable {
  uint64_t tcap = 0;
  int attempts = 0;
  uint32_t nrec = 0;
  std::vector<unsigned long long> hrec;   // [nrec]: key, count, glob
  std::vector<unsigned long long> spec;   // [ng]: NULL rows, all-ones-key rows
};

struct TRow {
  uint32_t glob;
  bool null;
  unsigned long long key;
  uint64_t count;
  std::string text;
};

// The TAGNUM pass, its table regrown while it overflows; then the occupied slots as records.
TagTable tagnum_scan(const EvalCall& C, const XShape& qs, const XFilter& fp, const XGlobs& gp, const XSegs& sg, XDev& D) {
  CallCtx& X = C.X;
  hipStream_t st = D.st;
  XParams& P = D.P;
  const size_t ng = gp.globs.size();
  auto pow2 = [](uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
  };
  const uint64_t init_slots = pow2(env_u64("LK_TAGNUM_INIT_SLOTS", uint64_t(1) << 12, 64));
  TagTable T;
  const uint32_t tagk = uint32_t(std::find(qs.nums.begin(), qs.nums.end(), qs.numtag) - qs.nums.begin());
  P.tag_qc = uint32_t(2 + fp.strs.size() + tagk);
  for (size_t gi = 0; gi < ng; gi++) {
    const XGlob& g = gp.globs[gi];
    D.rng.range(gi, !g.skip && g.win_lo < g.win_hi, g.win_lo, g.win_hi);
  }
  uint64_t max_rows = 1;
  std::vector<uint64_t> grow(ng, 0);
  for (const XSegMeta& m : sg.meta) grow[m.glob] += uint64_t(m.seg->num_rows);
  for (uint64_t r : grow) max_rows = std::max(max_rows, r);
  const uint64_t cap_max = std::max<uint64_t>(1 << 12, pow2(2 * max_rows));
  uint64_t tcap = std::min<uint64_t>(cap_max, init_slots);
  HIP_TRY(hipMemcpyAsync(D.dbuf, D.hbuf, D.stage_bytes, hipMemcpyHostToDevice, st));
  P.mode = XMODE_TAGNUM;
  for (;;) {
    T.attempts++;
    const size_t tbytes = ng * tcap * 16 + ng * 16 + 64;
    uint8_t* tb = static_cast<uint8_t*>(X.workspace("tagnum", tbytes));
    P.tkeys = reinterpret_cast<unsigned long long*>(tb);
    P.tcnt = reinterpret_cast<unsigned long long*>(tb + ng * tcap * 8);
    P.tspec = reinterpret_cast<unsigned long long*>(tb + ng * tcap * 16);
    P.tflags = reinterpret_cast<uint32_t*>(tb + ng * tcap * 16 + ng * 16);
    P.tcap = tcap;
    HIP_TRY(hipMemsetAsync(tb, 0xff, ng * tcap * 8, st));
    HIP_TRY(hipMemsetAsync(tb + ng * tcap * 8, 0, ng * tcap * 8 + ng * 16 + 64, st));
    D.scan(X);
    uint32_t fl = 0;
    HIP_TRY(hipMemcpyAsync(&fl, P.tflags, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    D.scanned(X);
    if (!(fl & FLAG_HASH_FULL)) break;
    if (tcap >= cap_max) throw PlanError(LK_ERR_MEMORY, "tag value table full at its bound");
    tcap = std::min(cap_max, tcap * 8);
  }
  T.tcap = tcap;
  // occupied slots -> (key, count, glob) records; per-glob NULL / all-ones counts
  auto* recs = static_cast<unsigned long long*>(X.workspace("tagrecs", ng * tcap * 24 + 64));
  uint32_t* d_n = reinterpret_cast<uint32_t*>(recs);
  HIP_TRY(hipMemsetAsync(d_n, 0, 4, st));
  HIP_TRY(launch_tag_compact(P.tkeys, P.tcnt, tcap, uint32_t(ng), recs + 1, d_n, st));
  T.spec.resize(ng * 2);
  HIP_TRY(hipMemcpyAsync(&T.nrec, d_n, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(T.spec.data(), P.tspec, ng * 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  T.hrec.resize(size_t(T.nrec) * 3);
  if (T.nrec) {
    HIP_TRY(hipMemcpyAsync(T.hrec.data(), recs + 1, size_t(T.nrec) * 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return T;
}

// Per glob: (key, count) in the union type's value order, NULL last; merged: counts summed per tag text (NULL apart).
std::vector<TRow> tagnum_rows(const XShape& qs, const XGlobs& gp, const TagTable& T) {
  const size_t ng = gp.globs.size();
  std::vector<int> ut(ng);   // the tag's union type per glob
  for (size_t gi = 0; gi < ng; gi++) ut[gi] = gp.globs[gi].type_or(qs.numtag, pq::INT64);
  std::vector<TRow> rows;
  for (uint32_t i = 0; i < T.nrec; i++)
    rows.push_back(TRow{uint32_t(T.hrec[3 * i + 2]), false, T.hrec[3 * i], T.hrec[3 * i + 1], std::string()});
  for (uint32_t gi = 0; gi < ng; gi++) {
    if (T.spec[2 * gi + 1]) rows.push_back(TRow{gi, false, TAG_EMPTY, T.spec[2 * gi + 1], std::string()});
    if (T.spec[2 * gi]) rows.push_back(TRow{gi, true, 0, T.spec[2 * gi], std::string()});
  }
  for (auto& r : rows)
    if (!r.null) r.text = value_text(r.key, ut[r.glob], ut[r.glob]);
  std::sort(rows.begin(), rows.end(), [&](const TRow& a, const TRow& b) {
    if (a.glob != b.glob) return a.glob < b.glob;
    if (a.null != b.null) return b.null;
    if (a.null) return false;
    const int t = ut[a.glob];
    if (t != pq::DOUBLE && t != pq::FLOAT)       // integers (the all-ones key is -1): exact order, not as doubles
      return int64_t(a.key) < int64_t(b.key);    // (beyond 2^53 doubles tie and the text order is wrong)
    const double x = raw_as_double(a.key, t), y = raw_as_double(b.key, t);
    if (x != y && x == x && y == y) return x < y;
    return a.text < b.text;
  });
  if (!qs.per_glob_rows) {
    rows = sum_first_seen(
        rows, [](const TRow& r) { return std::make_pair(r.null, r.text); },
        [](TRow& kept, const TRow& r) { kept.count += r.count; });
    for (auto& r : rows) r.glob = 0;
  }
  return rows;
}

// Rows: Commons.toDataPoint's tag branch (Commons.scala:406-423): the tag (dropped when NULL / "" / "null" or a noisy
// name, NoisyTagsDropper) and "count"; value = the count, timestamp = now (as the string tag path).
void tagnum_result(const EvalCall& C, const XShape& qs, const XGlobs& gp, const XSegs& sg, const XDev& D,
                   const TagTable& T, const std::vector<TRow>& rows) {
  lk_result* res = C.res;
  const int64_t now_ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                             std::chrono::system_clock::now().time_since_epoch()).count();
  const bool hide = noisy_tag(qs.numtag);
  res->per_glob = qs.per_glob_rows;
  res->alloc_rows(rows.size());
  res->tag_names = {qs.numtag, "count"};
  res->ex_tags.assign(rows.size() * 2, nullptr);
  for (size_t i = 0; i < rows.size(); i++) {
    res->ts[i] = now_ms;
    res->val[i] = double(rows[i].count);
    res->glob[i] = rows[i].glob;
    res->gid[i] = uint32_t(i);
    if (!rows[i].null && !hide && !null_like(rows[i].text)) {
      res->owned.push_back(rows[i].text);
      res->ex_tags[2 * i] = res->owned.back().c_str();
    }
    res->owned.push_back(std::to_string((unsigned long long)rows[i].count));
    res->ex_tags[2 * i + 1] = res->owned.back().c_str();
  }
  char buf[320];
  snprintf(buf, sizeof buf,
           "{\"scan_ms\":%.4f,\"total_ms\":%.4f,\"rows_scanned\":%llu,\"tag_values\":%u,\"attempts\":%d,"
           "\"slots\":%llu,\"table\":\"tagnum\",\"failed_globs\":%zu}",
           double(D.scan_ms), ms_since(C.t_start), (unsigned long long)sg.rows_scanned, T.nrec, T.attempts,
           (unsigned long long)T.tcap,
           size_t(std::count_if(gp.globs.begin(), gp.globs.end(), [](const XGlob& g) { return g.skip; })));
  res->stats = buf;
}

// ---- exemplar rows ----

// HIST passes: narrow every open glob to the rows that can make its top `limit` (ex_select.hpp); returns the passes.
int select(const EvalCall& C, const XShape& qs, XGlobs& gp, const XSegs& sg, XDev& D) {
  // rows listed beyond each glob's `limit` at most, unless tied on one millisecond; rows a zone-map probe covers first
  // (tests shrink them with LK_EX_CAND_CAP / LK_EX_PROBE_ROWS to exercise the refinement and the probes)
  const uint64_t cand_cap = env_u64("LK_EX_CAND_CAP", uint64_t(1) << 24, 1);
  const uint64_t probe_rows = env_u64("LK_EX_PROBE_ROWS", uint64_t(1) << 20, 1);
  std::vector<XGlob>& globs = gp.globs;
  const size_t ng = globs.size();
  hipStream_t st = D.st;
  std::vector<std::vector<XTile>> zones(ng);
  for (const XSegMeta& m : sg.meta)
    for (const TileDesc& td : m.seg->tiles) zones[m.glob].push_back(XTile{td.ts_min, td.ts_max, td.nrows});
  for (size_t gi = 0; gi < ng; gi++) {
    XGlob& g = globs[gi];
    g.start(qs.limit);
    if (g.open) g.probes = probe_boundaries(zones[gi], g.win_lo, g.win_hi, qs.desc, probe_rows);
  }
  int passes = 0;
  bool first_upload = true;   // the whole staged block once, the range words alone afterwards
  std::vector<XPass> pass(ng);
  while (std::any_of(globs.begin(), globs.end(), [](const XGlob& g) { return g.open; })) {
    for (size_t gi = 0; gi < ng; gi++) {
      const XPass& p = pass[gi] = next_pass(globs[gi], qs.desc, XBINS);
      D.rng.rlo(gi) = p.rlo;
      D.rng.rhi(gi) = p.rhi;
      D.rng.hbase(gi) = p.hbase;
      D.rng.hwidth(gi) = p.hwidth;
    }
    HIP_TRY(hipMemcpyAsync(first_upload ? D.dbuf : D.dbuf + D.o_rng, first_upload ? D.hbuf : D.hbuf + D.o_rng,
                            first_upload ? D.stage_bytes : ng * 32, hipMemcpyHostToDevice, st));
    first_upload = false;
    HIP_TRY(hipMemsetAsync(D.d_hist, 0, ng * XBINS * 4, st));
    D.P.mode = XMODE_HIST;
    D.P.nbins = XBINS;
    D.P.hist = D.d_hist;
    D.scan(C.X);
    HIP_TRY(hipMemcpyAsync(D.hist, D.d_hist, ng * XBINS * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    D.scanned(C.X);
    passes++;
    for (size_t gi = 0; gi < ng; gi++)
      if (globs[gi].open) narrow(globs[gi], D.hist + gi * XBINS, pass[gi].nb, pass[gi].hwidth, qs.desc, cand_cap);
  }
  return passes;
}

// EMIT: the `total` candidates of every glob's final range.
std::vector<Cand> emit_candidates(const EvalCall& C, const XGlobs& gp, const XSegs& sg, XDev& D, uint64_t total) {
  if (total > (uint64_t(1) << 28)) throw PlanError(LK_ERR_UNSUPPORTED, "too many exemplar candidates");
  std::vector<Cand> cands;
  if (!total) return cands;
  const size_t ng = gp.globs.size();
  hipStream_t st = D.st;
  for (size_t gi = 0; gi < ng; gi++) D.rng.range(gi, gp.globs[gi].count > 0, gp.globs[gi].elo, gp.globs[gi].ehi);
  unsigned long long* d_out = static_cast<unsigned long long*>(C.X.workspace("xcand", total * 16));
  HIP_TRY(hipMemcpyAsync(D.dbuf + D.o_rng, D.hbuf + D.o_rng, ng * 16, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(D.dbuf + D.o_n, 0, 8, st));
  D.P.mode = XMODE_EMIT;
  D.P.out = d_out;
  D.P.cap = uint32_t(total);
  D.scan(C.X);
  // pinned destinations: a device-to-host copy into pageable memory goes through the runtime's staging buffers
  PinnedTmp eo(total * 16 + 64);
  const unsigned long long* h_out = static_cast<const unsigned long long*>(eo.p());
  HIP_TRY(hipMemcpyAsync(eo.p(), d_out, total * 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(eo.p()) + total * 16, D.dbuf + D.o_n, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint32_t got = 0;
  memcpy(&got, static_cast<const uint8_t*>(eo.p()) + total * 16, 4);
  D.scanned(C.X);
  if (got != total) throw PlanError(LK_ERR_DEVICE, "internal: exemplar candidate count disagrees with the histogram");
  cands.resize(total);
  for (uint64_t i = 0; i < total; i++) {
    const unsigned long long ref = h_out[2 * i + 1];
    const uint32_t qs = uint32_t(ref >> 48), tile = uint32_t((ref >> 16) & 0xffffffffu), r = uint32_t(ref & 0xffffu);
    const Segment& S = *sg.meta[qs].seg;
    const TileDesc& td = S.tiles[tile];
    uint64_t row = uint64_t(td.row0) + r;
    for (uint32_t k = 0; k < td.rg; k++) row += uint64_t(S.rg_rows[k]);
    cands[i] = Cand{int64_t(h_out[2 * i]), qs, sg.meta[qs].pos, row, ref};
  }
  return cands;
}

// Per glob the top `limit` in ORDER BY order (ties: file order), then the Akka mergeSorted fold over the globs' streams
// (Commons.scala:391-392): merge(merge(merge([], g0), g1), g2)...
std::vector<const Cand*> order_and_fold(const EvalCall& C, const XShape& qs, size_t ng, const XSegs& sg,
                                        const std::vector<Cand>& cands) {
  std::vector<std::vector<const Cand*>> per(ng);
  for (auto& c : cands) per[sg.meta[c.qseg].glob].push_back(&c);
  const bool rev = C.R.reverse_sort;   // rollupAgg is empty for exemplars (Commons.scala:125-129)
  std::vector<const Cand*> stream;
  for (auto& v : per) {
    std::sort(v.begin(), v.end(), [&](const Cand* a, const Cand* b) {
      if (a->ts != b->ts) return qs.desc ? a->ts > b->ts : a->ts < b->ts;
      if (a->pos != b->pos) return a->pos < b->pos;
      return a->row < b->row;
    });
    if (v.size() > qs.limit) v.resize(size_t(qs.limit));
    stream = merge_sorted(stream, v, [&](const Cand* a, const Cand* b) { return rev ? a->ts > b->ts : a->ts < b->ts; });
  }
  return stream;
}

}  // namespace

XGathered gather_columns(const EvalCall& C, const XGlobs& gp, const XSegs& sg, hipStream_t st,
                         const std::vector<const Cand*>& stream) {
  XGathered G;
  std::vector<std::string>& out_cols = G.out_cols;
  for (auto& g : gp.globs) {
    if (g.skip) continue;
    for (auto& c : g.cols)
      if (std::find(out_cols.begin(), out_cols.end(), c) == out_cols.end()) out_cols.push_back(c);
  }
  const size_t nsel = stream.size(), ncols = out_cols.size(), nq = sg.qsegs.size();
  G.val.resize(nsel * ncols);
  G.ok.resize(nsel * ncols);
  if (!nsel || !ncols) return G;
  std::vector<GCol> gcols(nq * ncols);
  for (size_t q = 0; q < nq; q++) {
    const Segment& S = *sg.meta[q].seg;
    for (size_t k = 0; k < ncols; k++) {
      const int c = S.col_index(out_cols[k]);
      if (c < 0) {
        if (S.all_columns.count(out_cols[k]))
          throw PlanError(LK_ERR_UNSUPPORTED, "column " + out_cols[k] + " has a physical type the engine does not load");
        continue;
      }
      const HostCol& hc = S.cols[c];
      gcols[q * ncols + k] = GCol{S.d_data, hc.d_runs, hc.d_tcols, hc.d_remap, 1u, 0u};
    }
  }
  const size_t gb = gcols.size() * sizeof(GCol), sb = nsel * 8, vb = nsel * ncols * 8, ob = nsel * ncols;
  PinnedTmp gio(gb + sb + vb + ob + 64);   // pinned staging both ways: [columns | selected refs | values | ok]
  uint8_t* hg = static_cast<uint8_t*>(gio.p());
  memcpy(hg, gcols.data(), gb);
  for (size_t i = 0; i < nsel; i++) reinterpret_cast<unsigned long long*>(hg + gb)[i] = stream[i]->ref;
  uint8_t* dg = static_cast<uint8_t*>(C.X.workspace("xgather", gb + sb + vb + ob + 1024));
  HIP_TRY(hipMemcpyAsync(dg, hg, gb + sb, hipMemcpyHostToDevice, st));
  GParams P{};
  P.cols = reinterpret_cast<const GCol*>(dg);
  P.sel = reinterpret_cast<const unsigned long long*>(dg + gb);
  P.nsel = uint32_t(nsel);
  P.ncols = uint32_t(ncols);
  P.val = reinterpret_cast<unsigned long long*>(dg + gb + sb);
  P.ok = dg + gb + sb + vb;
  HIP_TRY(launch_ex_gather(P, st));
  HIP_TRY(hipMemcpyAsync(hg + gb + sb, P.val, vb + ob, hipMemcpyDeviceToHost, st));   // values and ok flags
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(G.val.data(), hg + gb + sb, vb);
  memcpy(G.ok.data(), hg + gb + sb + vb, ob);
  return G;
}

// Rows: timestamp, getDouble(value column) (SQL NULL -> 0.0), tags as JDBC getString text.
void write_rows(const EvalCall& C, const XGlobs& gp, const XSegs& sg, const std::vector<const Cand*>& stream,
                const XGathered& G, bool second_col, const std::vector<uint8_t>* keep) {
  lk_result* res = C.res;
  const std::vector<std::string>& out_cols = G.out_cols;
  const size_t nsel = stream.size(), ncols = out_cols.size(), nq = sg.qsegs.size();
  res->alloc_rows(nsel);
  res->tag_names = out_cols;
  res->ex_tags.assign(nsel * ncols, nullptr);
  // the value column per glob: "_cardinalhq.value", or the glob's second column (SELECT *)
  std::vector<size_t> vcol(gp.globs.size(), ncols);
  for (size_t gi = 0; gi < gp.globs.size(); gi++) {
    const std::vector<std::string>& gc = gp.globs[gi].cols;
    if (second_col && gc.size() < 2) continue;
    vcol[gi] = size_t(std::find(out_cols.begin(), out_cols.end(), second_col ? gc[1] : std::string(kValue)) - out_cols.begin());
  }
  for (size_t i = 0; i < nsel; i++) {
    res->ts[i] = stream[i]->ts;
    res->glob[i] = sg.meta[stream[i]->qseg].glob;
    res->gid[i] = uint32_t(i);
    res->val[i] = 0.0;
  }
  // column by column: each (segment, column)'s physical / union type looked up once, each dictionary locked once
  std::vector<const HostCol*> qcol(nq);
  std::vector<int> qut(nq);
  for (size_t k = 0; k < ncols; k++) {
    const std::string& name = out_cols[k];
    bool any_string = false;
    for (size_t q = 0; q < nq; q++) {
      const Segment& S = *sg.meta[q].seg;
      const int ci = S.col_index(name);
      qcol[q] = ci < 0 ? nullptr : &S.cols[size_t(ci)];
      if (!qcol[q]) continue;
      qut[q] = gp.globs[sg.meta[q].glob].type_or(name, qcol[q]->ptype);
      any_string = any_string || qcol[q]->is_string;
    }
    GlobalDict* gd = any_string ? &C.E.dict(name) : nullptr;
    std::unique_lock<std::mutex> dl;
    if (gd) {
      dl = std::unique_lock<std::mutex>(gd->mu);
      res->keep.push_back(gd->vals);   // tag text outlives a compaction
    }
    for (size_t i = 0; i < nsel; i++) {
      if (!G.ok[i * ncols + k]) continue;
      const uint32_t q = stream[i]->qseg;
      const HostCol& hc = *qcol[q];
      const unsigned long long raw = G.val[i * ncols + k];
      if (k == vcol[sg.meta[q].glob]) res->val[i] = raw_as_double(raw, hc.ptype);
      if (keep && !(*keep)[i * ncols + k]) continue;
      if (hc.is_string) {
        if (qut[q] != pq::BYTE_ARRAY) throw PlanError(LK_ERR_UNSUPPORTED, "union_by_name over string and numeric " + name);
        const std::string& s = (*gd)[size_t(raw)];
        if (!null_like(s)) res->ex_tags[i * ncols + k] = s.c_str();   // Commons.scala:433
      } else {
        res->owned.push_back(value_text(raw, hc.ptype, qut[q]));
        res->ex_tags[i * ncols + k] = res->owned.back().c_str();
      }
    }
  }
}

namespace {

// This process's segments; the time in ex_scan goes to *scan_ms too (the distributed call's stats).
void exemplar_local(const EvalCall& C, const std::string& numtag, double* scan_ms) {
  lk_result* res = C.res;
  const XShape qs = x_gate(C, numtag);
  res->exemplar = true;
  res->per_glob = true;
  if (C.R.segments.empty()) return sentinel_row(C, qs);
  const XFilter fp = x_filter(C, qs);
  XGlobs gp = x_globs(C, qs, fp);
  const std::vector<std::vector<uint32_t>> tabs = x_tables(C.E, fp);
  const XSegs sg = x_segments(qs, fp, gp);
  XDev D = x_stage(C, qs, fp, tabs, sg, gp.globs.size());
  if (qs.tagnum) {
    const TagTable T = tagnum_scan(C, qs, fp, gp, sg, D);
    tagnum_result(C, qs, gp, sg, D, T, tagnum_rows(qs, gp, T));
    *scan_ms = double(D.scan_ms);
    return;
  }
  const int passes = select(C, qs, gp, sg, D);
  uint64_t total = 0;
  for (auto& g : gp.globs) total += g.count;
  const std::vector<Cand> cands = emit_candidates(C, gp, sg, D, total);
  const std::vector<const Cand*> stream = order_and_fold(C, qs, gp.globs.size(), sg, cands);
  write_rows(C, gp, sg, stream, gather_columns(C, gp, sg, D.st, stream));
  char buf[256];
  snprintf(buf, sizeof buf,
           "{\"scan_ms\":%.4f,\"total_ms\":%.4f,\"rows_scanned\":%llu,\"candidates\":%llu,\"hist_passes\":%d}",
           double(D.scan_ms), ms_since(C.t_start), (unsigned long long)sg.rows_scanned, (unsigned long long)total, passes);
  res->stats = buf;
  *scan_ms = double(D.scan_ms);
}

// ---- the ranks' exchange ----

// Row streams as bytes: tag names, then per row ts | value | present tags (column, text).
void put_u32(std::string& b, uint32_t x) { b.append(reinterpret_cast<const char*>(&x), 4); }
void put_str(std::string& b, const std::string& s) {
  put_u32(b, uint32_t(s.size()));
  b += s;
}
struct Reader {
  const std::string& b;
  size_t o = 0;
  template <class T>
  T get() {
    if (o + sizeof(T) > b.size()) throw PlanError(LK_ERR_DEVICE, "internal: short exemplar stream from a rank");
    T x;
    memcpy(&x, b.data() + o, sizeof(T));
    o += sizeof(T);
    return x;
  }
  std::string str() {
    const uint32_t n = get<uint32_t>();
    if (o + n > b.size()) throw PlanError(LK_ERR_DEVICE, "internal: short exemplar stream from a rank");
    std::string s = b.substr(o, n);
    o += n;
    return s;
  }
};
struct XRow {
  int64_t ts;
  double val;
  std::vector<std::pair<std::string, std::string>> tags;   // (column name, text), the row's present tags
};

std::string encode_rows(const lk_result& local) {
  std::string blob;
  const size_t nt = local.tag_names.size();
  put_u32(blob, uint32_t(nt));
  for (auto& n : local.tag_names) put_str(blob, n);
  const uint64_t n = local.nrows;
  blob.append(reinterpret_cast<const char*>(&n), 8);
  for (size_t i = 0; i < local.nrows; i++) {
    blob.append(reinterpret_cast<const char*>(&local.ts[i]), 8);
    blob.append(reinterpret_cast<const char*>(&local.val[i]), 8);
    uint32_t present = 0;
    for (size_t c = 0; c < nt; c++) present += local.tag(i, c) != nullptr;
    put_u32(blob, present);
    for (size_t c = 0; c < nt; c++)
      if (const char* v = local.tag(i, c)) {
        put_u32(blob, uint32_t(c));
        put_str(blob, v);
      }
  }
  return blob;
}

// The ranks' streams; `names`: their tag columns in first-seen order over the ranks.
std::vector<std::vector<XRow>> decode_rows(const std::vector<std::string>& all, std::vector<std::string>& names) {
  std::vector<std::vector<XRow>> streams(all.size());
  for (size_t r = 0; r < all.size(); r++) {
    if (all[r].empty()) continue;
    Reader rd{all[r]};
    const uint32_t nt = rd.get<uint32_t>();
    std::vector<std::string> tn(nt);
    for (auto& t : tn) t = rd.str();
    for (auto& t : tn)
      if (std::find(names.begin(), names.end(), t) == names.end()) names.push_back(t);
    const uint64_t n = rd.get<uint64_t>();
    streams[r].resize(size_t(n));
    for (auto& row : streams[r]) {
      row.ts = rd.get<int64_t>();
      row.val = rd.get<double>();
      const uint32_t np = rd.get<uint32_t>();
      for (uint32_t j = 0; j < np; j++) {
        const uint32_t c = rd.get<uint32_t>();
        if (c >= nt) throw PlanError(LK_ERR_DEVICE, "internal: bad tag column in a rank's exemplar stream");
        row.tags.emplace_back(tn[c], rd.str());
      }
    }
  }
  return streams;
}

// Rank 0's fold.  Exemplars: Akka mergeSorted over the ranks' streams in rank order, then take(limit).  Numeric tags:
// counts summed per tag text (the "count" tag rewritten), NULL / dropped tag apart, first-seen order.
// A deliberate deviation: query-api's streamTags (QueryEngineV2.scala:452-487) flatMapMerges the
// pods' (tag, count) rows unsummed, in arrival order (TagQueryUtils.aggregate is commented out there), so a
// value present on two pods reaches the client twice.  The distributed call returns one merged table instead
// -- the same table the string-tag distributed path returns (one row per value, counts added) -- because
// arrival order across ranks is not reproducible; DESIGN.md §5 records this.
std::vector<XRow> fold_ranks(const Request& R, const std::string& numtag, std::vector<std::vector<XRow>>& streams) {
  std::vector<XRow> out;
  if (numtag.empty()) {
    const bool rev = R.reverse_sort;
    for (auto& v : streams)
      out = merge_sorted(out, v, [&](const XRow& a, const XRow& b) { return rev ? a.ts > b.ts : a.ts < b.ts; });
    if (R.limit >= 0 && out.size() > uint64_t(R.limit)) out.resize(size_t(R.limit));
    return out;
  }
  for (auto& v : streams) std::move(v.begin(), v.end(), std::back_inserter(out));
  out = sum_first_seen(
      out,
      [&](const XRow& row) {
        std::string key = "\x01";   // the tag dropped (NULL or a null-like text)
        for (auto& kv : row.tags)
          if (kv.first == numtag) key = "\x02" + kv.second;
        return key;
      },
      [](XRow& kept, const XRow& row) { kept.val += row.val; });
  for (auto& row : out)
    for (auto& kv : row.tags)
      if (kv.first == "count") kv.second = std::to_string((unsigned long long)row.val);
  return out;
}

void write_dist_rows(lk_result* res, const std::vector<XRow>& out, const std::vector<std::string>& names) {
  res->alloc_rows(out.size());
  res->tag_names = names;
  res->ex_tags.assign(out.size() * names.size(), nullptr);
  for (size_t i = 0; i < out.size(); i++) {
    res->ts[i] = out[i].ts;
    res->val[i] = out[i].val;
    res->glob[i] = 0;
    res->gid[i] = uint32_t(i);
    for (auto& kv : out[i].tags) {
      const size_t c = size_t(std::find(names.begin(), names.end(), kv.first) - names.begin());
      res->owned.push_back(kv.second);
      res->ex_tags[i * names.size() + c] = res->owned.back().c_str();
    }
  }
}

// Distributed exemplar / numeric-tag query (VERDICT r4 missing #1-2).  Reference: query-api fans the pushdown out to
// every worker pod holding segments of the group (SegmentSequencer.allSources), each pod evaluates its own segments
// (globs of its own request, Commons.scala:361-392), and query-api merges the pods' streams -- exemplars:
// flatMapMerge then take(limit) (QueryEngineV2.scala:493-535); tag queries: every pod's (tag, count) rows
// (QueryEngineV2.scala:452-487).  Here each rank is a pod: it evaluates the segments of its shard as the worker
// would (its exemplar stream: per-glob top `limit`, globs folded by mergeSorted; its numeric tag rows: counts per tag
// text over its globs), one all-gather carries every rank's rows (and status: a rank-local failure fails every
// rank), and rank 0 folds them (fold_ranks; rank order is the deterministic stand-in for flatMapMerge's arrival
// order).  Other ranks return no rows.
void exemplar_dist(const EvalCall& C, const std::string& numtag) {
  const Request& R = C.R;
  const int32_t* shard = C.shard;
  const bool tagnum = !numtag.empty();
  const int world = comm_world(C.E), rank = comm_rank(C.E);
  Request sub = copy_request(R);
  sub.segments.clear();
  std::vector<const char*> sp;
  for (size_t i = 0; i < C.n_paths; i++)
    if ((shard ? shard[i] : int32_t(i % size_t(world))) == rank) {
      sp.push_back(C.paths[i]);
      sub.segments.push_back(R.segments[i]);
    }
  int code = 0;
  std::string msg, blob;
  double scan_ms = 0;
  uint64_t local_rows = 0;
  if (!sp.empty()) {   // a pod with no segment of the group is not asked at all (no sentinel row)
    try {
      lk_result local;
      const unsigned flags = tagnum ? LK_MERGED : LK_PER_GLOB_ROWS;
      exemplar_local(EvalCall{C.E, C.X, sub, sp.data(), sp.size(), C.glob_size, flags, nullptr, false, 0, &local,
                              std::chrono::steady_clock::now()}, numtag, &scan_ms);
      blob = encode_rows(local);
      local_rows = local.nrows;
    } catch (const PlanError& e) {
      code = e.code;
      msg = e.what();
    } catch (const std::exception& e) {
      code = LK_ERR_DEVICE;
      msg = e.what();
    }
  }
  const std::vector<std::string> all = comm_allgather_status(C.E, C.X, code, msg, blob);
  C.res->exemplar = true;
  C.res->per_glob = false;
  std::vector<XRow> out;
  std::vector<std::string> names;
  if (rank == 0) {
    std::vector<std::vector<XRow>> streams = decode_rows(all, names);
    out = fold_ranks(R, numtag, streams);
  }
  write_dist_rows(C.res, out, names);
  char buf[320];
  snprintf(buf, sizeof buf,
           "{\"scan_ms\":%.4f,\"total_ms\":%.4f,\"rank_rows\":%llu,\"rows\":%zu,\"reduce\":\"%s\",\"table\":\"%s\"}",
           scan_ms, ms_since(C.t_start), (unsigned long long)local_rows, out.size(),
           tagnum ? "tag_counts" : "merge_sorted", tagnum ? "tagnum" : "exemplar");
  C.res->stats = buf;
}

}  // namespace

int evaluate_exemplar(Engine& E, CallCtx& X, const Request& R, const char* const* paths, size_t n_paths,
                      int glob_size, unsigned flags, bool dist, lk_result* res, const std::string& numtag,
                      const int32_t* shard) {
  const EvalCall C{E, X, R, paths, n_paths, glob_size <= 0 ? 10 : glob_size, flags, shard, dist, 0, res,
                   std::chrono::steady_clock::now()};
  double scan_ms = 0;
  if (dist) exemplar_dist(C, numtag);
  else exemplar_local(C, numtag, &scan_ms);
  return LK_OK;
}

}  // namespace lk
