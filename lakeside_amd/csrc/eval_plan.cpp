// Host planning of an aggregate evaluation: PushDownRequest -> shape -> filter -> globs -> dims -> cells -> segments.
//
// Semantics: globs of `glob_size` segments in request order (Commons.scala:361-366);
// per glob the column union decides nonExistentFields (Commons.scala:214-224) -> literal `false` leaves
// (BaseExpr.scala:462-464) and dropped groupBys (338-346); a column the SQL references that no file of the
// glob has is a DuckDB Binder Error -> empty glob (Commons.scala:249-253); window [min startTs, max endTs)
// (Commons.scala:225-226); step of the glob head (Commons.scala:232); bucket ts - ts % step (logs/traces,
// BaseExpr.scala:163-165) or raw ts (metrics, 376-394).
#include "eval_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <unordered_set>

#include "../../include/lakeside_text.h"
#include "clu.hpp"
#include "comm.hpp"
#include "hostutil.hpp"
#include "layout.hpp"
#include "numgroup_agree.hpp"
#include "parquet.hpp"
#include "regex.hpp"

namespace lk {

// One leaf on one dictionary value (BaseExpr.scala:470-501).  `re`: the compiled RE2-semantics matcher of a
// regex / contains leaf; `set`: the value list of a large in / not_in.
bool leaf_eval(const FilterNode& f, const std::string& s, re::Regex* re, const std::unordered_set<std::string>* set) {
  const std::string& op = f.op;
  if (op == "eq") return s == f.v[0];
  if (op == "!=") return s != f.v[0];
  if (op == "in") return set ? set->count(s) != 0 : std::find(f.v.begin(), f.v.end(), s) != f.v.end();
  if (op == "not_in") return set ? set->count(s) == 0 : std::find(f.v.begin(), f.v.end(), s) == f.v.end();
  if (op == "has" || op == "exists") return true;
  if (op == "regex" || op == "contains") return re->search(s);
  throw PlanError(LK_ERR_UNSUPPORTED, "operator " + op);
}

bool null_like(const std::string& s) { return s.empty() || s == "null"; }
bool null_like(std::string_view s) { return s.empty() || s == "null"; }

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// NoisyTagsDropper.DO_NOT_DISPLAY_TAGS / DO_NOT_DISPLAY_TAG_PREFIXES (core/.../utils/NoisyTagsDropper.scala)
bool noisy_tag(const std::string& t) {
  static const char* const names[] = {
      "day", "month", "hour", "minute", "year", "sketch", "_cardinalhq.tid", "_cardinalhq.would_filter",
      "_cardinalhq.trace_has_error", "_cardinalhq.id", "_cardinalhq.telemetry_type", "_cardinalhq.filtered",
      "_cardinalhq.is_root_span", "_cardinalhq.positive_counts", "_cardinalhq.negative_counts", "metric.stepTs",
      "metric.tagName", "metric.metrics_type", "scope.telemetry.sdk.name", "metric.filter", "metric.dd.israte",
      "metric.dd.rateinterval"};
  for (const char* n : names)
    if (t == n) return true;
  return t.rfind("rollup_", 0) == 0;
}

LockedLeafBits extend_leaf_bits(Engine& E, const LeafCol& sc, const GlobalDict& gd, uint32_t dict_n,
                                const std::vector<char>* skip) {
  std::string key = sc.name;
  for (const FilterNode* l : sc.leaves) {
    key += '\x1f';
    key += l->op;
    for (auto& v : l->v) {
      key += '\x1e';
      key += v;
    }
  }
  std::vector<std::unique_ptr<re::Regex>> res(sc.leaves.size());
  std::vector<std::unique_ptr<std::unordered_set<std::string>>> sets(sc.leaves.size());
  for (size_t j = 0; j < sc.leaves.size(); j++) {
    const FilterNode* l = sc.leaves[j];
    if (skip && (*skip)[j]) continue;
    if (l->op == "regex" || l->op == "contains") res[j] = std::make_unique<re::Regex>(compile_leaf_regex(*l));
    if ((l->op == "in" || l->op == "not_in") && l->v.size() > 8)
      sets[j] = std::make_unique<std::unordered_set<std::string>>(l->v.begin(), l->v.end());
  }
  LockedLeafBits k{E.leaf_bits(key), {}};
  k.guard = std::unique_lock<std::mutex>(k.lb->mu);
  k.lb->hit.reserve(dict_n);
  for (uint32_t gid = uint32_t(k.lb->hit.size()); gid < dict_n; gid++) {
    const std::string& v = gd[gid];
    uint8_t bits = 0;
    for (size_t j = 0; j < sc.leaves.size(); j++)
      if (!(skip && (*skip)[j]) && leaf_eval(*sc.leaves[j], v, res[j].get(), sets[j].get())) bits |= uint8_t(1u << j);
    k.lb->hit.push_back(bits);
  }
  return k;
}

namespace {
// The column's FieldTab over dictionary ids [0, n) (values below n are immutable; the caller holds ft.mu).
void extend_field_tab(FieldTab& ft, const GlobalDict& gd, uint32_t n) {
  ft.val.reserve(n);
  ft.cls.reserve(n);
  for (uint32_t id = uint32_t(ft.cls.size()); id < n; id++) {
    const std::string& s = gd[id];
    double v = 0.0;
    const int c = lk_field_number(s.data(), s.size(), &v);
    ft.val.push_back(c == 1 ? v : 0.0);
    ft.cls.push_back(int8_t(c));
  }
}

// A field chart over VARCHAR column `c` of segment S: every value the column's chunk dictionaries reference must be a
// number or cast to NULL (FieldTab::cls); *bad names the first one that is neither.  The ids come from the segment's
// device remap (the host copy is dropped after the upload); the verdict is kept with the segment.
bool segment_text_ok(Engine& E, const Segment& S, int c, const FieldTab& ft, std::string* bad) {
  std::lock_guard<std::mutex> g(S.field_mu);
  auto it = S.field_text_ok.find(c);
  if (it != S.field_text_ok.end() && it->second) return true;   // (a refused column is searched again for its message)
  const HostCol& hc = S.cols[size_t(c)];
  std::vector<uint32_t> ids(hc.nremap);
  if (hc.nremap) {
    HIP_TRY(hipSetDevice(E.device));
    HIP_TRY(hipMemcpy(ids.data(), hc.d_remap, hc.nremap * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  const GlobalDict& gd = E.dict(hc.name);
  bool ok = true;
  for (uint32_t id : ids) {
    if (id >= ft.cls.size()) throw PlanError(LK_ERR_DEVICE, "internal: dictionary id beyond the field table");
    if (ft.cls[id] >= 0) continue;
    ok = false;
    *bad = gd[id];
    break;
  }
  S.field_text_ok[c] = ok;
  return ok;
}

// Field charts (chart.fieldName / fieldType).  For logs and traces with a standard aggregate BaseExpr.getChartSql
// (BaseExpr.scala:319-405) emits
//   SELECT <step_ts>, <agg>(try_cast(<fieldName>$<fieldType> as double)) [/ 1000000 | / 1000], "_cardinalhq.name" as name ..
//   FROM (..) WHERE <fieldName>$<fieldType> IS NOT NULL AND <filter> GROUP BY ..
// -- the value chart's scan over another column, one more conjunct and a constant divisor (duration: nanoseconds to
// ms, datasize: to KB, BaseExpr.scala:363-367).  The shapes evaluated are the ones whose SQL this engine can restate
// without guessing what DuckDB binds; every other one fails with LK_ERR_UNSUPPORTED and a message naming its rule
// (field charts).  Returns the divisor (0.0: none); every rule depends on the request alone.
double field_chart_gate(const Request& R, int agg, bool per_glob_rows) {
  auto refuse = [](const std::string& why) -> double { throw PlanError(LK_ERR_UNSUPPORTED, "field chart: " + why); };
  if (R.dataset != "logs" && R.dataset != "traces") refuse("the dataset must be logs or traces, not " + R.dataset);
  if (agg != AGG_SUM && agg != AGG_MIN && agg != AGG_MAX && agg != AGG_COUNT && agg != AGG_AVG)
    refuse("aggregation " + R.aggregation + (R.rollup.empty() ? "" : " (rollup " + R.rollup + ")") +
           "; sum, min, max, count and avg are evaluated");
  if (!R.field_type) return 0.0;   // generateSql throws (BaseExpr.scala:355-356): every glob is empty (answer_without_segments)
  // the column is written unquoted (BaseExpr.scala:357-362): only names an unquoted DuckDB identifier keeps as they are
  const std::string col = value_column(R);
  bool plain = !col.empty() && !(col[0] >= '0' && col[0] <= '9') && col[0] != '$';
  for (char c : col) plain = plain && ((c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' || c == '$');
  if (!plain) refuse("column " + col + " is not of the form [a-z_][a-z0-9_$]*");
  // Commons.toDataPoint resets the value to a result tag named fieldName (Commons.scala:442-447)
  if (std::find(R.group_bys.begin(), R.group_bys.end(), *R.field_name) != R.group_bys.end())
    refuse("fieldName " + *R.field_name + " is also a groupBy (resetValueToField)");
  const double scale = *R.field_type == "duration" ? 1e6 : (*R.field_type == "datasize" ? 1e3 : 0.0);
  if (scale != 0.0) {
    // COUNT(..) / 1000 divides a BIGINT by an integer literal: integer or float division by DuckDB version
    if (agg == AGG_COUNT) refuse("count over a " + *R.field_type + " field");
    if (agg == AGG_AVG && !per_glob_rows) refuse("merged avg over a " + *R.field_type + " field (its SUM / COUNT split)");
  }
  return scale;
}
}  // namespace

void shape_gate(const EvalCall& C, QueryShape& qs) {
  qs.per_glob_rows = (C.flags & LK_PER_GLOB_ROWS) != 0;
  qs.merged = !qs.per_glob_rows;
  // ---- shape gate ----
  // Tag query (isTagQuery with a tagDataType): BaseExpr.generateSql (BaseExpr.scala:127-143) emits
  //   SELECT "<tag>", COUNT(*) AS count FROM {table} WHERE <filter> AND <window> GROUP BY "<tag>"
  // i.e. the same scan with one group dim (the tag), one bucket and COUNT(*) (rows, NULL values included).
  qs.tagq = C.R.is_tag_query && !C.R.tag_name.empty();
  // (tagDataType -- "string", "number", ... from the API's query parameter, QueryApi.scala:128-129 -- does not enter
  // the worker's SQL: the tag column's own type decides; a numeric tag column takes the row scan, load_segments)
  if (!qs.tagq && C.R.is_tag_query)   // isTagQuery without a tagDataType: SELECT * ... WHERE <filter> (BaseExpr.scala:231-232)
    throw PlanError(LK_ERR_UNSUPPORTED, "tag queries without a tagDataType");
  if (C.R.has_extract || C.R.has_compute) throw PlanError(LK_ERR_UNSUPPORTED, "extract / compute are not on the hot path");
  qs.fchart = C.R.field_chart();
  if (qs.fchart && C.R.is_tag_query) throw PlanError(LK_ERR_UNSUPPORTED, "field chart: a tag query takes no chart field");
  if (C.R.dataset != "logs" && C.R.dataset != "traces" && C.R.dataset != "metrics")
    throw PlanError(LK_ERR_ARG, "Invalid dataset: " + C.R.dataset);
  shape_aggregation(C.R, qs);   // agg, sketch, ces, no_value_col (filter_plan.cpp)
  // Field chart (chart.fieldName / fieldType): the same scan over `<fieldName>$<fieldType>` (field_chart_gate)
  qs.fscale = qs.fchart ? field_chart_gate(C.R, qs.agg, qs.per_glob_rows) : 0.0;
  if (qs.sketch) {
    char* end = nullptr;
    const std::string pct = C.R.aggregation.substr(1);
    qs.quantile = strtod(pct.c_str(), &end) / 100.0;
    if (end == pct.c_str() || *end || !(qs.quantile >= 0.0 && qs.quantile <= 1.0))
      throw PlanError(LK_ERR_ARG, "percentile aggregation " + C.R.aggregation);
  }
  // Merged avg: query-api runs AVG as separate SUM and COUNT pushdowns, merges them per (timestamp, tags) into
  // a {sum, count} map and divides (QueryEngineV2.scala:280-283, TimeGroupedSketchAggregator.scala:74-78,
  // BaseExpr.scala:88-91).  The table holds both, so one scan gives Σsum / Σcount (NaN when no value).
  // (metrics percentiles evaluate their per-glob MAX rows distributed: kEvalDistPerGlob, internal)
  if (C.dist && qs.per_glob_rows && !(C.flags & kEvalDistPerGlob))
    throw PlanError(LK_ERR_ARG, "distributed evaluation returns merged rows");
  qs.metrics = C.R.dataset == "metrics" && !qs.tagq;   // a tag query groups no timestamps
  qs.vcol = value_column(C.R);

  shape_leaves(C.R, qs);   // the filter's leaves, its numeric columns (filter_plan.cpp)
  // p<NN> / ces: numeric leaves run only as value leaves -- decided from a scratch plan of the request's filter, so the
  // refusal still reads the request and the shape alone and comes before a segment is loaded or a collective issued
  sketch_leaf_gate(C.R, qs);
  // (distributed: the numeric leaves' per-glob decisions -- a bad literal, a VARCHAR column -- come from the agreed glob
  // unions, and the general row scan's partial tables reduce like any other)
}

bool answer_without_segments(const EvalCall& C, const QueryShape& qs) {
  // no segments: the worker answers one sentinel row (Commons.scala:393-396)
  if (C.R.segments.empty()) {
    if (qs.per_glob_rows) {
      C.res->alloc_rows(1);
      C.res->ts[0] = -1;
      C.res->val[0] = -1.0;
      C.res->glob[0] = 0;
      C.res->gid[0] = 0;
    }
    C.res->stats = "{\"scan_ms\":0,\"total_ms\":0,\"rows_scanned\":0,\"algorithmic_bytes\":0,\"tiles\":0,\"cells\":0}";
    return true;
  }
  // fieldName without fieldType: generateSql throws inside toGlobResultSet's try (BaseExpr.scala:355-356,
  // Commons.scala:228-253), so every glob is empty and the call succeeds -- no segment is read (every rank alike)
  if (qs.fchart && !C.R.field_type) {
    C.res->per_glob = qs.per_glob_rows;
    C.res->stats = "{\"scan_ms\":0,\"total_ms\":0,\"rows_scanned\":0,\"algorithmic_bytes\":0,\"tiles\":0,\"cells\":0,"
                 "\"segments\":0,\"general_segments\":0,\"field_chart\":\"no fieldType\"}";
    return true;
  }
  return false;
}

void plan_filter(const EvalCall& C, const QueryShape& qs, FilterPlan& fp) { plan_filter(C.R, qs, fp); }

void load_segments(const EvalCall& C, const QueryShape& qs, GlobPlan& gp) {
  // ---- segments: which ones this process evaluates ----
  gp.world = C.dist ? comm_world(C.E) : 1;
  gp.rank = C.dist ? comm_rank(C.E) : 0;
  std::vector<char> mine(C.n_paths, 1);
  if (C.dist)
    for (size_t i = 0; i < C.n_paths; i++) mine[i] = (C.shard ? C.shard[i] : int32_t(i % size_t(gp.world))) == gp.rank;
  gp.segs.resize(C.n_paths);
  // A segment the worker cannot read (missing file, corrupt Parquet, a file shape the loader does not take) fails
  // its glob's DuckDB query, which Commons.toGlobResultSet turns into an empty result for that glob alone
  // (Commons.scala:249-253, 338-340): such segments are marked here and empty their glob in plan_globs.
  gp.seg_bad.assign(C.n_paths, 0);
  // A rank-local failure of the engine itself (HIP, HBM, host memory) must not leave the other ranks waiting in the
  // next collective: the ranks agree on a status first and fail together (folded into the glob-union exchange
  // of plan_globs: one all-gather carries both).
  try {
    for (size_t i = 0; i < C.n_paths; i++) {
      if (!mine[i]) continue;
      try {
        gp.segs[i] = C.E.get_segment(C.paths[i], true);
      } catch (const PlanError& e) {
        // only the file's own faults (missing, unreadable, corrupt) empty its glob; an engine capability gap
        // (LK_ERR_UNSUPPORTED) or an evicted put key (LK_ERR_EVICTED) fails the call
        if (e.code != LK_ERR_IO) throw;
        gp.seg_bad[i] = 1;
        if (gp.bad_msg.empty()) gp.bad_msg = e.what();
      }
    }
  } catch (const PlanError& e) {
    if (!C.dist) throw;
    gp.load_err = e.code;
    gp.load_msg = e.what();
  } catch (const std::exception& e) {
    if (!C.dist) throw;
    gp.load_err = LK_ERR_DEVICE;
    gp.load_msg = e.what();
  }
  // A tag query over a numeric tag column (INT32 / INT64 / FLOAT / DOUBLE / BOOLEAN in a loaded segment): the values are
  // grouped and printed by the row scan's TAGNUM mode (exemplar.cpp).  Distributed: agreed on with the glob unions.
  gp.tag_numeric = false;
  if (qs.tagq)
    for (size_t i = 0; i < C.n_paths && !gp.tag_numeric; i++) {
      if (!gp.segs[i]) continue;
      const int c = gp.segs[i]->col_index(C.R.tag_name);
      gp.tag_numeric = c >= 0 && !gp.segs[i]->cols[size_t(c)].is_string;
    }
}

namespace {
// A groupBy that may become a numeric group dimension: not the name, and no string leaf on it (a string leaf keeps
// the string role: DuckDB's cast of its literal is unpinned, a numeric file empties the glob as before).
bool numeric_gb_candidate(const EvalCall& C, const QueryShape& qs, const std::string& gb) {
  if (qs.tagq || gb == kName) return false;
  return std::none_of(qs.all_leaves.begin(), qs.all_leaves.end(),
                      [&](const FilterNode* l) { return l->k == gb && !numeric_op(l->op); });
}
bool numeric_dim_type(int ptype) { return ptype == pq::BOOLEAN || value_rank(ptype) != 0; }
size_t glob_count(const EvalCall& C) { return (C.n_paths + size_t(C.glob_size) - 1) / size_t(C.glob_size); }

// One loaded file's class of candidate groupBy `gb` into its glob's (absent, or of a type the loader does not decode
// -- refused in plan_globs: no class).
void add_file_class(GbClass& c, const Segment& S, const std::string& gb) {
  const int col = S.col_index(gb);
  if (col >= 0) gb_class_add(c, S.cols[size_t(col)].is_string, S.cols[size_t(col)].ptype);
}
}  // namespace

std::vector<std::string> numeric_gb_candidates(const EvalCall& C, const QueryShape& qs) {
  std::vector<std::string> out;
  for (const std::string& gb : C.R.group_bys)
    if (std::find(out.begin(), out.end(), gb) == out.end() && numeric_gb_candidate(C, qs, gb)) out.push_back(gb);
  return out;
}

// Numeric group dimensions.  BaseExpr.getChartSql writes `GROUP BY step_ts, "<col>", name`
// (BaseExpr.scala:338-346, 401-403) and DuckDB groups a BIGINT / DOUBLE / BOOLEAN column like any other, each value
// printed by JDBC getString (Commons.scala:430-437): a groupBy-only column (or one with gt/ge/lt/le leaves) that some
// loaded file stores as INT32 / INT64 / FLOAT / DOUBLE / BOOLEAN becomes a numeric query column whose values the row
// scan discovers (XMODE_NUMDIM) and looks up.  The unions this engine does not restate fail the whole call.
// `cls`: [candidate][glob] classes -- this process's files, or what the ranks of a distributed call agreed on
// (plan_globs), which every rank then decides alike and refuses with the same text.
void decide_numeric_group_bys(const EvalCall& C, QueryShape& qs, const std::vector<std::string>& cands,
                              const std::vector<GbClass>& cls) {
  const size_t ng = glob_count(C);
  const std::string over = C.dist ? ", over the ranks of this distributed evaluation" : "";
  for (size_t ci = 0; ci < cands.size(); ci++) {
    const std::string& gb = cands[ci];
    auto refuse = [&](const std::string& why) { throw PlanError(LK_ERR_UNSUPPORTED, "numeric groupBy: column " + gb + " " + why); };
    bool any_num = false, any_text = false;
    long text_glob = -1, num_glob = -1;
    for (size_t gi = 0; gi < ng; gi++) {
      const GbClass& c = cls[ci * ng + gi];
      const std::string gs = std::to_string(gi);
      switch (gb_class_union(c, nullptr)) {
        case GB_TEXT_WITH_NUMBER: refuse("is VARCHAR in some files and numeric in others of glob " + gs + over); break;
        case GB_BOOLEAN_WITH_NUMBER: refuse("is BOOLEAN in some files and numeric in others of glob " + gs + over); break;
        case GB_OK: break;
      }
      if (c.text) any_text = true, text_glob = long(gi);
      if (c.numeric()) any_num = true, num_glob = long(gi);
    }
    if (!any_num) continue;   // a string groupBy, or a column no loaded file has
    if (any_text)
      refuse("is VARCHAR in glob " + std::to_string(text_glob) + " and numeric in glob " + std::to_string(num_glob) + " of the same call" + over);
    if ((C.flags & kEvalMetricsPct) || (qs.ces && C.R.dataset == "metrics"))
      refuse("is numeric; metrics p<NN> / ces take no numeric groupBy");
    if (qs.numgbs.size() >= size_t(MAXND)) refuse("is numeric: more than " + std::to_string(MAXND) + " numeric groupBys");
    qs.numgbs.push_back(gb);
    if (std::find(qs.nums.begin(), qs.nums.end(), gb) == qs.nums.end()) qs.nums.push_back(gb);
    qs.numeric = true;   // every segment takes the general row scan
  }
}

// Before the filter's string columns are listed.  One process: decided from its loaded files.  Distributed: the classes
// are agreed on in plan_globs, whose all-gather needs a filter plan first -- so this pass decides from the request alone
// (every rank alike, no rank-local refusal ahead of the collective): a groupBy is taken as a string column, unless a
// gt/ge/lt/le leaf reads it (plan_filter would refuse the column in both roles); evaluate_once plans again from the
// agreed classes wherever they, or such a leaf, say the first pass may be wrong (dist_numeric_replan).
void plan_numeric_group_bys(const EvalCall& C, QueryShape& qs, const GlobPlan& gp) {
  const std::vector<std::string> cands = numeric_gb_candidates(C, qs);
  if (C.dist) {
    for (const std::string& gb : cands)
      if (std::find(qs.nums.begin(), qs.nums.end(), gb) != qs.nums.end()) qs.numgbs.push_back(gb);
    return;
  }
  const size_t ng = glob_count(C);
  std::vector<GbClass> cls(cands.size() * ng);
  for (size_t ci = 0; ci < cands.size(); ci++)
    for (size_t j = 0; j < C.n_paths; j++)
      if (gp.segs[j]) add_file_class(cls[ci * ng + j / size_t(C.glob_size)], *gp.segs[j], cands[ci]);
  decide_numeric_group_bys(C, qs, cands, cls);
}

bool dist_numeric_replan(const EvalCall& C, const QueryShape& qs, const GlobPlan& gp) {
  if (!C.dist) return false;
  if (!qs.numgbs.empty()) return true;   // the first pass took a leafed groupBy as numeric: the files decide
  return std::any_of(gp.gb_class.begin(), gp.gb_class.end(), [](const GbClass& c) { return c.numeric(); });
}

// The second pass of a distributed call: the loaded segments stay, everything plan_globs filled starts over.
void reset_glob_plan(GlobPlan& gp) {
  GlobPlan fresh;
  fresh.world = gp.world;
  fresh.rank = gp.rank;
  fresh.segs = std::move(gp.segs);
  fresh.seg_bad = std::move(gp.seg_bad);
  fresh.bad_msg = std::move(gp.bad_msg);
  fresh.tag_numeric = gp.tag_numeric;
  gp = std::move(fresh);   // (releases the FieldTab lock the first pass may hold)
}

void plan_globs(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, GlobPlan& gp) {
  // ---- globs ----
  gp.fset = field_set(C.R);
  gp.probe_cols.assign(gp.fset.begin(), gp.fset.end());   // columns whose existence matters
  for (auto& k : qs.tagq ? std::vector<std::string>{kTimestamp, C.R.tag_name}
                      : (qs.no_value_col ? std::vector<std::string>{kTimestamp, kName}
                                      : std::vector<std::string>{kTimestamp, kName, qs.vcol}))
    if (std::find(gp.probe_cols.begin(), gp.probe_cols.end(), k) == gp.probe_cols.end()) gp.probe_cols.push_back(k);
  for (auto* l : qs.all_leaves)
    if (std::find(gp.probe_cols.begin(), gp.probe_cols.end(), l->k) == gp.probe_cols.end()) gp.probe_cols.push_back(l->k);
  for (size_t i = 0; i < C.n_paths; i += size_t(C.glob_size)) {
    GlobInfo g;
    for (size_t j = i; j < std::min(C.n_paths, i + size_t(C.glob_size)); j++) g.segs.push_back(int(j));
    gp.globs.push_back(std::move(g));
  }
  // Per glob: the union of columns (over the probe columns), "this glob's query fails" (a segment that did not load,
  // or a column whose type the query cannot use), the union_by_name type of the value column, and "value column may
  // be NULL".  Layout: [globs x np exists | globs fail | globs value-type rank | value NULLs].
  const size_t np = gp.probe_cols.size();
  const size_t ng = gp.globs.size();
  // [.. | value NULLs | numeric tag column | globs: a numeric file of the chart field | globs: a VARCHAR file of it]
  // [.. | candidate groupBys x globs: the column's class over the glob's files, 3 bytes (GbClass)]
  const std::vector<std::string> cands = numeric_gb_candidates(C, qs);
  gp.exists.assign(ng * np + 2 * ng + 2 + 2 * ng + cands.size() * ng * kGbClassBytes, 0);
  const size_t vnull_at = ng * np + 2 * ng;
  const size_t gbclass_at = vnull_at + 2 + 2 * ng;
  std::vector<GbClass> cls(cands.size() * ng);
  gp.num_ut.assign(qs.numgbs.size(), std::vector<int>(ng, -1));
  gp.exists[vnull_at + 1] = gp.tag_numeric ? 1 : 0;
  uint8_t* gfnum = gp.exists.data() + vnull_at + 2;
  uint8_t* gftext = gfnum + ng;
  // Field chart over a VARCHAR field: the column's dictionary as doubles (FieldTab), extended to the dictionary's size
  // now -- every segment of this call is loaded, so its ids lie below it
  // A referenced column this engine does not decode (Segment::unloaded) fails the call with LK_ERR_UNSUPPORTED: DuckDB
  // would read it, so the shim must fall back rather than see an empty glob.  Rank-local (it depends on
  // this rank's segments): agreed on with the load status below.
  std::vector<std::string> ref_cols(gp.probe_cols);
  for (auto& sc : fp.cols) ref_cols.push_back(sc.name);
  for (auto& nm : qs.nums) ref_cols.push_back(nm);
  uint8_t* gfail = gp.exists.data() + ng * np;
  uint8_t* gvrank = gfail + ng;
  for (size_t gi = 0; gi < ng; gi++)
    for (int si : gp.globs[gi].segs) {
      if (gp.seg_bad[si]) gfail[gi] = 1;
      if (!gp.segs[si]) continue;
      const Segment& S = *gp.segs[si];
      for (size_t k = 0; k < np; k++)
        if (S.all_columns.count(gp.probe_cols[k])) gp.exists[gi * np + k] = 1;
      // a failure of the call that depends on this rank's segments: agreed on with the load status below
      auto fail_call = [&](const std::string& m) {
        if (gp.load_err) return;
        if (!C.dist) throw PlanError(LK_ERR_UNSUPPORTED, m);
        gp.load_err = LK_ERR_UNSUPPORTED;
        gp.load_msg = m;
      };
      if (!S.unloaded.empty() && !gp.load_err)
        for (auto& c : ref_cols) {
          auto u = S.unloaded.find(c);
          if (u == S.unloaded.end()) continue;
          fail_call(u->second + " (" + S.key + ")");
          break;
        }
      int vc = S.col_index(qs.vcol);
      // a NULL value anywhere (or no value column): a glob cell may hold only NULLs and read back 0.0
      if (vc < 0 || S.cols[vc].any_nulls) gp.exists[vnull_at] = 1;
      // Column types per role.  read_parquet(union_by_name=True) (Commons.scala:213) unifies each column's type
      // over the glob's files; a column the query cannot bind (the value column as text, a string filter /
      // groupBy column stored as a number, a numeric comparison on text, INT96 / FIXED_LEN_BYTE_ARRAY, which the
      // engine does not load) makes DuckDB fail the glob's SQL -> that glob is empty (Commons.scala:249-253).
      auto bad = [&](const std::string& name, int role) -> bool {
        if (!S.all_columns.count(name)) return false;   // absent: nonExistentFields / NULL, not an error
        const int c = S.col_index(name);
        if (c < 0) return true;
        const HostCol& hc = S.cols[size_t(c)];
        if (role == 0) return hc.ptype != pq::INT64 && hc.ptype != pq::INT32;   // BIGINT over INT32 / INT64 files
        if (role == 2) return !hc.is_string;
        return value_rank(hc.ptype) == 0;   // value column / numeric comparison column
      };
      if (bad(kTimestamp, 0)) gfail[gi] = 1;
      if (qs.fchart) {
        // The chart field per file: numeric (unified over the glob as the value column is) or VARCHAR (try_cast of
        // its text); BOOLEAN -- and a VARCHAR value this engine does not cast -- fail the call, never a glob alone.
        if (vc >= 0 && S.cols[size_t(vc)].is_string) {
          gftext[gi] = 1;
          gp.exists[vnull_at] = 1;   // text that casts to NULL: a cell may hold no value
          try {
            if (!gp.ftab) {
              gp.ftab = C.E.field_tab(qs.vcol);
              gp.ftab_guard = std::unique_lock<std::mutex>(gp.ftab->mu);
              GlobalDict& gd = C.E.dict(qs.vcol);
              {
                std::lock_guard<std::mutex> g(gd.mu);
                gp.ftab_n = uint32_t(gd.size());
              }
              extend_field_tab(*gp.ftab, gd, gp.ftab_n);
            }
            std::string badv;
            if (!gp.load_err && !segment_text_ok(C.E, S, vc, *gp.ftab, &badv))
              fail_call("field chart: " + qs.vcol + " holds '" + json_escape(badv) + "', neither a plain number nor text that casts to NULL (" + S.key + ")");
          } catch (const PlanError& e) {
            if (!C.dist) throw;
            if (!gp.load_err) {
              gp.load_err = e.code;
              gp.load_msg = e.what();
            }
          }
        } else if (vc >= 0 && value_rank(S.cols[size_t(vc)].ptype)) {
          gfnum[gi] = 1;
          gvrank[gi] = std::max<uint8_t>(gvrank[gi], uint8_t(value_rank(S.cols[size_t(vc)].ptype)));
        } else if (S.all_columns.count(qs.vcol)) {   // BOOLEAN (an unloaded physical type was refused above)
          fail_call("field chart: column " + qs.vcol + " is neither numeric nor VARCHAR (" + S.key + ")");
        }
      } else if (!qs.no_value_col) {
        if (bad(qs.vcol, 1)) {
          // sum / avg over a VARCHAR value column is DuckDB's Binder Error (empty glob); count / min / max over it
          // run in DuckDB and this engine does not implement them: the call fails (LK_ERR_UNSUPPORTED)
          if (vc >= 0 && S.cols[size_t(vc)].is_string && qs.agg != AGG_SUM && qs.agg != AGG_AVG)
            fail_call("aggregation over the VARCHAR value column " + qs.vcol + " (" + S.key + ")");
          gfail[gi] = 1;
        }
        else if (vc >= 0) gvrank[gi] = std::max<uint8_t>(gvrank[gi], uint8_t(value_rank(S.cols[size_t(vc)].ptype)));
      }
      for (auto& sc : fp.cols)
        if (bad(sc.name, 2)) gfail[gi] = 1;
      for (auto& nm : qs.nums) {
        const int k = qs.numgb_index(nm);
        const int c = k >= 0 ? S.col_index(nm) : -1;
        if (c >= 0 && numeric_dim_type(S.cols[size_t(c)].ptype) && !S.cols[size_t(c)].is_string) {
          // a BOOLEAN group column binds; a comparison leaf on it stays a glob failure
          const int pt = S.cols[size_t(c)].ptype;
          const bool leafed = std::any_of(qs.all_leaves.begin(), qs.all_leaves.end(), [&](const FilterNode* l) { return l->k == nm; });
          if (pt == pq::BOOLEAN && !leafed) continue;
        }
        if (bad(nm, 3)) gfail[gi] = 1;
      }
      // which groupBys are numeric, and of which union type, depends on every rank's segments: the classes travel
      // with the unions, and their element-wise max over the ranks is union_by_name
      for (size_t ci = 0; ci < cands.size(); ci++) add_file_class(cls[ci * ng + gi], S, cands[ci]);
    }
  for (size_t i = 0; i < cls.size(); i++) {
    uint8_t* b = gp.exists.data() + gbclass_at + i * kGbClassBytes;
    b[0] = cls[i].text, b[1] = cls[i].boolean, b[2] = cls[i].rank;
  }
  // every rank sees every glob's union, failures and value type; a rank-local engine failure fails every rank here
  if (C.dist) comm_agree_max_u8(C.E, C.X, gp.load_err, gp.load_msg, gp.exists.data(), gp.exists.size());
  for (size_t i = 0; i < cls.size(); i++) {
    const uint8_t* b = gp.exists.data() + gbclass_at + i * kGbClassBytes;
    cls[i] = GbClass{b[0], b[1], b[2]};
  }
  gp.gb_cands = cands;
  gp.gb_class = cls;
  // the numeric group columns' union_by_name type per glob, from the agreed classes alone: a rank holding only an INT32
  // file of a glob whose DOUBLE file is another rank's keys and prints its values as DOUBLE
  for (size_t k = 0; k < qs.numgbs.size(); k++) {
    const size_t ci = size_t(std::find(cands.begin(), cands.end(), qs.numgbs[k]) - cands.begin());
    for (size_t gi = 0; gi < ng && ci < cands.size(); gi++) {
      int ut = -1;
      if (gb_class_union(cls[ci * ng + gi], &ut) == GB_OK && ut != pq::BYTE_ARRAY) gp.num_ut[k][gi] = ut;
    }
  }
  gp.value_nulls = gp.exists[vnull_at] != 0;
  if (qs.fchart)
    for (size_t gi = 0; gi < ng; gi++) {
      // union_by_name of a numeric and a VARCHAR file makes the column VARCHAR, the numbers printed as text: refused
      if (gfnum[gi] && gftext[gi])
        throw PlanError(LK_ERR_UNSUPPORTED, "field chart: column " + qs.vcol + " is numeric in some files and VARCHAR in others of glob " + std::to_string(gi));
      gp.ftext_any = gp.ftext_any || gftext[gi];
    }
  gp.tag_numeric = gp.exists[vnull_at + 1] != 0;   // agreed: a numeric tag column on some rank
  if (gp.tag_numeric) return;
  for (size_t gi = 0; gi < ng; gi++)
    if (gfail[gi]) {
      gp.globs[gi].skip = true;
      gp.nfailed++;
    }
  for (size_t gi = 0; gi < gp.globs.size(); gi++) {
    GlobInfo& g = gp.globs[gi];
    const SegmentReq& head = C.R.segments[g.segs[0]];
    g.step = head.step;
    g.query_tags = head.query_tags;
    g.win_lo = INT64_MAX;
    g.win_hi = INT64_MIN;
    for (int si : g.segs) {
      g.win_lo = std::min(g.win_lo, C.R.segments[si].start_ts);
      g.win_hi = std::max(g.win_hi, C.R.segments[si].end_ts);
    }
    // nonExistentFields (Commons.scala:224) -> leaves compiled to `false`
    std::set<std::string> nonexist;
    for (auto& f : gp.fset)
      if (!gp.has(gi, f)) nonexist.insert(f);
    for (auto& l : fp.leaves)
      if (nonexist.count(l.node->k)) g.leaf_false |= 1u << l.index;
    // Binder Error: referenced column absent from the whole glob
    if (qs.tagq) {
      if (!gp.has(gi, kTimestamp) || !gp.has(gi, C.R.tag_name)) g.skip = true;   // SELECT "<tag>": Binder Error
    } else if (!gp.has(gi, kTimestamp) || !gp.has(gi, kName) || (!qs.no_value_col && !gp.has(gi, qs.vcol))) {
      g.skip = true;
    }
    for (auto& l : fp.leaves)
      if (!nonexist.count(l.node->k) && !gp.has(gi, l.node->k)) g.skip = true;
    for (auto& k : fp.bad_literal)   // normalizedValue failed for a field this glob has
      if (!nonexist.count(k)) g.skip = true;
    // a regex leaf RE2 rejects fails the SQL of every glob where its field exists (where it does not, the leaf is
    // the literal `false` and the pattern is never compiled, BaseExpr.scala:462-464)
    for (auto& l : fp.leaves)
      if (fp.bad_regex[size_t(l.index)] && !nonexist.count(l.node->k)) g.skip = true;
    // (`<string column> > 1.5`, a Binder Error -> empty glob, is among the column-type failures of the segment loop)
    if (qs.tagq) continue;
    if (g.step <= 0) throw PlanError(LK_ERR_ARG, "stepInMillis must be positive");
    if (gp.step < 0) gp.step = g.step;
    else if (g.step != gp.step) throw PlanError(LK_ERR_DEVICE, "internal: globs with different steps (evaluate splits them)");
  }

  // A tag query's single bucket: ts - ts % 2^62 = 0 for every |ts| < 2^62, so bucket_base = 0 and one bucket.
  if (qs.tagq) gp.step = int64_t(1) << 62;
  // metrics off the step grid: one bucket per millisecond, i.e. the raw timestamp (see evaluate())
  if ((C.redo & REDO_METRICS_RAW) && C.R.dataset == "metrics" && !qs.tagq) gp.step = 1;
}

void cell_policy(const EvalCall& C, const QueryShape& qs, const GlobPlan& gp, CellSpace& cs) {
  // Merged min/max over values that can be NULL: NULL, "null" and "" group values stay apart in the table
  // (each is its own DuckDB group, and an all-NULL group reads back 0.0); they collapse after per-glob
  // finalization (rekey_minmax).  Everywhere else they can share a cell.
  // MIN re-run (REDO_MIN_APART): a DuckDB group whose values are all NaN has MIN = NaN, and query-api's math.min of
  // the globs' rows (TimeGroupedSketchAggregator.scala:79-88) -- or of a glob's NULL / "null" / "" groups, which share
  // an output key -- is then NaN; cells shared in the table would lose it (NaN orders above every number), so they stay
  // apart exactly as for NULL values.
  cs.min_max_nulls = (qs.agg == AGG_MIN || qs.agg == AGG_MAX) && (gp.value_nulls || (C.redo & REDO_MIN_APART));
  cs.collapse_in_table = qs.merged && !cs.min_max_nulls;
  cs.per_glob_cells = qs.per_glob_rows || cs.min_max_nulls;
  cs.collapse = qs.merged && C.R.group_bys.empty() && !qs.tagq;
}

void plan_dims(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, DimPlan& dp) {
  dp.dims.assign(fp.cols.size() + qs.numgbs.size(), DimCol{});
  // numeric group dimensions: sized once the discovery pass has listed their values (eval.cpp: discover_numdims)
  for (size_t k = 0; k < qs.numgbs.size(); k++) {
    DimCol& dc = dp.dims[fp.cols.size() + k];
    dc.is_dim = dc.restricted = dc.numeric = true;
    dc.ndim = 1;
    dc.dim_null = 0;
  }
  for (size_t s = 0; s < fp.cols.size(); s++) {
    const LeafCol& sc = fp.cols[s];
    DimCol& dc = dp.dims[s];
    dc.is_dim = (s == 0) || std::find(fp.gbs.begin(), fp.gbs.end(), sc.name) != fp.gbs.end();
    GlobalDict& gd = C.E.dict(sc.name);
    {
      std::lock_guard<std::mutex> g(gd.mu);
      dc.dict_n = uint32_t(gd.size());
    }
    if (!dc.is_dim) continue;
    if (restricted_values(C.R.filter.get(), sc.name, dc.cand)) {
      dc.restricted = true;
      // A passing row holds one of the candidates (the filter is `col IN cand AND ...`): NULL / absent / other
      // values never reach a cell, so the absent slot is needed only where a null-like candidate ("" / "null")
      // is itself folded into it.  Without it the dim has cand.size() ids and dim_null is past them (C5: the
      // name dim of `:eq name` no longer doubles the 10M-group cell space).
      const bool nl_cand = std::any_of(dc.cand.begin(), dc.cand.end(), [](const std::string& v) { return null_like(v); });
      dc.ndim = uint32_t(dc.cand.size()) + ((nl_cand || dc.cand.empty()) ? 1u : 0u);
      dc.dim_null = uint32_t(dc.cand.size());
    } else if (C.dist) {
      // Every rank holds its own engine dictionary: the dim space is the agreed union of the ranks' value keys
      // (dims.cpp), cached while no rank's dictionary changes.
      double ms = 0;
      bool rebuilt = false;
      dc.uni = agree_dim_union(C.E, C.X, sc.name, dc.dict_n, ms, rebuilt);
      dp.dims_ms += ms;
      dp.dims_rebuilt += rebuilt ? 1 : 0;
      dc.exchanged = true;
      dc.ndim = dc.uni->size + 1;
      dc.dim_null = dc.uni->size;
    } else {
      if (dc.dict_n + 1 > DIM_MASK) throw PlanError(LK_ERR_UNSUPPORTED, "group dimension too large");
      dc.ndim = dc.dict_n + 1;
      dc.dim_null = dc.dict_n;
    }
  }
  plan_strides(dp);
}

void plan_strides(DimPlan& dp) {
  dp.ngroups = 1;
  for (int s = int(dp.dims.size()) - 1; s >= 0; s--) {
    if (!dp.dims[s].is_dim) continue;
    dp.dims[s].stride = dp.ngroups;
    dp.ngroups *= dp.dims[s].ndim;
    if (dp.ngroups > 0xffffffffull) throw PlanError(LK_ERR_UNSUPPORTED, "group space beyond 2^32 groups");
  }
}

void plan_tables(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, const GlobPlan& gp, const CellSpace& cs,
                 DimPlan& dp) {
  // ---- lookup tables: global id -> leaf bits << 24 | dim id ----
  dp.tabs.assign(fp.cols.size(), {});
  dp.need_tab.assign(fp.cols.size(), 0);
  for (size_t s = 0; s < fp.cols.size(); s++) {
    const LeafCol& sc = fp.cols[s];
    DimCol& dc = dp.dims[s];
    GlobalDict& gd = C.E.dict(sc.name);
    bool null_like_present;
    {
      std::lock_guard<std::mutex> g(gd.mu);
      null_like_present = gd.ids.count("null") || gd.ids.count("");
    }
    dp.need_tab[s] = !sc.leaves.empty() || dc.restricted || dc.exchanged ||
                  (dc.is_dim && cs.collapse_in_table && null_like_present) || (!dc.is_dim && sc.leaves.empty());
    // an agreed union dim without leaves reads its global id -> dim id table straight from HBM (built once with the
    // agreement), unless null-like values must fold into dim_null in this query's table
    if (dc.exchanged && sc.leaves.empty() && !(cs.collapse_in_table && null_like_present) && dc.uni->d_dim_of_gid)
      dp.need_tab[s] = false;
    if (!dp.need_tab[s]) continue;
    // Leaf outcomes over the column's dictionary (values [0, dict_n) are immutable: StableStrs), cached per
    // (column, leaves) and extended only over values added since: a regex runs once per distinct value.
    LockedLeafBits cached;
    if (!sc.leaves.empty()) {
      std::vector<char> skip_leaf(sc.leaves.size(), 0);   // a rejected pattern: every glob it could run in is empty
      for (size_t j = 0; j < sc.leaves.size(); j++) skip_leaf[j] = char(fp.bad_regex[sc.lbase + j]);
      cached = extend_leaf_bits(C.E, sc, gd, dc.dict_n, &skip_leaf);
    }
    const LeafBits* lb = cached.lb.get();
    auto& tab = dp.tabs[s];
    tab.resize(std::max<uint32_t>(dc.dict_n, 1));
    for (uint32_t gid = 0; gid < dc.dict_n; gid++) {
      const std::string& v = gd[gid];
      const uint32_t bits = lb ? lb->hit[gid] : 0u;
      uint32_t dim = 0;
      if (dc.is_dim) {
        if (dc.restricted) {
          auto it = std::find(dc.cand.begin(), dc.cand.end(), v);
          dim = it == dc.cand.end() ? dc.dim_null : uint32_t(it - dc.cand.begin());
          if (cs.collapse_in_table && null_like(v)) dim = dc.dim_null;
        } else {
          dim = (cs.collapse_in_table && null_like(v)) ? dc.dim_null : (dc.exchanged ? dc.exchanged_dim(gid) : gid);
        }
      }
      tab[gid] = (bits << 24) | dim;
    }
  }
  if (cs.collapse && dp.dims[0].is_dim) {
    // "tags of the first input" (TimeGroupedSketchAggregator.scala:57-60) is arrival-order dependent in the
    // reference; we pick the smallest name string among the merged cells, deterministically.
    // Order = the row's resulting tag map as a sorted (key, value) list: {"name": v}, or the first glob's
    // queryTags when the name is NULL / "null" / "" (Commons.scala:433, 450-452).
    using TagList = std::vector<std::pair<std::string, std::string>>;
    TagList qt = gp.globs[0].query_tags;
    std::sort(qt.begin(), qt.end());
    std::vector<std::pair<TagList, uint32_t>> order;
    GlobalDict& gd = C.E.dict(kName);
    std::lock_guard<std::mutex> g(gd.mu);
    for (uint32_t d = 0; d < dp.dims[0].ndim; d++) {
      const std::string_view v = d == dp.dims[0].dim_null ? std::string_view() : dp.dims[0].dim_value(d, gd);
      if (!null_like(v)) order.emplace_back(TagList{{"name", std::string(v)}}, d);
      else order.emplace_back(qt, d);
    }
    std::sort(order.begin(), order.end());
    dp.name_rank.assign(dp.dims[0].ndim, 0);
    for (uint32_t r = 0; r < order.size(); r++) dp.name_rank[order[r].second] = r;
  }
}

void plan_cells(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, const GlobPlan& gp, const DimPlan& dp,
                CellSpace& cs) {
  // ---- bucket space ----
  int64_t min_lo = INT64_MAX;
  for (auto& g : gp.globs) {
    if (g.skip) continue;
    min_lo = std::min(min_lo, g.win_lo);
    cs.max_hi = std::max(cs.max_hi, g.win_hi);
  }
  if (min_lo < cs.max_hi) {
    if (qs.metrics) cs.bucket_base = min_lo;
    else cs.bucket_base = min_lo - min_lo % gp.step;
    int64_t last = cs.max_hi - 1;
    int64_t last_b = qs.metrics ? last : last - last % gp.step;
    cs.nbuckets = uint64_t((last_b - cs.bucket_base) / gp.step + 1);
  }
  // dims whose null-like values must be folded after per-glob finalization
  cs.fold_maps.assign(dp.dims.size(), {});   // (a numeric dimension's texts are never null-like: no map)
  if (qs.merged && cs.min_max_nulls && !fp.gbs.empty()) {
    for (size_t s = 0; s < fp.cols.size(); s++) {
      const DimCol& dc = dp.dims[s];
      if (!dc.is_dim) continue;
      GlobalDict& gd = C.E.dict(fp.cols[s].name);
      std::lock_guard<std::mutex> g(gd.mu);
      std::vector<uint32_t> m(dc.ndim);
      bool any = false;
      for (uint32_t d = 0; d < dc.ndim; d++) {
        m[d] = d;
        if (d == dc.dim_null) continue;
        if (null_like(dc.dim_value(d, gd))) { m[d] = dc.dim_null; any = true; }
      }
      if (any) { cs.fold_maps[s] = std::move(m); cs.rekey = true; }
    }
  }
  cs.nslots = cs.per_glob_cells ? uint32_t(gp.globs.size()) : 1u;
  if (cs.nbuckets && (double(cs.nslots) * double(cs.nbuckets) * double(dp.ngroups) > 9.0e18))
    throw PlanError(LK_ERR_UNSUPPORTED, "cell key space beyond 64 bits");
  cs.ncells = uint64_t(cs.nslots) * cs.nbuckets * dp.ngroups;
}

void plan_truth(const EvalCall& C, const QueryShape& qs, FilterPlan& fp) { plan_truth(C.R, qs, fp); }

void plan_segments(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, const GlobPlan& gp, const CellSpace& cs,
                   SegPlan& sg) {
  // ---- per-segment query descriptors ----
  // `qsegs` go to the fused kernels (scan_lean / scan_tiles: INT64 timestamps, DOUBLE values); `gsegs` to the general
  // row scan (ex_scan AGG mode): every segment of a numeric-leaf query, and segments whose timestamp or value column
  // needs union_by_name promotion (INT32 timestamps; INT32 / INT64 / FLOAT values, cast through FLOAT where the glob's
  // value type is FLOAT).  Both kinds aggregate into the same table.
  // scan_clu's query shape (clu_kernel.hpp): one string column, the name, filtered through a truth table; SUM, MIN,
  // MAX, COUNT or AVG (scanned as SUM with the row counts, setup_scan) of `_cardinalhq.value` with no value leaf, sketch
  // or cardinality estimate; buckets on the step grid.
  // LK_NO_CLUSTER=1 (read per call: A/B) sends every segment down the other kernels, as do the switches that turn
  // off the machinery it relies on.
  const bool clu_query = fp.cols.size() == 1 && !qs.tagq && fp.cols[0].name == kName && !fp.truth.empty() &&
                         (qs.agg == AGG_SUM || qs.agg == AGG_MIN || qs.agg == AGG_MAX || qs.agg == AGG_COUNT ||
                          qs.agg == AGG_AVG) && !qs.sketch && !qs.ces &&
                         !qs.numeric && !fp.vleaf && qs.nums.empty() && qs.numgbs.empty() && !qs.metrics && !qs.fchart &&
                         !qs.no_value_col && qs.vcol == kValue && gp.step > 0 && !getenv("LK_NO_CLUSTER") &&
                         !getenv("LK_NO_LEAN_SPLIT") && !getenv("LK_NO_SPLIT");
  try {
  for (size_t gi = 0; gi < gp.globs.size() && cs.nbuckets; gi++) {
    const GlobInfo& g = gp.globs[gi];
    if (g.skip) continue;
    const int vunion = value_type_of_rank(gp.gvrank()[gi]);   // the glob's union_by_name value type (-1: no value column)
    for (int si : g.segs) {
      if (!gp.segs[si]) continue;
      const Segment& S = *gp.segs[si];
      sg.rows_scanned += uint64_t(S.num_rows);
      QSeg q{};
      q.base = S.d_data;
      q.tiles = S.d_tiles;
      q.ntiles = uint32_t(S.tiles.size());
      q.glob_slot = cs.per_glob_cells ? uint32_t(gi) : 0;
      q.leaf_false = g.leaf_false;
      q.win_lo = g.win_lo;
      q.win_hi = g.win_hi;
      // (a field chart with a VARCHAR glob: every segment takes the row scan, whose `rows` count only rows with a
      // field -- the fused kernels' `rows` count NULL fields too, and one table holds one meaning)
      bool general = (qs.numeric && !fp.vleaf) || gp.ftext_any;
      // (column types were checked per glob in plan_globs: a type the query cannot bind emptied the glob)
      auto bind = [&](int qc, const std::string& name, bool want_string) {
        int c = S.col_index(name);
        if (c < 0) {
          if (S.all_columns.count(name))
            throw PlanError(LK_ERR_DEVICE, "internal: column " + name + " of an unloaded type in a live glob");
          return;
        }
        const HostCol& hc = S.cols[c];
        if (want_string != hc.is_string)
          throw PlanError(LK_ERR_DEVICE, "internal: column " + name + " of an unexpected type in a live glob");
        uint32_t pad = uint32_t(hc.ptype);
        if (const int k = qc >= 2 ? qs.numgb_index(name) : -1; k >= 0)   // a numeric group column: the glob's union type
          pad |= uint32_t(gp.num_ut[size_t(k)][gi]) << 8;
        if (qc == 0 && hc.ptype != pq::INT64) general = true;   // INT32 timestamps: sign-extended
        if (qc == 1) {
          if (hc.ptype != pq::DOUBLE) general = true;
          // an integer value column in a glob whose value type is FLOAT is cast to FLOAT first (DuckDB's implicit
          // BIGINT -> FLOAT of the union column), then aggregated as a float
          if (vunion == pq::FLOAT && hc.ptype != pq::FLOAT) pad |= VCONV_VIA_FLOAT;
          if (hc.is_string) pad |= VCONV_TEXT;   // a field chart's VARCHAR field: the row scan reads FieldTab
          if (hc.int_abs_max < 0.0) sg.vals_integral = false;
          sg.vals_abs_max = std::max(sg.vals_abs_max, hc.int_abs_max);
          sg.vals_rows += double(S.num_rows);
        }
        q.cols[qc] = QCol{hc.d_pages, hc.d_runs, hc.d_tcols, hc.d_remap, 1u, pad};
        sg.alg_bytes += hc.compressed_bytes;
      };
      bind(0, kTimestamp, false);
      if (!q.cols[0].present) continue;            // no timestamps: every row fails the window
      // COUNT(*) / metrics `ces` read no value column; a field chart's field may be VARCHAR (the whole glob then is)
      if (!qs.no_value_col) bind(1, qs.vcol, qs.fchart && gp.gftext()[gi] != 0);
      for (size_t s = 0; s < fp.cols.size(); s++) bind(2 + fp.dev_of[s], fp.cols[s].name, true);
      for (size_t n = 0; n < qs.nums.size(); n++) bind(int(2 + fp.cols.size() + n), qs.nums[n], false);
      // scan_lean takes every tile of this segment when no page of its three columns holds a NULL and every
      // name page has a small dictionary (lean_tile's test at page granularity)
      bool seg_lean = !general;
      if (seg_lean) {
        const int ct = S.col_index(kTimestamp), cv = qs.no_value_col ? -1 : S.col_index(qs.vcol);
        const int cn = fp.cols.size() <= 3 ? S.col_index(fp.cols[size_t(fp.lead)].name) : -1;
        seg_lean = ct >= 0 && (cv >= 0 || qs.no_value_col) && cn >= 0 && !S.cols[ct].any_nulls &&
                   (qs.no_value_col || !S.cols[cv].any_nulls) &&
                   !S.cols[cn].any_nulls;
        for (size_t s2 = 0; s2 < fp.cols.size() && seg_lean; s2++) {   // late columns: absent, or NULL-free dictionaries
          if (int(s2) == fp.lead) continue;
          const int cl = S.col_index(fp.cols[s2].name);
          if (cl < 0) continue;
          if (S.cols[cl].any_nulls || !S.cols[cl].pages_lean_late) seg_lean = false;
        }
        if (seg_lean && !S.cols[cn].pages_lean_name) seg_lean = false;
      }
      // vleaf: only scan_lean tests the value leaves -- a segment it does not take whole goes to the general row scan.
      // Not in p<NN> / ces calls: their scan_tiles (the COUNT instantiations) tests the leaves too, so the segment stays
      // fused -- p<NN>: scan_tiles takes every tile; ces: scan_lean the lean tiles, scan_tiles the rest
      if (fp.vleaf && (!seg_lean || !fp.vleaf_shape) && !(qs.sketch || qs.ces)) general = true;
      if (!general) sg.all_lean = sg.all_lean && seg_lean;
      // scan_clu takes the segment whole: its copy was built from these two columns, covers every tile, and every
      // tile that meets the window is pinned or split (clu.hpp) -- no other kernel then runs over the segment
      if (clu_query && !general && seg_lean && S.d_clu && S.clu_name_col == S.col_index(kName) &&
          S.clu_val_col == S.col_index(kValue) && !(q.cols[1].pad & (VCONV_VIA_FLOAT | VCONV_TEXT)) &&
          clu_segment_taken(S.clu_all_sorted, S.clu_widest, gp.step)) {
        q.clu = S.d_clu_desc;
        q.clu_base = S.d_clu;
        q.clu_sub = S.d_clu_sub;
        q.clu_sub_stride = S.clu_sub_stride;
        // the sample tables (this timestamp column's) lie in front of the area, in its allocation
        if (S.d_clu_sub && S.clu_sub_shared && S.d_ts_samp && S.ts_samp_col == S.col_index(kTimestamp))
          q.clu_samp_back = uint32_t(S.d_clu_sub - S.d_ts_samp);
      }
      q.tile_begin = sg.total_tiles;
      sg.seg_begin.push_back(sg.total_tiles);
      sg.total_tiles += q.ntiles;
      (general ? sg.gsegs : sg.qsegs).push_back(q);
      if (general) sg.gseg_glob.push_back(uint32_t(gi));
    }
  }

  if (sg.seg_begin.size() > 65535) throw PlanError(LK_ERR_UNSUPPORTED, "more than 65535 segments in one evaluation");
  if (sg.total_tiles >= (1u << 31)) throw PlanError(LK_ERR_UNSUPPORTED, "too many tiles");
  } catch (const PlanError& e) {
    if (!C.dist) throw;
    sg.local_err = e.code;
    sg.local_msg = e.what();
    sg.qsegs.clear();
    sg.gsegs.clear();
    sg.gseg_glob.clear();
    sg.total_tiles = 0;
  }
  for (auto& q : sg.qsegs) sg.max_tiles = std::max(sg.max_tiles, q.ntiles);
  for (auto& q : sg.gsegs) sg.gmax_tiles = std::max(sg.gmax_tiles, q.ntiles);
}

void plan_table_mode(const QueryShape& qs, const SegPlan& sg, CellSpace& cs) {
  // ---- table mode ----
  // Dense: array index = cell key = (glob slot, bucket, group).  Hash (SURVEY §2.2 K4 spill, high cardinality):
  // an open-addressing table keyed by the cell key, first sized from a bound on the distinct cells and grown
  // (the scan re-run) when the bound was optimistic.  Every passing row lands in one cell, so the distinct cells
  // never exceed the rows scanned.
  const uint64_t dense_max = getenv("LK_DENSE_MAX_CELLS") ? uint64_t(atoll(getenv("LK_DENSE_MAX_CELLS")))
                                                          : (uint64_t(1) << 26);
  cs.hash_mode = qs.sketch || qs.ces || cs.ncells > dense_max;   // sketch keys: (cell, bin), sparse
  if (qs.sketch && double(cs.ncells) * double(DD_NBINS) > 9.0e18) throw PlanError(LK_ERR_UNSUPPORTED, "sketch key space beyond 64 bits");
  auto pow2 = [](uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
  };
  const double key_space = double(cs.ncells) * (qs.sketch ? double(DD_NBINS) : 1.0);   // distinct keys <= both
  const uint64_t hash_bound = std::max<uint64_t>(1, key_space < double(sg.rows_scanned) ? uint64_t(key_space) : sg.rows_scanned);
  cs.cap_max = std::max<uint64_t>(pow2(2 * hash_bound), 1 << 16);
  cs.cap = cs.hash_mode ? std::min<uint64_t>(cs.cap_max, std::max<uint64_t>(1 << 16, std::min<uint64_t>(pow2(2 * hash_bound), 1 << 25))) : 0;
  if (cs.hash_mode && getenv("LK_HASH_INIT_SLOTS"))   // tests only: a deliberately small first table (regrowth path)
    cs.cap = std::min<uint64_t>(cs.cap_max, pow2(std::max<uint64_t>(64, uint64_t(atoll(getenv("LK_HASH_INIT_SLOTS"))))));
}

void plan_cluster(const CellSpace& cs, SegPlan& sg) {
  if (cs.hash_mode)   // scan_clu merges into dense tables only
    for (auto& q : sg.qsegs) q.clu = nullptr, q.clu_base = nullptr, q.clu_sub = nullptr, q.clu_sub_stride = 0, q.clu_samp_back = 0;
  sg.n_clu = 0;
  if (std::none_of(sg.qsegs.begin(), sg.qsegs.end(), [](const QSeg& q) { return q.clu != nullptr; })) return;
  // (stable: each kind keeps its order; QSeg::tile_begin is a statistic, no kernel indexes by it)
  const auto mid = std::stable_partition(sg.qsegs.begin(), sg.qsegs.end(), [](const QSeg& q) { return q.clu == nullptr; });
  sg.n_clu = uint32_t(sg.qsegs.end() - mid);
}

}  // namespace lk
