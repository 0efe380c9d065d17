// lk_eval_formula: a formula over DataExprs (a / b * 100) for one SegmentGroup, combined on the device.
//
// Restates QueryEngineV2.evaluateFormula (query-api/src/main/scala/com/cardinal/queryapi/engine/QueryEngineV2.scala:
// 310-389):
//   * every base expression the formula uses is evaluated as evaluateBaseExpr does (QueryEngineV2.scala:271-308) -- here
//     one merged evaluation each (LK_MERGED), whose finalized rows stay on the device (kEvalKeepDevice, eval.cpp);
//   * each result row becomes a MAP sketch {sum: value} (QueryEngineV2.scala:344-357) and the formula, with every base
//     expression's aggregation set to `sum` (367-371), is evaluated through astEvalFlow (eval/EvalUtils.scala:27-37):
//     BaseExpr.eval (utils/ast/BaseExpr.scala:665-695) therefore runs twice on a leaf, so the chart transformer
//     (ASTUtils.getTransformerFunc, ASTUtils.scala:190-219) is applied twice to a leaf's value -- a `rate` chart with a
//     60 s step divides by 60 twice -- and the per-key collapse runs twice (idempotent);
//   * per timestamp, Formula.eval joins the sides by group key (Formula.scala:32-69; formula_cell.hpp).
// On this engine an operand's rows are (bucket, group id) with group ids over engine-wide dictionaries, so the join is
// a keyed combine: cell = bucket x union group, the union built per groupBy column over the operands' dimension values
// (O(dims) on the host, never O(rows)).  Only the combined rows cross the host link.
//
// Deterministic stand-ins for what is hash-iteration order in the reference:
//   1. rows of one expression at one timestamp that share a group key collapse to the row with the smallest sorted tag
//      list (eval_merged_rows' rule);
//   2. keys are compared as the tuple of group values, absent read as "" (ASTUtils.toGroupByKey, ASTUtils.scala:87-89,
//      joins them with ":");
//   3. a constant's tags under groupBys are those of the first expression, in the order of `expressions`, that has a
//      row at that key and timestamp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "comm.hpp"
#include "engine.hpp"
#include "evalutil.hpp"
#include "formula.hpp"
#include "formula_kernels.hpp"
#include "hostutil.hpp"
#include "json.hpp"
#include "plan.hpp"

namespace lk {

int evaluate(Engine& E, const std::string& json, const char* const* paths, size_t n_paths, int glob_size,
             unsigned flags, const int32_t* shard, bool dist, lk_result* res);
int evaluate_keep_device(Engine& E, const std::shared_ptr<const Request>& Rp, const char* const* paths, size_t n_paths,
                         int glob_size, const int32_t* shard, bool dist, lk_result* res);
int evaluate_comm_held(Engine& E, const std::string& json, const char* const* paths, size_t n_paths, int glob_size,
                       const int32_t* shard, lk_result* res);

namespace {

void dump_json(const Json& j, std::string& o) {
  switch (j.kind) {
    case Json::Null: o += "null"; break;
    case Json::Bool: o += j.b ? "true" : "false"; break;
    case Json::Number: o += j.num_text; break;
    case Json::String: {
      o += '"';
      for (char c : j.str) {
        if (c == '"' || c == '\\') {
          o += '\\';
          o += c;
        } else if (static_cast<unsigned char>(c) < 0x20) {
          char b[8];
          snprintf(b, sizeof(b), "\\u%04x", unsigned(static_cast<unsigned char>(c)));
          o += b;
        } else {
          o += c;
        }
      }
      o += '"';
      break;
    }
    case Json::Array: {
      o += '[';
      for (size_t i = 0; i < j.arr.size(); i++) {
        if (i) o += ',';
        dump_json(j.arr[i], o);
      }
      o += ']';
      break;
    }
    case Json::Object: {
      o += '{';
      for (size_t i = 0; i < j.obj.size(); i++) {
        if (i) o += ',';
        Json key;
        key.kind = Json::String;
        key.str = j.obj[i].first;
        dump_json(key, o);
        o += ':';
        dump_json(j.obj[i].second, o);
      }
      o += '}';
      break;
    }
  }
}

std::string lower_trim(std::string s) {
  size_t a = 0, b = s.size();
  while (a < b && isspace(static_cast<unsigned char>(s[a]))) a++;
  while (b > a && isspace(static_cast<unsigned char>(s[b - 1]))) b--;
  s = s.substr(a, b - a);
  for (char& c : s) c = char(tolower(static_cast<unsigned char>(c)));
  return s;
}

// ASTUtils.getTransformerFunc (ASTUtils.scala:190-219) as one IEEE operation: identity, x secs or / secs, with
// ChartType.fromStr (model/query/common/ChartType.scala:41-47; default "count", ASTUtils.scala:350) and
// MetricType.fromStr (MetricType.scala:65-73; default gauge, ASTUtils.scala:298-303).
int transformer_of(const Request& R, const Json& base_expr, const std::string& var) {
  const std::string ct = lower_trim(R.has_chart ? R.chart_type : "count");
  if (ct != "count" && ct != "rate") throw PlanError(LK_ERR_ARG, "formula: " + var + ": unknown chart type " + R.chart_type);
  std::string mt = "gauge";
  if (const Json* m = base_expr.get("metricType"); m && m->is_str()) mt = lower_trim(m->str);
  if (mt == "count") mt = "counter";
  if (mt != "rate" && mt != "counter" && mt != "gauge" && mt != "histogram")
    throw PlanError(LK_ERR_ARG, "formula: " + var + ": unknown metric type " + mt);
  if (R.dataset == "metrics") {
    if (ct == "count" && mt == "rate") return FX_XF_MUL;
    if (ct == "rate" && mt == "counter") return FX_XF_DIV;
    return FX_XF_NONE;
  }
  return ct == "rate" ? FX_XF_DIV : FX_XF_NONE;
}

// dim id -> tag text of a name / groupBy tag column (lk_result::own_tag_gid for one dim id); nullptr: the tag is absent
const char* dim_text(const lk_result::TagCol& t, uint32_t d) {
  if (t.hidden) return nullptr;
  if (d == t.dim_null) return t.null_value;
  if (t.shared) return (*t.shared)[d];
  if (!t.local.empty()) return t.local[d];
  const std::string& s = (*t.dict)[t.order ? t.order->perm[d] : d];
  return (s.empty() || s == "null") ? nullptr : s.c_str();
}

struct Operand {
  std::string var;
  std::shared_ptr<const Request> R;
  std::vector<std::string> paths;
  std::vector<int32_t> shard;   // distributed: the rank of every path ("shard"); empty: i % world
  std::shared_ptr<lk_result> res;
  bool uploaded = false;
  int xform = FX_XF_NONE;
  std::vector<int> key_col;   // per key column: the operand's tag column
  int64_t ts_lo = 0, ts_hi = 0;
};

using TagList = std::vector<std::pair<std::string, std::string>>;

}  // namespace

// Distributed (lk_eval_formula_dist; DESIGN.md §7.6 "Distributed"): a rank is a pod.  Every operand is one sharded merged
// evaluation whose rows land on rank 0 (kept on its device, or uploaded by it), the join runs on rank 0 alone.  comm_mu is
// held for the whole call; the operands run in ascending byte order of their variable names, each closed by one
// agreement of the ranks' outcomes, so every rank issues the same collectives and all fail at the same operand.
// Everything decided before the first collective -- the parser, the gate, the shard check -- reads the request alone.
int evaluate_formula(Engine& E, const std::string& json, int glob_size, bool dist, lk_result* res) {
  const auto t_start = std::chrono::steady_clock::now();
  if (glob_size <= 0) glob_size = 10;
  Json top = Json::parse(json);
  const Json* ftext = top.get("formula");
  const Json* exprs = top.get("expressions");
  if (!ftext || !ftext->is_str()) throw PlanError(LK_ERR_ARG, "formula: missing \"formula\"");
  if (!exprs || !exprs->is_obj()) throw PlanError(LK_ERR_ARG, "formula: missing \"expressions\"");
  std::vector<std::string> names;
  for (auto& kv : exprs->obj) names.push_back(kv.first);

  // ---- parse; leaves renumbered over the referenced expressions, in the order of `expressions` ----
  FxProgram prog;
  {
    std::string err;
    const int rc = parse_formula(ftext->str, names, prog, err);
    if (rc) throw PlanError(rc, err);
  }
  std::vector<int> leaf_of(names.size(), -1);
  std::vector<Operand> ops;
  for (size_t v = 0; v < names.size(); v++) {
    bool used = false;
    for (int i = 0; i < prog.n; i++) used = used || (prog.ops[i].op == FX_LEAF && prog.ops[i].leaf == int32_t(v));
    if (!used) continue;
    leaf_of[v] = int(ops.size());
    ops.emplace_back();
    ops.back().var = names[v];
  }
  for (int i = 0; i < prog.n; i++)
    if (prog.ops[i].op == FX_LEAF) prog.ops[i].leaf = leaf_of[size_t(prog.ops[i].leaf)];
  if (ops.size() > size_t(FX_MAXLEAF))
    throw PlanError(LK_ERR_UNSUPPORTED, "formula: more than " + std::to_string(FX_MAXLEAF) + " expressions referenced");

  const int world = dist ? comm_world(E) : 1, rank = dist ? comm_rank(E) : 0;
  char fstats[512];
  auto finish_empty = [&]() {
    res->exemplar = true;
    snprintf(fstats, sizeof(fstats),
             "{\"scan_ms\":0,\"total_ms\":%.6f,\"rows_scanned\":0,\"cells\":0,\"formula\":{\"mode\":\"dense\",\"cells\":0,"
             "\"operands_on_device\":0,\"operands_uploaded\":0,\"regrows\":0,\"world\":%d,\"rank\":%d,\"operands\":[]}}",
             ms_since(t_start), world, rank);
    res->stats = fstats;
    return int(LK_OK);
  };
  if (ops.empty()) return finish_empty();   // no variable: no SketchGroup reaches the formula, no rows

  // ---- gate (every rule depends on the requests alone) ----
  auto refuse = [](const std::string& why) { throw PlanError(LK_ERR_UNSUPPORTED, "formula: " + why); };
  std::vector<std::string> key_cols;   // the groupBy set, sorted (toGroupByKey sorts, ASTUtils.scala:87-89)
  int64_t step = 0;
  for (size_t k = 0; k < ops.size(); k++) {
    Operand& o = ops[k];
    const Json& ex = *exprs->get(o.var);
    const Json* pd = ex.get("pushDown");
    if (!pd || !pd->is_obj()) throw PlanError(LK_ERR_ARG, "formula: expression " + o.var + " has no pushDown");
    std::string text;
    dump_json(*pd, text);
    o.R = E.parse_cached(text);
    if (const Json* ps = ex.get("paths"); ps && ps->is_arr())
      for (auto& p : ps->arr) o.paths.push_back(p.scalar_text());
    if (o.paths.size() != o.R->segments.size())
      throw PlanError(LK_ERR_ARG, "formula: expression " + o.var + ": paths must match segmentRequests");
    if (const Json* sh = ex.get("shard"); dist && sh && sh->kind != Json::Null) {
      if (!sh->is_arr() || sh->arr.size() != o.paths.size())
        throw PlanError(LK_ERR_ARG, "formula: expression " + o.var + ": shard must have one rank per path");
      for (auto& v : sh->arr) {
        const int64_t r = v.as_i64();
        if (r < 0 || r >= world)
          throw PlanError(LK_ERR_ARG, "formula: expression " + o.var + ": shard rank " + std::to_string(r) + " outside the world");
        o.shard.push_back(int32_t(r));
      }
    }
    const Request& R = *o.R;
    if (R.is_tag_query) refuse("expression " + o.var + " is a tag query");
    if (!R.has_chart) refuse("expression " + o.var + " has no chart (an exemplar query has no value to combine)");
    if (R.has_extract || R.has_compute) refuse("expression " + o.var + " uses extract / compute");
    const bool pct = R.aggregation.size() > 1 && R.aggregation[0] == 'p';
    if (pct && R.dataset == "metrics" && !R.field_chart())
      refuse("expression " + o.var + ": metrics percentiles are assembled per row on the host");
    std::vector<std::string> gb = R.group_bys;
    std::sort(gb.begin(), gb.end());
    gb.erase(std::unique(gb.begin(), gb.end()), gb.end());
    if (k == 0) key_cols = gb;
    else if (gb != key_cols)
      refuse("expressions " + ops[0].var + " and " + o.var + " have different groupBy sets");
    for (auto& s : R.segments) {
      if (s.step <= 0) throw PlanError(LK_ERR_ARG, "formula: expression " + o.var + ": stepInMillis must be positive");
      if (step && s.step != step) throw PlanError(LK_ERR_ARG, "formula: the expressions' steps differ");
      step = s.step;
    }
    o.xform = transformer_of(R, *pd->get("baseExpr"), o.var);
    // values assembled on the host (DDSketch quantiles, HLL estimates): evaluated as usual, then uploaded
    o.uploaded = pct || R.aggregation == "ces" || (R.rollup.find("ces") != std::string::npos && R.dataset != "metrics");
  }
  if (key_cols.size() > size_t(FX_MAXCOL))
    refuse("more than " + std::to_string(FX_MAXCOL) + " groupBy columns");
  const double secs = double(step / 1000);   // the Long quotient stepInMillis / 1000 (ASTUtils.scala:192)

  if (dist && !E.comm) throw PlanError(LK_ERR_ARG, "lk_comm_init has not been called");

  // ---- operands: merged rows (ts, value, group id) on the device ----
  unsigned long long rows_scanned = 0;
  double scan_ms = 0;
  size_t n_dev = 0, n_up = 0;
  // evaluated in ascending byte order of the variable names: the order of a distributed call's collectives must not
  // depend on how a rank's caller ordered the JSON object (leaf numbers and a constant's tags keep reading `expressions`)
  std::vector<size_t> order(ops.size());
  for (size_t k = 0; k < ops.size(); k++) order[k] = k;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return ops[a].var < ops[b].var; });
  std::unique_lock<std::mutex> comm_lock;
  if (dist) comm_lock = std::unique_lock<std::mutex>(E.comm_mu);   // one hold over every operand's collectives
  std::string op_stats;   // "operands": per variable, in evaluation order
  for (size_t k : order) {
    Operand& o = ops[k];
    o.res = std::make_shared<lk_result>();
    std::vector<const char*> pp;
    for (auto& p : o.paths) pp.push_back(p.c_str());
    const int32_t* shard = o.shard.empty() ? nullptr : o.shard.data();
    auto run = [&] {
      if (o.uploaded) {
        std::string text;
        dump_json(*exprs->get(o.var)->get("pushDown"), text);
        if (dist) evaluate_comm_held(E, text, pp.data(), pp.size(), glob_size, shard, o.res.get());
        else evaluate(E, text, pp.data(), pp.size(), glob_size, LK_MERGED, nullptr, false, o.res.get());
      } else {
        evaluate_keep_device(E, o.R, pp.data(), pp.size(), glob_size, shard, dist, o.res.get());
      }
    };
    if (!dist) {
      run();
    } else {
      // The operand's closing agreement.  Its own collectives fail every rank together; what a rank meets alone behind
      // the last of them (rank 0 folding the gathered tables, placing the kept rows) is agreed on here, so no rank
      // starts the next operand's collectives while another unwinds.  Every rank passes the `merge` fault point.
      int code = 0;
      std::string msg;
      try {
        run();
        fault_point(E, "merge");
      } catch (const PlanError& e) {
        code = e.code, msg = e.what();
      } catch (const JsonError& e) {
        code = LK_ERR_ARG, msg = e.what();
      } catch (const std::bad_alloc&) {
        code = LK_ERR_MEMORY, msg = "out of host memory";
      } catch (const std::exception& e) {
        code = LK_ERR_DEVICE, msg = e.what();
      }
      CtxLease X(E);
      X->pend_code = 0;
      X->pend_msg.clear();
      comm_agree(E, *X, code, msg.empty() ? std::string() : "formula: expression " + o.var + ": " + msg);
    }
    (o.uploaded ? n_up : n_dev)++;
    std::string reduce = "none";
    if (!o.res->stats.empty()) {
      try {
        Json st = Json::parse(o.res->stats);
        if (const Json* x = st.get("rows_scanned")) rows_scanned += (unsigned long long)x->as_i64();
        if (const Json* x = st.get("scan_ms")) scan_ms += x->num;
        if (const Json* x = st.get("reduce"); x && x->is_str()) reduce = x->str;
      } catch (const JsonError&) {
      }
    }
    op_stats += std::string(op_stats.empty() ? "" : ",") + "{\"var\":\"" + json_escape(o.var) + "\",\"reduce\":\"" + json_escape(reduce) +
                "\",\"rows\":" + std::to_string(o.res->nrows) + ",\"kept\":" + (o.uploaded ? "false" : "true") + "}";
  }
  const std::string fx_tail = ",\"world\":" + std::to_string(world) + ",\"rank\":" + std::to_string(rank) + ",\"operands\":[" + op_stats + "]}}";
  // Behind the last operand's last collective: from here a failure unwinds this rank alone.  The other ranks return
  // their empty result; rank 0 looks at the rows for the first time.
  if (rank != 0) {
    res->exemplar = true;
    char b0[384];
    snprintf(b0, sizeof(b0),
             "{\"scan_ms\":%.6f,\"total_ms\":%.6f,\"rows_scanned\":%llu,\"cells\":0,\"operand_rows\":0,\"formula\":{\"mode\":\"dense\","
             "\"cells\":0,\"operands_on_device\":%zu,\"operands_uploaded\":%zu,\"regrows\":0",
             scan_ms, ms_since(t_start), rows_scanned, n_dev, n_up);
    res->stats = b0 + fx_tail;
    return LK_OK;
  }
  HIP_TRY(hipSetDevice(E.device));
  for (Operand& o : ops) {
    lk_result& r = *o.res;
    if (r.exemplar) refuse("expression " + o.var + ": rows with per-row tags");
    if (r.nrows > 0xffffffffull) refuse("expression " + o.var + " has 2^32 rows or more");
    if (!r.nrows) continue;
    const size_t n = r.nrows;
    if (o.uploaded) {
      HIP_TRY(hipMalloc(&r.dev_rows, n * 20 + 64));
      uint8_t* d = static_cast<uint8_t*>(r.dev_rows);
      HIP_TRY(hipMemcpy(d, r.ts, n * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(d + n * 8, r.val, n * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(d + n * 16, r.gid, n * 4, hipMemcpyHostToDevice));
      o.ts_lo = r.ts[0];
      o.ts_hi = r.ts[n - 1];
    } else {   // rows ascend in time: the first and the last timestamp bound the buckets
      const int64_t* dts = static_cast<const int64_t*>(r.dev_rows);
      HIP_TRY(hipMemcpy(&o.ts_lo, dts, 8, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(&o.ts_hi, dts + (n - 1), 8, hipMemcpyDeviceToHost));
    }
  }
  const double operands_ms = ms_since(t_start);

  // ---- result tag columns: the union of the operands' tag columns, in order of first appearance ----
  for (Operand& o : ops)
    for (auto& tn : o.res->tag_names)
      if (std::find(res->tag_names.begin(), res->tag_names.end(), tn) == res->tag_names.end()) res->tag_names.push_back(tn);
  res->exemplar = true;   // tags materialized per row (ex_tags): no bulk export of group ids

  int64_t base = INT64_MAX, last = INT64_MIN;
  size_t total_rows = 0;
  for (Operand& o : ops)
    if (o.res->nrows) {
      base = std::min(base, o.ts_lo);
      last = std::max(last, o.ts_hi);
      total_rows += o.res->nrows;
    }
  char buf[768];
  auto write_stats = [&](const char* mode, unsigned long long cells, int regrows, double scatter_ms, double eval_ms,
                         double transfer_ms, size_t out_rows) {
    snprintf(buf, sizeof(buf),
             "{\"scan_ms\":%.6f,\"total_ms\":%.6f,\"rows_scanned\":%llu,\"cells\":%llu,\"operand_rows\":%zu,"
             "\"operands_ms\":%.6f,\"scatter_ms\":%.6f,\"eval_ms\":%.6f,\"transfer_ms\":%.6f,\"link_bytes\":%zu,"
             "\"formula\":{\"mode\":\"%s\",\"cells\":%llu,\"operands_on_device\":%zu,\"operands_uploaded\":%zu,"
             "\"regrows\":%d",
             scan_ms, ms_since(t_start), rows_scanned, cells, total_rows, operands_ms, scatter_ms, eval_ms, transfer_ms,
             out_rows * 24, mode, cells, n_dev, n_up, regrows);
    res->stats = buf + fx_tail;
  };
  if (!total_rows) {
    write_stats("dense", 0, 0, 0, 0, 0, 0);
    return LK_OK;
  }

  // ---- union group space: per key column the union of the operands' dimension values; id 0 = absent ("") ----
  const size_t nk = key_cols.size();
  std::vector<std::unordered_map<std::string, uint32_t>> uni(nk);
  // A column every operand reads through the same engine dictionary (unrestricted groupBy, one generation) needs no
  // table: union id = dim id + 1, the absent ids (NULL, "", "null") read 0 -- a 10M-value column costs nothing here.
  // Values met outside the dictionary's dims (queryTags) take ids past them.
  std::vector<char> ident(nk, 0);
  std::vector<GlobalDict*> ident_gd(nk, nullptr);
  std::vector<uint32_t> ident_max(nk, 0), ident_nl0(nk, IdMap::kNone), ident_nl1(nk, IdMap::kNone);
  for (Operand& o : ops) {
    if (!o.res->nrows) continue;
    o.key_col.assign(nk, -1);
    for (size_t j = 0; j < nk; j++) {
      const auto& gbs = o.R->group_bys;
      const size_t at = size_t(std::find(gbs.begin(), gbs.end(), key_cols[j]) - gbs.begin());
      if (1 + at >= o.res->tcols.size()) throw PlanError(LK_ERR_DEVICE, "internal: groupBy column missing from the operand");
      o.key_col[j] = int(1 + at);
    }
  }
  for (size_t j = 0; j < nk; j++) {
    const StableStrs* dict = nullptr;
    bool ok = true, any = false;
    for (Operand& o : ops) {
      if (!o.res->nrows) continue;
      const lk_result::TagCol& t = o.res->tcols[size_t(o.key_col[j])];
      const bool plain = !t.hidden && !t.shared && t.local.empty() && !t.order && t.dict && !t.null_value &&
                         t.ndim <= 0xfffffff0ull && t.dim_null + 1 == t.ndim;
      ok = ok && plain && (!any || t.dict == dict);
      dict = t.dict;
      any = true;
      ident_max[j] = std::max<uint32_t>(ident_max[j], uint32_t(t.ndim));
    }
    if (!ok || !any) continue;
    GlobalDict& gd = E.dict(key_cols[j]);
    std::lock_guard<std::mutex> g(gd.mu);
    if (gd.vals.get() != dict) continue;   // (another generation: take the tables)
    ident[j] = 1;
    ident_gd[j] = &gd;
    ident_nl0[j] = gd.ids.find("");
    ident_nl1[j] = gd.ids.find("null");
  }
  auto union_id = [&](size_t j, const char* s) -> uint32_t {
    if (!s || !*s) return 0;
    if (ident[j]) {
      uint32_t id;
      {
        std::lock_guard<std::mutex> g(ident_gd[j]->mu);
        id = ident_gd[j]->ids.find(s);
      }
      if (id != IdMap::kNone && id + 1 < ident_max[j]) return id + 1;   // a dim id of the dictionary (not dim_null)
      auto it = uni[j].find(s);
      if (it != uni[j].end()) return it->second;
      const uint32_t nid = ident_max[j] + 1 + uint32_t(uni[j].size());
      uni[j].emplace(s, nid);
      return nid;
    }
    auto it = uni[j].find(s);
    if (it != uni[j].end()) return it->second;
    const uint32_t id = uint32_t(uni[j].size()) + 1;
    uni[j].emplace(s, id);
    return id;
  };
  std::vector<std::vector<std::vector<uint32_t>>> maps(ops.size(), std::vector<std::vector<uint32_t>>(nk));
  std::vector<std::vector<uint32_t>> name_rank(ops.size());
  std::vector<std::vector<uint32_t>> qt_ids(ops.size(), std::vector<uint32_t>(nk, 0));
  std::vector<uint32_t> qt_rank(ops.size(), 1);
  for (size_t k = 0; k < ops.size(); k++) {
    Operand& o = ops[k];
    const lk_result& r = *o.res;
    if (!r.nrows) continue;   // (an expression without rows -- no segments, an empty glob -- is absent everywhere)
    if (r.tcols.empty()) throw PlanError(LK_ERR_DEVICE, "internal: operand without tag columns");
    for (size_t j = 0; j < nk; j++) {
      if (ident[j]) continue;
      const lk_result::TagCol& tc = r.tcols[size_t(o.key_col[j])];
      if (tc.ndim > 0xffffffffull) refuse("group dimension too large");
      auto& m = maps[k][j];
      m.resize(size_t(tc.ndim));
      for (uint32_t d = 0; d < uint32_t(tc.ndim); d++) m[d] = union_id(j, dim_text(tc, d));
    }
    // the name dimension is not part of the key: its rank, by text, decides the collapse (2 * order + 4)
    const lk_result::TagCol& nc = r.tcols[0];
    std::vector<std::string> texts;
    std::vector<const char*> nt(size_t(nc.ndim), nullptr);
    for (uint32_t d = 0; d < uint32_t(nc.ndim); d++) {
      nt[d] = dim_text(nc, d);
      if (nt[d]) texts.emplace_back(nt[d]);
    }
    std::sort(texts.begin(), texts.end());
    texts.erase(std::unique(texts.begin(), texts.end()), texts.end());
    name_rank[k].assign(size_t(nc.ndim), FX_RANK_ABSENT);
    for (uint32_t d = 0; d < uint32_t(nc.ndim); d++)
      if (nt[d])
        name_rank[k][d] = 2u * uint32_t(std::lower_bound(texts.begin(), texts.end(), std::string(nt[d])) - texts.begin()) + 4u;
    // a row whose own tags are all absent takes its glob's queryTags (Commons.scala:450-452; merged rows: the first
    // glob's): its key reads the groupBy columns there, and its rank is its sorted tag list's place among the lists
    // of the named rows of that key (2 * place + 3), or past the key's row without a name tag (formula_kernels.hpp)
    TagList qt;
    if (!r.qt_of_glob.empty())
      for (auto& kv : r.qt_of_glob[0]) qt.emplace_back(r.tag_names[kv.first], kv.second ? kv.second : "");
    std::sort(qt.begin(), qt.end());
    TagList rest;   // the groupBy tags a named row of that key carries
    for (size_t j = 0; j < nk; j++) {
      std::string v;
      for (auto& kv : qt)
        if (kv.first == key_cols[j]) v = kv.second;
      qt_ids[k][j] = union_id(j, v.c_str());
      if (!v.empty()) rest.emplace_back(r.tag_names[size_t(o.key_col[j])], v);
    }
    std::sort(rest.begin(), rest.end());
    bool noname_last = false;   // as fx_scatter ranks the key's row without a name tag
    for (auto& kv : rest) noname_last = noname_last || kv.first > r.tag_names[0];
    uint32_t place = 0;   // (no queryTags: the empty list sorts first)
    for (auto& nm : texts) {
      if (qt.empty()) break;
      TagList l = rest;
      l.emplace_back(r.tag_names[0], nm);
      std::sort(l.begin(), l.end());
      if (l < qt) place++;
    }
    qt_rank[k] = 2u * place + 3u;
    if (!rest.empty()) {
      if (!noname_last && place == 0 && qt < rest) qt_rank[k] = 0u;
      if (noname_last && place == texts.size() && rest < qt) qt_rank[k] = FX_RANK_NONAME_LAST + 1u;
    }
  }
  std::vector<unsigned long long> ustride(nk, 1);
  unsigned long long U = 1;
  for (size_t j = nk; j-- > 0;) {
    ustride[j] = U;
    const unsigned long long n = (unsigned long long)uni[j].size() + 1 + (ident[j] ? ident_max[j] : 0);
    if (U > (~0ull) / n) refuse("the union group space does not fit in 64 bits");
    U *= n;
  }
  const unsigned long long nbuckets = (unsigned long long)((last - base) / step) + 1;
  if (nbuckets > (1ull << 26)) refuse("more than 2^26 buckets");
  if (U > (~0ull - 1) / nbuckets) refuse("the cell key (buckets x union groups) does not fit in 64 bits");
  const unsigned long long nkeys = nbuckets * U;

  // ---- device: tables, scatter, evaluate, write ----
  CtxLease X(E);
  hipStream_t st = X->stream;
  const int L = int(ops.size());
  // one staging block: per operand the key column maps and the name rank
  size_t tab_words = 0;
  for (size_t k = 0; k < ops.size(); k++) {
    for (auto& m : maps[k]) tab_words += m.size();
    tab_words += name_rank[k].size();
  }
  uint32_t* d_tabs = static_cast<uint32_t*>(X->workspace("fx_tabs", tab_words * 4 + 64));
  {
    std::vector<uint32_t> h;
    h.reserve(tab_words);
    for (size_t k = 0; k < ops.size(); k++) {
      for (auto& m : maps[k]) h.insert(h.end(), m.begin(), m.end());
      h.insert(h.end(), name_rank[k].begin(), name_rank[k].end());
    }
    if (!h.empty()) HIP_TRY(hipMemcpyAsync(d_tabs, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (h is pageable and leaves scope)
  }
  std::vector<FxOperand> fo(ops.size());
  {
    size_t off = 0;
    for (size_t k = 0; k < ops.size(); k++) {
      const lk_result& r = *ops[k].res;
      FxOperand& f = fo[k];
      memset(&f, 0, sizeof(f));
      f.leaf = int(k);
      if (!r.nrows) continue;
      const size_t n = r.nrows;
      const uint8_t* d = static_cast<const uint8_t*>(r.dev_rows);
      f.ts = reinterpret_cast<const int64_t*>(d);
      f.val = reinterpret_cast<const double*>(d + n * 8);
      f.gid = reinterpret_cast<const uint32_t*>(d + n * 16);
      f.nrows = uint32_t(n);
      f.leaf = int(k);
      f.ncols = int(nk);
      for (size_t j = 0; j < nk; j++) {
        const lk_result::TagCol& tc = r.tcols[size_t(ops[k].key_col[j])];
        f.stride[j] = tc.stride ? tc.stride : 1;
        f.ndim[j] = tc.ndim ? tc.ndim : 1;
        f.ustride[j] = ustride[j];
        f.map[j] = ident[j] ? nullptr : d_tabs + off;
        off += maps[k][j].size();
        f.dim_null[j] = tc.dim_null;
        f.nl0[j] = ident_nl0[j];
        f.nl1[j] = ident_nl1[j];
        if (r.tag_names[size_t(ops[k].key_col[j])] > r.tag_names[0]) f.after_name |= 1u << j;
        f.qt_u += (unsigned long long)qt_ids[k][j] * ustride[j];
      }
      f.name_stride = r.tcols[0].stride ? r.tcols[0].stride : 1;
      f.name_ndim = r.tcols[0].ndim ? r.tcols[0].ndim : 1;
      f.name_rank = d_tabs + off;
      off += name_rank[k].size();
      f.qt_rank = qt_rank[k];
    }
  }
  const bool dense = nkeys <= E.formula_dense_max_cells;
  unsigned long long ncells = nkeys;
  if (!dense) {
    unsigned long long want = E.formula_hash_slots ? E.formula_hash_slots : 2ull * total_rows;
    ncells = 64;
    while (ncells < want) ncells <<= 1;
  }
  int regrows = 0;
  FxTable T{};
  uint32_t* d_flags = static_cast<uint32_t*>(X->workspace("fx_flags", 64));
  const double t_scatter0 = ms_since(t_start);
  for (;;) {
    if (ncells > (1ull << 34) / (unsigned long long)L) throw PlanError(LK_ERR_MEMORY, "formula: cell table too large");
    uint8_t* tb = static_cast<uint8_t*>(X->workspace("fx_table", size_t(ncells) * 8 * size_t(L + (dense ? 0 : 1)) + 256));
    T.slots = reinterpret_cast<unsigned long long*>(tb);
    T.keys = dense ? nullptr : T.slots + ncells * (unsigned long long)L;
    T.ncells = ncells;
    T.U = U;
    T.nbuckets = nbuckets;
    T.base = base;
    T.step = step;
    T.flags = d_flags;
    T.live = d_flags + 1;
    T.nleaves = L;
    HIP_TRY(hipMemsetAsync(d_flags, 0, 64, st));
    HIP_TRY(launch_fx_fill(T.slots, ncells * (unsigned long long)(L + (dense ? 0 : 1)), st));
    for (auto& f : fo) HIP_TRY(launch_fx_scatter(T, f, st));
    uint32_t fl = 0;
    HIP_TRY(hipMemcpyAsync(&fl, d_flags, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (fl & FX_FLAG_OFFGRID) refuse("an expression's timestamps are off the step grid");
    if (fl & FX_FLAG_RANGE) throw PlanError(LK_ERR_DEVICE, "internal: formula cell outside the table");
    if (!(fl & FX_FLAG_FULL)) break;
    ncells <<= 2;   // a full hash table regrows and scatters again: no row is dropped
    regrows++;
  }
  const double scatter_ms = ms_since(t_start) - t_scatter0;

  FxEval V{};
  V.T = T;
  V.nops = prog.n;
  V.has_group_bys = nk ? 1 : 0;
  memcpy(V.ops, prog.ops, sizeof(FxOp) * size_t(prog.n));
  for (int l = 0; l < L; l++) {
    V.val[l] = fo[size_t(l)].val;
    V.gid[l] = fo[size_t(l)].gid;
    V.xform[l] = ops[size_t(l)].xform;
    V.secs[l] = secs;
  }
  const uint32_t nb = fx_blocks(ncells);
  uint32_t* d_counts = static_cast<uint32_t*>(X->workspace("fx_counts", (size_t(nb) + 2) * 4));
  if (!dense) {
    uint32_t* bc = static_cast<uint32_t*>(X->workspace("fx_buckets", (size_t(nbuckets) * 2 + 2) * 4));
    HIP_TRY(hipMemsetAsync(bc, 0, (size_t(nbuckets) * 2 + 2) * 4, st));
    V.bucket_count = bc;
    V.bucket_cursor = bc + nbuckets + 1;
  }
  HIP_TRY(launch_fx_eval_count(V, d_counts, st));
  uint32_t nout = 0;
  HIP_TRY(hipMemcpyAsync(&nout, d_counts + nb, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<int32_t> src_op(nout);
  std::vector<uint32_t> src_gid(nout);
  double eval_ms = 0, transfer_ms = 0;
  if (nout) {
    const size_t n = nout;
    uint8_t* ob = static_cast<uint8_t*>(X->workspace("fx_out", n * 24 + 64));
    int64_t* o_ts = reinterpret_cast<int64_t*>(ob);
    double* o_val = reinterpret_cast<double*>(ob + n * 8);
    int32_t* o_op = reinterpret_cast<int32_t*>(ob + n * 16);
    uint32_t* o_gid = reinterpret_cast<uint32_t*>(ob + n * 20);
    HIP_TRY(launch_fx_eval_write(V, d_counts, o_ts, o_val, o_op, o_gid, st));
    HIP_TRY(hipStreamSynchronize(st));
    eval_ms = ms_since(t_start) - t_scatter0 - scatter_ms;
    const double t1 = ms_since(t_start);
    res->alloc_rows(n, false);
    res->gid = nullptr;   // formula rows carry no group ids (lk_result_group_ids: NULL)
    HIP_TRY(hipMemcpyAsync(res->ts, o_ts, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(res->val, o_val, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(src_op.data(), o_op, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(src_gid.data(), o_gid, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    transfer_ms = ms_since(t_start) - t1;
  } else {
    res->alloc_rows(0, false);
    res->gid = nullptr;
  }

  // ---- tags from (source operand, source group id); the operands' device rows are done with ----
  for (Operand& o : ops) {
    if (o.res->dev_rows) (void)hipFree(o.res->dev_rows);
    o.res->dev_rows = nullptr;
  }
  const size_t ncol = res->tag_names.size();
  // (an operand names a column twice when a queryTags key is also a groupBy: the row's own tag, else the queryTag)
  std::vector<std::vector<std::vector<size_t>>> col_of(ops.size(), std::vector<std::vector<size_t>>(ncol));
  for (size_t k = 0; k < ops.size(); k++)
    for (size_t c = 0; c < ncol; c++) {
      auto& tn = ops[k].res->tag_names;
      for (size_t oc = 0; oc < tn.size(); oc++)
        if (tn[oc] == res->tag_names[c]) col_of[k][c].push_back(oc);
    }
  res->ex_tags.assign(size_t(nout) * ncol, nullptr);
  for (size_t r = 0; r < nout; r++) {
    const int32_t k = src_op[r];
    if (k < 0 || k >= L) continue;   // a constant's empty tags
    const lk_result& orow = *ops[size_t(k)].res;
    for (size_t c = 0; c < ncol; c++)
      for (size_t oc : col_of[size_t(k)][c]) {
        const char* v = orow.tag_of_gid(src_gid[r], oc);
        if (v) res->ex_tags[r * ncol + c] = v;   // (a later column of the same name overwrites, as a tag map does)
      }
  }
  for (Operand& o : ops) res->keep.push_back(o.res);   // the tag strings live in the operands' results
  write_stats(dense ? "dense" : "hash", dense ? nkeys : ncells, regrows, scatter_ms, eval_ms, transfer_ms, nout);
  return LK_OK;
}

}  // namespace lk
