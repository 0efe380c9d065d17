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
//
// This file is the stages that need the engine, the communicator or the device; what they decide from the request and
// from the dimensions' texts alone is formula_join.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "comm.hpp"
#include "engine.hpp"
#include "eval_plan.hpp"
#include "evalutil.hpp"
#include "formula.hpp"
#include "formula_join.hpp"
#include "formula_kernels.hpp"
#include "hostutil.hpp"
#include "json.hpp"
#include "plan.hpp"

namespace lk {

namespace {

// The call: its arguments, fixed while it runs.
struct FxRun {
  Engine& E;
  lk_result* res;
  std::chrono::steady_clock::time_point t_start;
  int glob_size;
  bool dist;
  int world, rank;
};

// One referenced expression while the call runs: its evaluation and its place in the join.
struct Operand {
  const FxExpr* x;
  std::shared_ptr<lk_result> res;
  std::vector<int> key_col;   // per key column: the operand's tag column
  int64_t ts_lo = 0, ts_hi = 0;
};

// What the call reports; the stages fill it as they go.
struct FxStats {
  enum Kind { NO_OPERANDS, OFF_ROOT, ROOT } kind = NO_OPERANDS;
  int world = 1, rank = 0;
  double scan_ms = 0;                      // the operands' totals
  unsigned long long rows_scanned = 0;
  size_t n_dev = 0, n_up = 0;
  std::string operands;                    // "operands": per variable, in evaluation order
  size_t operand_rows = 0;                 // rank 0: the rows it joins ...
  double operands_ms = 0;                  // ... and the time until they were placed
  const char* mode = "dense";              // the device join's outcome
  unsigned long long cells = 0;
  int regrows = 0;
  double scatter_ms = 0, eval_ms = 0, transfer_ms = 0;
  size_t out_rows = 0;
};

// The operands' rows on rank 0: the bucket range they span.
struct RowSpan {
  int64_t base = INT64_MAX, last = INT64_MIN;
  size_t total_rows = 0;
};

// The cell table after the scatter.
struct Scattered {
  FxTable T{};
  bool dense = true;
  unsigned long long ncells = 0;
  double t0 = 0;   // ms since the call's start when the scatter began
};

// The combined rows' sources, fetched: (source operand, source gid) per output row.
struct Joined {
  std::vector<int32_t> src_op;
  std::vector<uint32_t> src_gid;
};

std::string fixed6(double v) {
  char b[64];
  snprintf(b, sizeof(b), "%.6f", v);
  return b;
}

// The stats text of all three outcomes: no operand (NO_OPERANDS), a rank that joins nothing (OFF_ROOT), rank 0 (ROOT).
void write_stats(const FxRun& c, const FxStats& s) {
  std::string o = std::string("{\"scan_ms\":") + (s.kind == FxStats::NO_OPERANDS ? "0" : fixed6(s.scan_ms)) +
                  ",\"total_ms\":" + fixed6(ms_since(c.t_start)) + ",\"rows_scanned\":" + std::to_string(s.rows_scanned) +
                  ",\"cells\":" + std::to_string(s.cells);
  if (s.kind != FxStats::NO_OPERANDS) o += ",\"operand_rows\":" + std::to_string(s.operand_rows);
  if (s.kind == FxStats::ROOT)
    o += ",\"operands_ms\":" + fixed6(s.operands_ms) + ",\"scatter_ms\":" + fixed6(s.scatter_ms) + ",\"eval_ms\":" +
         fixed6(s.eval_ms) + ",\"transfer_ms\":" + fixed6(s.transfer_ms) + ",\"link_bytes\":" + std::to_string(s.out_rows * 24);
  o += std::string(",\"formula\":{\"mode\":\"") + s.mode + "\",\"cells\":" + std::to_string(s.cells) +
       ",\"operands_on_device\":" + std::to_string(s.n_dev) + ",\"operands_uploaded\":" + std::to_string(s.n_up) +
       ",\"regrows\":" + std::to_string(s.regrows) + ",\"world\":" + std::to_string(s.world) + ",\"rank\":" +
       std::to_string(s.rank) + ",\"operands\":[" + s.operands + "]}}";
  c.res->stats = o;
}

// ---- operands: merged rows (ts, value, group id) on the device ----
void evaluate_operand(const FxRun& c, Operand& o) {
  std::vector<const char*> pp;
  for (auto& p : o.x->paths) pp.push_back(p.c_str());
  const int32_t* shard = o.x->shard.empty() ? nullptr : o.x->shard.data();
  if (!o.x->uploaded)
    evaluate_keep_device(c.E, o.x->R, pp.data(), pp.size(), c.glob_size, shard, c.dist, o.res.get());
  else if (c.dist)
    evaluate_comm_held(c.E, o.x->push_down, pp.data(), pp.size(), c.glob_size, shard, o.res.get());
  else
    evaluate(c.E, o.x->push_down, pp.data(), pp.size(), c.glob_size, LK_MERGED, nullptr, false, o.res.get());
}

// A distributed operand with its closing agreement.  Its own collectives fail every rank together; what a rank meets
// alone behind the last of them (rank 0 folding the gathered tables, placing the kept rows) is agreed on here, so no
// rank starts the next operand's collectives while another unwinds.  Every rank passes the `merge` fault point.
void evaluate_operand_agreed(const FxRun& c, Operand& o) {
  int code = 0;
  std::string msg;
  try {
    evaluate_operand(c, o);
    fault_point(c.E, "merge");
  } catch (const PlanError& e) {
    code = e.code, msg = e.what();
  } catch (const JsonError& e) {
    code = LK_ERR_ARG, msg = e.what();
  } catch (const std::bad_alloc&) {
    code = LK_ERR_MEMORY, msg = "out of host memory";
  } catch (const std::exception& e) {
    code = LK_ERR_DEVICE, msg = e.what();
  }
  CtxLease X(c.E);
  X->pend_code = 0;
  X->pend_msg.clear();
  comm_agree(c.E, *X, code, msg.empty() ? std::string() : "formula: expression " + o.x->var + ": " + msg);
}

// Every operand, in the gate's evaluation order; a distributed call holds comm_mu over all of them.
void run_operands(const FxRun& c, const FxCall& call, std::vector<Operand>& ops, FxStats& st) {
  std::unique_lock<std::mutex> comm_lock;
  if (c.dist) comm_lock = std::unique_lock<std::mutex>(c.E.comm_mu);   // one hold over every operand's collectives
  for (size_t k : call.order) {
    Operand& o = ops[k];
    o.res = std::make_shared<lk_result>();
    if (c.dist) evaluate_operand_agreed(c, o);
    else evaluate_operand(c, o);
    (o.x->uploaded ? st.n_up : st.n_dev)++;
    st.rows_scanned += o.res->rows_scanned;
    st.scan_ms += o.res->scan_ms;
    st.operands += std::string(st.operands.empty() ? "" : ",") + "{\"var\":\"" + json_escape(o.x->var) + "\",\"reduce\":\"" +
                   json_escape(o.res->reduce) + "\",\"rows\":" + std::to_string(o.res->nrows) + ",\"kept\":" +
                   (o.x->uploaded ? "false" : "true") + "}";
  }
}

// Rank 0 looks at the rows for the first time: a host-assembled operand's rows are uploaded; the kept rows ascend in
// time, so their first and last timestamp bound the buckets.
void place_rows(const FxRun& c, std::vector<Operand>& ops) {
  HIP_TRY(hipSetDevice(c.E.device));
  for (Operand& o : ops) {
    lk_result& r = *o.res;
    if (r.exemplar) throw PlanError(LK_ERR_UNSUPPORTED, "formula: expression " + o.x->var + ": rows with per-row tags");
    if (r.nrows > 0xffffffffull) throw PlanError(LK_ERR_UNSUPPORTED, "formula: expression " + o.x->var + " has 2^32 rows or more");
    if (!r.nrows) continue;
    const size_t n = r.nrows;
    if (o.x->uploaded) {
      HIP_TRY(hipMalloc(&r.dev_rows, n * 20 + 64));
      uint8_t* d = static_cast<uint8_t*>(r.dev_rows);
      HIP_TRY(hipMemcpy(d, r.ts, n * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(d + n * 8, r.val, n * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(d + n * 16, r.gid, n * 4, hipMemcpyHostToDevice));
      o.ts_lo = r.ts[0];
      o.ts_hi = r.ts[n - 1];
    } else {
      const int64_t* dts = static_cast<const int64_t*>(r.dev_rows);
      HIP_TRY(hipMemcpy(&o.ts_lo, dts, 8, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(&o.ts_hi, dts + (n - 1), 8, hipMemcpyDeviceToHost));
    }
  }
}

// The result's tag columns: the union of the operands' tag columns, in order of first appearance; the span of the rows.
RowSpan span_rows(const std::vector<Operand>& ops, lk_result* res) {
  for (const Operand& o : ops)
    for (auto& tn : o.res->tag_names)
      if (std::find(res->tag_names.begin(), res->tag_names.end(), tn) == res->tag_names.end()) res->tag_names.push_back(tn);
  RowSpan s;
  for (const Operand& o : ops)
    if (o.res->nrows) {
      s.base = std::min(s.base, o.ts_lo);
      s.last = std::max(s.last, o.ts_hi);
      s.total_rows += o.res->nrows;
    }
  return s;
}

// ---- union group space: the operands' tag columns as formula_join.hpp reads them ----
// dim id -> tag text of a name / groupBy tag column (lk_result::own_tag_gid for one dim id); nullptr: the tag is absent
const char* dim_text(const lk_result::TagCol& t, uint32_t d) {
  if (t.hidden) return nullptr;
  if (d == t.dim_null) return t.null_value;
  if (t.shared) return (*t.shared)[d];
  if (!t.local.empty()) return t.local[d];
  const std::string& s = (*t.dict)[t.order ? t.order->perm[d] : d];
  return (s.empty() || s == "null") ? nullptr : s.c_str();
}

void find_key_columns(const std::vector<std::string>& key_cols, std::vector<Operand>& ops) {
  for (Operand& o : ops) {
    if (!o.res->nrows) continue;
    o.key_col.assign(key_cols.size(), -1);
    for (size_t j = 0; j < key_cols.size(); j++) {
      const auto& gbs = o.x->R->group_bys;
      const size_t at = size_t(std::find(gbs.begin(), gbs.end(), key_cols[j]) - gbs.begin());
      if (1 + at >= o.res->tcols.size()) throw PlanError(LK_ERR_DEVICE, "internal: groupBy column missing from the operand");
      o.key_col[j] = int(1 + at);
    }
  }
}

// A column every operand reads through the same engine dictionary (unrestricted groupBy, one generation) needs no
// table: union id = dim id + 1, the absent ids (NULL, "", "null") read 0 -- a 10M-value column costs nothing here.
// Values met outside the dictionary's dims (queryTags) take ids past them.
FxIdentity identity_column(Engine& E, const std::string& col, size_t j, const std::vector<Operand>& ops) {
  FxIdentity id;
  const StableStrs* dict = nullptr;
  bool ok = true, any = false;
  for (const Operand& o : ops) {
    if (!o.res->nrows) continue;
    const lk_result::TagCol& t = o.res->tcols[size_t(o.key_col[j])];
    const bool plain = !t.hidden && !t.shared && t.local.empty() && !t.order && t.dict && !t.null_value &&
                       t.ndim <= 0xfffffff0ull && t.dim_null + 1 == t.ndim;
    ok = ok && plain && (!any || t.dict == dict);
    dict = t.dict;
    any = true;
    id.ndim = std::max<uint32_t>(id.ndim, uint32_t(t.ndim));
  }
  if (!ok || !any) return id;
  GlobalDict* gd = &E.dict(col);
  std::lock_guard<std::mutex> g(gd->mu);
  if (gd->vals.get() != dict) return id;   // (another generation: take the tables)
  id.on = true;
  id.nl0 = gd->ids.find("");
  id.nl1 = gd->ids.find("null");
  id.dict_id = [gd](const char* s) {
    std::lock_guard<std::mutex> g2(gd->mu);
    return gd->ids.find(s);
  };
  return id;
}

FxOperandDims describe(const Operand& o) {
  FxOperandDims d;
  const lk_result& r = *o.res;
  if (!r.nrows) return d;
  if (r.tcols.empty()) throw PlanError(LK_ERR_DEVICE, "internal: operand without tag columns");
  d.has_rows = true;
  auto dim_of = [&r](size_t c) {
    const lk_result::TagCol* t = &r.tcols[c];
    return FxDim{r.tag_names[c], t->ndim, [t](uint32_t i) { return dim_text(*t, i); }};
  };
  d.name = dim_of(0);
  for (int c : o.key_col) d.key.push_back(dim_of(size_t(c)));
  if (!r.qt_of_glob.empty())
    for (auto& kv : r.qt_of_glob[0]) d.query_tags.emplace_back(r.tag_names[kv.first], kv.second ? kv.second : "");
  return d;
}

FxUnion union_space(Engine& E, const FxCall& call, std::vector<Operand>& ops, std::vector<FxIdentity>& ident) {
  find_key_columns(call.key_cols, ops);
  for (size_t j = 0; j < call.key_cols.size(); j++) ident.push_back(identity_column(E, call.key_cols[j], j, ops));
  std::vector<FxOperandDims> dims;
  for (const Operand& o : ops) dims.push_back(describe(o));
  return fx_union_space(call.key_cols, dims, ident);
}

// ---- device: tables, scatter, evaluate, write ----
// One staging block: per operand the key column maps and the name rank; the FxOperands that point into it.
std::vector<FxOperand> stage_operands(CallCtx& X, const std::vector<Operand>& ops, const FxUnion& un,
                                      const std::vector<FxIdentity>& ident) {
  std::vector<uint32_t> h;
  for (const FxOperandJoin& j : un.ops) {
    for (auto& m : j.map) h.insert(h.end(), m.begin(), m.end());
    h.insert(h.end(), j.name_rank.begin(), j.name_rank.end());
  }
  uint32_t* d_tabs = static_cast<uint32_t*>(X.workspace("fx_tabs", h.size() * 4 + 64));
  if (!h.empty()) HIP_TRY(hipMemcpyAsync(d_tabs, h.data(), h.size() * 4, hipMemcpyHostToDevice, X.stream));
  HIP_TRY(hipStreamSynchronize(X.stream));   // (h is pageable and leaves scope)
  std::vector<FxOperand> fo(ops.size());
  size_t off = 0;
  for (size_t k = 0; k < ops.size(); k++) {
    const lk_result& r = *ops[k].res;
    const FxOperandJoin& j = un.ops[k];
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
    f.ncols = int(ident.size());
    for (size_t c = 0; c < ident.size(); c++) {
      const lk_result::TagCol& tc = r.tcols[size_t(ops[k].key_col[c])];
      f.stride[c] = tc.stride ? tc.stride : 1;
      f.ndim[c] = tc.ndim ? tc.ndim : 1;
      f.ustride[c] = un.ustride[c];
      f.map[c] = ident[c].on ? nullptr : d_tabs + off;
      off += j.map[c].size();
      f.dim_null[c] = tc.dim_null;
      f.nl0[c] = ident[c].nl0;
      f.nl1[c] = ident[c].nl1;
    }
    f.after_name = j.after_name;
    f.qt_u = j.qt_u;
    f.name_stride = r.tcols[0].stride ? r.tcols[0].stride : 1;
    f.name_ndim = r.tcols[0].ndim ? r.tcols[0].ndim : 1;
    f.name_rank = d_tabs + off;
    off += j.name_rank.size();
    f.qt_rank = j.qt_rank;
  }
  return fo;
}

// Fills the cell table from every operand's rows; a full hash table regrows fourfold and scatters again.
Scattered scatter(const FxRun& c, CallCtx& X, const FxCall& call, const std::vector<FxOperand>& fo, const RowSpan& span,
                  const FxCells& cells, unsigned long long U, FxStats& st) {
  hipStream_t stream = X.stream;
  const unsigned long long L = fo.size();
  Scattered s;
  s.dense = cells.nkeys <= c.E.formula_dense_max_cells;
  s.ncells = cells.nkeys;
  if (!s.dense) {
    const unsigned long long want = c.E.formula_hash_slots ? c.E.formula_hash_slots : 2ull * span.total_rows;
    s.ncells = 64;
    while (s.ncells < want) s.ncells <<= 1;
  }
  uint32_t* d_flags = static_cast<uint32_t*>(X.workspace("fx_flags", 64));
  s.t0 = ms_since(c.t_start);
  for (;;) {
    if (s.ncells > (1ull << 34) / L) throw PlanError(LK_ERR_MEMORY, "formula: cell table too large");
    const unsigned long long words = s.ncells * (L + (s.dense ? 0 : 1));
    s.T.slots = static_cast<unsigned long long*>(X.workspace("fx_table", size_t(words) * 8 + 256));
    s.T.keys = s.dense ? nullptr : s.T.slots + s.ncells * L;
    s.T.ncells = s.ncells;
    s.T.U = U;
    s.T.nbuckets = cells.nbuckets;
    s.T.base = span.base;
    s.T.step = call.step;
    s.T.flags = d_flags;
    s.T.live = d_flags + 1;
    s.T.nleaves = int(L);
    HIP_TRY(hipMemsetAsync(d_flags, 0, 64, stream));
    HIP_TRY(launch_fx_fill(s.T.slots, words, stream));
    for (auto& f : fo) HIP_TRY(launch_fx_scatter(s.T, f, stream));
    uint32_t fl = 0;
    HIP_TRY(hipMemcpyAsync(&fl, d_flags, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (fl & FX_FLAG_OFFGRID) throw PlanError(LK_ERR_UNSUPPORTED, "formula: an expression's timestamps are off the step grid");
    if (fl & FX_FLAG_RANGE) throw PlanError(LK_ERR_DEVICE, "internal: formula cell outside the table");
    if (!(fl & FX_FLAG_FULL)) break;
    s.ncells <<= 2;   // no row is dropped
    st.regrows++;
  }
  st.scatter_ms = ms_since(c.t_start) - s.t0;
  st.mode = s.dense ? "dense" : "hash";
  st.cells = s.dense ? cells.nkeys : s.ncells;
  return s;
}

// Runs the program over every cell, compacts the rows that come out and fetches them with their sources.
Joined evaluate_cells(const FxRun& c, CallCtx& X, const FxCall& call, const std::vector<FxOperand>& fo,
                      const Scattered& sc, FxStats& st) {
  hipStream_t stream = X.stream;
  FxEval V{};
  V.T = sc.T;
  V.nops = call.prog.n;
  V.has_group_bys = call.key_cols.empty() ? 0 : 1;
  memcpy(V.ops, call.prog.ops, sizeof(FxOp) * size_t(call.prog.n));
  for (size_t l = 0; l < fo.size(); l++) {
    V.val[l] = fo[l].val;
    V.gid[l] = fo[l].gid;
    V.xform[l] = call.exprs[l].xform;
    V.secs[l] = call.secs;
  }
  const uint32_t nb = fx_blocks(sc.ncells);
  uint32_t* d_counts = static_cast<uint32_t*>(X.workspace("fx_counts", (size_t(nb) + 2) * 4));
  if (!sc.dense) {
    const size_t words = size_t(sc.T.nbuckets) * 2 + 2;
    uint32_t* bc = static_cast<uint32_t*>(X.workspace("fx_buckets", words * 4));
    HIP_TRY(hipMemsetAsync(bc, 0, words * 4, stream));
    V.bucket_count = bc;
    V.bucket_cursor = bc + sc.T.nbuckets + 1;
  }
  HIP_TRY(launch_fx_eval_count(V, d_counts, stream));
  uint32_t nout = 0;
  HIP_TRY(hipMemcpyAsync(&nout, d_counts + nb, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  const size_t n = nout;
  Joined j{std::vector<int32_t>(n), std::vector<uint32_t>(n)};
  st.out_rows = n;
  if (!n) {
    c.res->alloc_rows(0, false);
    c.res->gid = nullptr;
    return j;
  }
  uint8_t* ob = static_cast<uint8_t*>(X.workspace("fx_out", n * 24 + 64));
  int64_t* o_ts = reinterpret_cast<int64_t*>(ob);
  double* o_val = reinterpret_cast<double*>(ob + n * 8);
  int32_t* o_op = reinterpret_cast<int32_t*>(ob + n * 16);
  uint32_t* o_gid = reinterpret_cast<uint32_t*>(ob + n * 20);
  HIP_TRY(launch_fx_eval_write(V, d_counts, o_ts, o_val, o_op, o_gid, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  st.eval_ms = ms_since(c.t_start) - sc.t0 - st.scatter_ms;
  const double t1 = ms_since(c.t_start);
  c.res->alloc_rows(n, false);
  c.res->gid = nullptr;   // formula rows carry no group ids (lk_result_group_ids: NULL)
  HIP_TRY(hipMemcpyAsync(c.res->ts, o_ts, n * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(c.res->val, o_val, n * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(j.src_op.data(), o_op, n * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(j.src_gid.data(), o_gid, n * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  st.transfer_ms = ms_since(c.t_start) - t1;
  return j;
}

// ---- tags from (source operand, source group id); the operands' device rows are done with ----
void fill_tags(const std::vector<Operand>& ops, const Joined& j, lk_result* res) {
  for (const Operand& o : ops) {
    if (o.res->dev_rows) (void)hipFree(o.res->dev_rows);
    o.res->dev_rows = nullptr;
  }
  const size_t ncol = res->tag_names.size(), nout = j.src_op.size();
  // (an operand names a column twice when a queryTags key is also a groupBy: the row's own tag, else the queryTag)
  std::vector<std::vector<std::vector<size_t>>> col_of(ops.size(), std::vector<std::vector<size_t>>(ncol));
  for (size_t k = 0; k < ops.size(); k++)
    for (size_t c = 0; c < ncol; c++) {
      auto& tn = ops[k].res->tag_names;
      for (size_t oc = 0; oc < tn.size(); oc++)
        if (tn[oc] == res->tag_names[c]) col_of[k][c].push_back(oc);
    }
  res->ex_tags.assign(nout * ncol, nullptr);
  for (size_t r = 0; r < nout; r++) {
    const int32_t k = j.src_op[r];
    if (k < 0 || size_t(k) >= ops.size()) continue;   // a constant's empty tags
    const lk_result& orow = *ops[size_t(k)].res;
    for (size_t c = 0; c < ncol; c++)
      for (size_t oc : col_of[size_t(k)][c]) {
        const char* v = orow.tag_of_gid(j.src_gid[r], oc);
        if (v) res->ex_tags[r * ncol + c] = v;   // (a later column of the same name overwrites, as a tag map does)
      }
  }
  for (const Operand& o : ops) res->keep.push_back(o.res);   // the tag strings live in the operands' results
}

}  // namespace

// Distributed (lk_eval_formula_dist; DESIGN.md §7.6 "Distributed"): a rank is a pod.  Every operand is one sharded merged
// evaluation whose rows land on rank 0 (kept on its device, or uploaded by it), the join runs on rank 0 alone.  comm_mu is
// held for the whole call; the operands run in ascending byte order of their variable names, each closed by one
// agreement of the ranks' outcomes, so every rank issues the same collectives and all fail at the same operand.
// Everything decided before the first collective -- the parser, the gate, the shard check: fx_gate -- reads the request
// alone.
int evaluate_formula(Engine& E, const std::string& json, int glob_size, bool dist, lk_result* res) {
  const FxRun c{E, res, std::chrono::steady_clock::now(), glob_size <= 0 ? 10 : glob_size, dist,
                dist ? comm_world(E) : 1, dist ? comm_rank(E) : 0};
  const FxCall call = fx_gate(json, dist, c.world, [&E](const std::string& pd) { return E.parse_cached(pd); });
  FxStats st;
  st.world = c.world, st.rank = c.rank;
  res->exemplar = true;   // tags materialized per row (ex_tags): no bulk export of group ids
  if (call.exprs.empty()) {   // no variable: no SketchGroup reaches the formula, no rows
    write_stats(c, st);
    return LK_OK;
  }
  if (dist && !E.comm) throw PlanError(LK_ERR_ARG, "lk_comm_init has not been called");
  std::vector<Operand> ops(call.exprs.size());
  for (size_t k = 0; k < ops.size(); k++) ops[k].x = &call.exprs[k];
  run_operands(c, call, ops, st);
  // Behind the last operand's last collective: from here a failure unwinds this rank alone.  The other ranks return
  // their empty result; rank 0 looks at the rows for the first time.
  st.kind = c.rank != 0 ? FxStats::OFF_ROOT : FxStats::ROOT;
  if (c.rank != 0) {
    write_stats(c, st);
    return LK_OK;
  }
  place_rows(c, ops);
  st.operands_ms = ms_since(c.t_start);
  const RowSpan span = span_rows(ops, res);
  st.operand_rows = span.total_rows;
  if (!span.total_rows) {
    write_stats(c, st);
    return LK_OK;
  }
  std::vector<FxIdentity> ident;
  const FxUnion un = union_space(E, call, ops, ident);
  const FxCells cells = fx_cell_space(span.base, span.last, call.step, un.U);
  CtxLease X(E);
  const std::vector<FxOperand> fo = stage_operands(*X, ops, un, ident);
  const Scattered sc = scatter(c, *X, call, fo, span, cells, un.U, st);
  const Joined j = evaluate_cells(c, *X, call, fo, sc, st);
  fill_tags(ops, j, res);
  write_stats(c, st);
  return LK_OK;
}

}  // namespace lk
