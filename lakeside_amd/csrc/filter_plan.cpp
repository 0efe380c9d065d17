// The pure part of the filter planning: the request's filter tree -> numbered leaves, the postfix Kleene program and
// its truth tables (whole filter, early / late split, value-leaf table), the device order of the string columns.  Reads
// the request and the QueryShape alone -- no Engine, no HIP call -- so the CPU tests reach it through
// liblakeside_text.so (filter_plan_sim.cpp); eval_plan.cpp calls it with the call's request.
#include <algorithm>
#include <cstdlib>

#include "eval_plan.hpp"
#include "layout.hpp"
#include "regex.hpp"

namespace lk {

// regexp_matches(label, p, 'i') (BaseExpr.scala:485-486) / regexp_matches(label, '.*p.*', 'i') (500-501).  A pattern
// RE2 rejects makes DuckDB fail the glob's query, which Commons.toGlobResultSet turns into an empty result
// (Commons.scala:249-253): LK_ERR_ARG, which the shim maps to the same empty source.
re::Regex compile_leaf_regex(const FilterNode& l) {
  const std::string pat = l.op == "contains" ? ".*" + l.v[0] + ".*" : l.v[0];
  try {
    return re::Regex(pat, true);
  } catch (const re::RegexError& e) {
    throw PlanError(e.unsupported ? LK_ERR_UNSUPPORTED : LK_ERR_ARG, std::string("regex '") + pat + "': " + e.what());
  }
}

void postfix(const FilterNode* n, const std::vector<LeafInfo>& leaves, std::vector<uint8_t>& prog) {
  switch (n->kind) {
    case FilterNode::LEAF:
      for (auto& l : leaves)
        if (l.node == n) { prog.push_back(uint8_t(l.index)); return; }
      throw PlanError(LK_ERR_ARG, "internal: leaf not numbered");
    case FilterNode::AND:
    case FilterNode::OR:
      postfix(n->a.get(), leaves, prog);
      postfix(n->b.get(), leaves, prog);
      prog.push_back(n->kind == FilterNode::AND ? OP_AND : OP_OR);
      return;
    case FilterNode::NOT:
      postfix(n->a.get(), leaves, prog);
      prog.push_back(OP_NOT);
      return;
  }
}

void collect_leaves(const FilterNode* n, std::vector<const FilterNode*>& out) {
  if (n->kind == FilterNode::LEAF) out.push_back(n);
  else {
    collect_leaves(n->a.get(), out);
    if (n->b) collect_leaves(n->b.get(), out);
  }
}

// Conjuncts of the filter's top-level AND chain (a AND (b AND c) -> a, b, c).
void conjuncts(const FilterNode* n, std::vector<const FilterNode*>& out) {
  if (n->kind == FilterNode::AND) {
    conjuncts(n->a.get(), out);
    conjuncts(n->b.get(), out);
  } else {
    out.push_back(n);
  }
}

// Truth table of a postfix Kleene program over L leaves: bit (T | F << L) = the program is TRUE.  An empty
// program is TRUE.
std::vector<uint32_t> truth_table(const std::vector<uint8_t>& prog, uint32_t L) {
  std::vector<uint32_t> truth(((1u << (2 * L)) + 31) / 32, 0u);
  for (uint32_t idx = 0; idx < (1u << (2 * L)); idx++) {
    const uint32_t T = idx & ((1u << L) - 1), F = idx >> L;
    uint64_t st = 0, sf = 0;
    for (uint8_t op : prog) {
      if (op < 0x80) {
        st = (st << 1) | ((T >> op) & 1u);
        sf = (sf << 1) | ((F >> op) & 1u);
      } else if (op == OP_NOT) {
        uint64_t t1 = st & 1, f1 = sf & 1;
        st = (st & ~1ull) | f1;
        sf = (sf & ~1ull) | t1;
      } else if (op == OP_TRUE) {
        st = (st << 1) | 1;
        sf = sf << 1;
      } else {
        uint64_t t2 = st & 1, f2 = sf & 1;
        st >>= 1;
        sf >>= 1;
        uint64_t t1 = st & 1, f1 = sf & 1;
        uint64_t tt = op == OP_AND ? (t1 & t2) : (t1 | t2);
        uint64_t ff = op == OP_AND ? (f1 | f2) : (f1 & f2);
        st = (st & ~1ull) | tt;
        sf = (sf & ~1ull) | ff;
      }
    }
    if (prog.empty() || (st & 1)) truth[idx >> 5] |= 1u << (idx & 31);
  }
  return truth;
}

void shape_leaves(const Request& R, QueryShape& qs) {
  collect_leaves(R.filter.get(), qs.all_leaves);
  // Numeric comparison leaves (gt/ge/lt/le, BaseExpr.scala:488-498) compare a numeric column per row: such queries
  // run on the general row scan (ex_scan AGG mode, ex_kernels.hip) instead of the fused string-filter kernels.
  for (auto* l : qs.all_leaves) {
    if (l->extracted || l->computed) throw PlanError(LK_ERR_UNSUPPORTED, "extracted/computed filter fields");
    if (numeric_op(l->op)) {
      if (std::find(qs.nums.begin(), qs.nums.end(), l->k) == qs.nums.end()) qs.nums.push_back(l->k);
      continue;
    }
    static const char* ok[] = {"eq", "!=", "in", "not_in", "regex", "contains", "has", "exists"};
    if (std::none_of(std::begin(ok), std::end(ok), [&](const char* o) { return l->op == o; }))
      throw PlanError(LK_ERR_ARG, "Invalid operator " + l->op);
  }
  qs.numeric = !qs.nums.empty();
  qs.num_leaves = qs.numeric;   // (numeric groupBys make a shape numeric later; the sketch gate asks about leaves)
}

// The aggregate a chart asks for; qs.tagq is set.
// Cardinality (`ces` in the chart's rollup, PushDownAggregatorStage.scala:44,82-94; computeCardinality sets it,
// QueryEngineV2.scala:616-617): per step one HLL over the rows' group-key strings, whatever the SQL aggregate.
// Metrics: `ces` as the chart's aggregation compiles to `SELECT ts, 1.0 as value, name, <groupBys> ... WHERE
// <filter>` -- every passing row, no rollup column (BaseExpr.scala:385-388); a metrics rollup of "ces" under another
// aggregation stays that aggregation over rollup_ces (the SQL reads that column).
void shape_aggregation(const Request& R, QueryShape& qs) {
  if (qs.tagq) qs.agg = AGG_ROWS;
  else if (R.aggregation == "ces" || (R.rollup.find("ces") != std::string::npos && R.dataset != "metrics")) qs.agg = AGG_CES;
  else if (R.aggregation == "sum") qs.agg = AGG_SUM;
  else if (R.aggregation == "min") qs.agg = AGG_MIN;
  else if (R.aggregation == "max") qs.agg = AGG_MAX;
  else if (R.aggregation == "count") qs.agg = AGG_COUNT;
  else if (R.aggregation == "avg") qs.agg = AGG_AVG;
  else if (R.aggregation.size() > 1 && R.aggregation[0] == 'p' && R.dataset != "metrics") qs.agg = AGG_SKETCH;
  else throw PlanError(LK_ERR_UNSUPPORTED, "aggregation " + R.aggregation + " (sketch path) is not on the hot path");
  // Percentiles (logs / traces): BaseExpr.getChartSql selects the passing rows (BaseExpr.scala:397-399), the
  // worker's PushDownAggregatorStage builds one DDSketch per (step, group-key tags) (PushDownAggregatorStage.scala:
  // 69-81, 188-197), query-api merges per (timestamp, tags) and reads getValueAtQuantile(p / 100)
  // (BaseExpr.scala:59-61).  Here: the scan bins every value on the GPU (COUNT per (cell, DDSketch bin)), the host
  // assembles the sketches.
  qs.sketch = qs.agg == AGG_SKETCH;
  qs.ces = qs.agg == AGG_CES;
  // queries whose SQL references no value column: tag queries (COUNT(*)) and metrics `ces` (1.0 per row)
  qs.no_value_col = qs.tagq || (qs.ces && R.dataset == "metrics");
}

// Numeric comparison leaves in p<NN> / ces charts.  The reference compiles them into the row-selecting SQL's WHERE like
// any other leaf (BaseExpr.scala:397-399 with 488-498); here the sketch routes take them only as value leaves
// (FilterPlan::vleaf: every numeric leaf on the chart's value column, in conjuncts of their own, <= VLEAF_MAX of them
// and <= TT_MAX_LEAVES leaves in all), which scan_tiles, scan_lean and ex_scan all test.  Every other one is refused --
// a leaf on another column, a mixed conjunct, LK_NO_VLEAF=1, metrics `ces` (no value column is bound) -- and so is a
// filter the planner itself refuses, under this text, which came first before the gate read the plan.  Reads the
// request and the shape alone: every rank of a distributed call decides alike, before its first collective.
static const char* const kSketchLeafRefusal = "numeric comparison leaves in sketch queries";
void sketch_leaf_gate(const Request& R, const QueryShape& qs) {
  if (!qs.num_leaves || !(qs.sketch || qs.ces)) return;
  bool ok = !qs.no_value_col;
  if (ok) {
    try {
      FilterPlan fp;
      plan_filter(R, qs, fp);
      plan_truth(R, qs, fp);
      ok = fp.vleaf;
    } catch (const PlanError&) {
      ok = false;
    }
  }
  if (!ok) throw PlanError(LK_ERR_UNSUPPORTED, kSketchLeafRefusal);
}
// The same rule on the call's own plan: a groupBy the loaded files store as a number joins the numeric columns after
// the gate (plan_numeric_group_bys) and takes the value leaves' route away (in a distributed call from agreed classes:
// every rank refuses alike).
void sketch_leaf_check(const QueryShape& qs, const FilterPlan& fp) {
  if (qs.num_leaves && (qs.sketch || qs.ces) && !fp.vleaf) throw PlanError(LK_ERR_UNSUPPORTED, kSketchLeafRefusal);
}

void plan_filter(const Request& R, const QueryShape& qs, FilterPlan& fp) {
  // ---- string columns: name first, then leaf keys, then groupBys ----
  auto col = [&](const std::string& name) -> LeafCol& {
    const int i = fp.col_index(name);
    if (i >= 0) return fp.cols[size_t(i)];
    fp.cols.push_back(LeafCol{});
    fp.cols.back().name = name;
    return fp.cols.back();
  };
  col(qs.tagq ? R.tag_name : kName);   // the first string column is the leading group dim
  for (auto* l : qs.all_leaves)
    if (!numeric_op(l->op)) col(l->k).leaves.push_back(l);
  for (auto& g : R.group_bys)
    if (std::find(fp.gbs.begin(), fp.gbs.end(), g) == fp.gbs.end()) fp.gbs.push_back(g);
  for (auto& g : fp.gbs)
    if (qs.numgb_index(g) < 0) col(g);   // (a numeric group dimension is a numeric query column, no string column)
  if (fp.cols.size() > size_t(MAXSTR)) throw PlanError(LK_ERR_UNSUPPORTED, "too many string columns in one query");
  for (auto& nm : qs.nums)   // a column compared both as a string and as a number fails the glob's SQL either way
    if (fp.col_index(nm) >= 0)
      throw PlanError(LK_ERR_UNSUPPORTED, "column " + nm + " used both as a string and as a number");
  if (2 + fp.cols.size() + qs.nums.size() > size_t(MAXQCOL)) throw PlanError(LK_ERR_UNSUPPORTED, "too many filter columns");
  if (qs.all_leaves.size() > size_t(MAXLEAF)) throw PlanError(LK_ERR_UNSUPPORTED, "too many filter leaves");
  // (a tag query's tag may be the value / timestamp column: numeric, it takes the TAGNUM row scan, load_segments)
  if (std::find_if(fp.cols.begin(), fp.cols.end(), [&](const LeafCol& s) {
        return (s.name == kTimestamp || s.name == qs.vcol) && !(qs.tagq && s.name == R.tag_name);
      }) != fp.cols.end() ||
      std::find_if(qs.numgbs.begin(), qs.numgbs.end(), [&](const std::string& g) { return g == kTimestamp || g == qs.vcol; }) !=
          qs.numgbs.end())
    throw PlanError(LK_ERR_UNSUPPORTED, "filters / groupBys on the timestamp or value column");
  static_cast<LeafNumbering&>(fp) = number_leaves(R.filter.get(), qs.all_leaves,
                                                  [](const FilterNode* l) { return numeric_op(l->op); }, qs.nums, fp.cols);
  // Regex leaves RE2 rejects (LK_ERR_ARG) fail the SQL only of the globs where the leaf's field exists (plan_globs);
  // a pattern RE2 takes but this matcher does not (LK_ERR_UNSUPPORTED) fails the call.
  fp.bad_regex.assign(fp.leaves.size(), 0);
  for (auto& l : fp.leaves)
    if (l.node->op == "regex" || l.node->op == "contains") {
      try {
        (void)compile_leaf_regex(*l.node);
      } catch (const PlanError& e) {
        if (e.code != LK_ERR_ARG) throw;
        fp.bad_regex[size_t(l.index)] = 1;
      }
    }
}

void plan_truth(const Request& R, const QueryShape& qs, FilterPlan& fp) {
  // Numeric leaves on the value column alone (`:and(:eq name, :gt value 1.5)`), in conjuncts of their own: the fused
  // kernels filter on the string conjuncts and test the value of each passing row (QParams.vl / vtab) -- the segments
  // whose tiles all qualify for scan_lean; the other segments take the general row scan as before.
  std::vector<uint8_t> prog_str;   // vleaf: the string conjuncts (the fused kernels' filter)
  if (qs.numeric && !qs.tagq && qs.nums.size() == 1 && qs.nums[0] == qs.vcol && fp.nleaves.size() <= size_t(VLEAF_MAX) &&
      fp.leaves.size() <= size_t(TT_MAX_LEAVES) && !getenv("LK_NO_VLEAF")) {
    std::vector<const FilterNode*> conj;
    conjuncts(R.filter.get(), conj);
    std::vector<uint8_t> pn;
    bool ok = true;
    for (auto* c : conj) {
      std::vector<const FilterNode*> ls;
      collect_leaves(c, ls);
      const size_t nn = size_t(std::count_if(ls.begin(), ls.end(), [](const FilterNode* l) { return numeric_op(l->op); }));
      if (nn && nn != ls.size()) ok = false;   // a conjunct mixing string and numeric leaves
      std::vector<uint8_t>& dst = nn ? pn : prog_str;
      const bool first = dst.empty();
      postfix(c, fp.leaves, dst);
      if (!first) dst.push_back(OP_AND);
    }
    if (ok && !pn.empty()) {
      fp.vleaf = true;
      if (prog_str.empty()) prog_str.push_back(OP_TRUE);
      // vtab bit m: the numeric conjuncts with leaf k TRUE iff bit k of m (no UNKNOWN: scan_lean tiles hold no NULL)
      const uint32_t L = uint32_t(fp.leaves.size()), nsl = L - uint32_t(fp.nleaves.size());
      const std::vector<uint32_t> tn = truth_table(pn, L);
      for (uint32_t m = 0; m < (1u << fp.nleaves.size()); m++) {
        const uint32_t full = (1u << fp.nleaves.size()) - 1u;
        const uint32_t ix = (m << nsl) | (((~m & full) << nsl) << L);
        if ((tn[ix >> 5] >> (ix & 31)) & 1u) fp.vtab |= 1u << m;
      }
    }
  }
  // filter truth table: bit (T | F << L) = Kleene value of the tree is TRUE (host-evaluated once per query)
  if (fp.leaves.size() <= size_t(TT_MAX_LEAVES)) {
    const uint32_t L = uint32_t(fp.leaves.size());
    fp.truth = truth_table(fp.vleaf ? prog_str : fp.prog, L);
    if (fp.vleaf) fp.truth_x = truth_table(fp.prog, L);
    // Predicate pushdown + late materialization.  filter = C_early AND C_late where C_early is the conjuncts
    // over one "early" column (the name column when a conjunct constrains it alone).  The kernel decodes the
    // early column for every row, lists the rows where C_early is TRUE, and decodes every other string column
    // (late filter columns, group dims) only for listed rows, where it evaluates C_late.
    std::vector<const FilterNode*> conj;
    conjuncts(R.filter.get(), conj);
    auto cols_of = [&](const FilterNode* n) {
      std::vector<const FilterNode*> ls;
      collect_leaves(n, ls);
      uint32_t m = 0;
      for (auto* l : ls) m |= numeric_op(l->op) ? (1u << 31) : (1u << fp.col_index(l->k));   // no StrCol for numbers
      return m;
    };
    // A conjunct of only `exists`/`has` leaves (IS NOT NULL: passes nearly every row, e.g. the one query-api adds
    // to a tag query) is a poor early filter: it is chosen only when no other single-column conjunct exists.
    auto weak = [&](const FilterNode* n) {
      std::vector<const FilterNode*> ls;
      collect_leaves(n, ls);
      return std::all_of(ls.begin(), ls.end(), [](const FilterNode* l) { return l->op == "exists" || l->op == "has"; });
    };
    bool early_weak = true;
    if (fp.vleaf)   // the value-leaf conjuncts are tested per passing row, outside the early / late split
      conj.erase(std::remove_if(conj.begin(), conj.end(), [&](const FilterNode* c) { return cols_of(c) == (1u << 31); }),
                 conj.end());
    for (auto* c : conj) {
      const uint32_t m = cols_of(c);
      if (__builtin_popcount(m) != 1) continue;
      const int col = __builtin_ctz(m);
      const bool w = weak(c);
      if (fp.early < 0 || (early_weak && !w) || (w == early_weak && col == 0)) {
        fp.early = col;
        early_weak = w;
      }
    }
    // The late pass sees only the late columns' leaves: a conjunct mixing the early column with others keeps
    // every column early (no late pass).
    bool mixed = false;
    for (auto* c : conj) {
      const uint32_t m = cols_of(c);
      if (fp.early >= 0 && m != (1u << fp.early) && ((m >> fp.early) & 1u)) mixed = true;
    }
    if (fp.early >= 0 && fp.cols.size() >= 2 && !mixed && (!qs.numeric || fp.vleaf)) {
      std::vector<uint8_t> pe, pl;
      for (auto* c : conj) {
        std::vector<uint8_t>& dst = cols_of(c) == (1u << fp.early) ? pe : pl;
        const bool first = dst.empty();
        postfix(c, fp.leaves, dst);
        if (!first) dst.push_back(OP_AND);
      }
      fp.truth_early = truth_table(pe, L);
      fp.truth_late = truth_table(pl, L);
      for (size_t sidx = 0; sidx < fp.cols.size(); sidx++)
        if (int(sidx) != fp.early) fp.late_mask |= 1u << sidx;
    }
  }
  // Device order of the string columns (query column 2 + dev_of[s]): the early column first when the filter's late
  // materialization lists every other column late, so scan_lean (whose early column is query column 2) takes the
  // query even when the leading group dim -- a tag query's tag, a :by column -- is not the filter's early column.
  fp.dev_of.resize(fp.cols.size());
  for (size_t i = 0; i < fp.cols.size(); i++) fp.dev_of[i] = int(i);
  // (LK_NO_EARLY_FIRST=1: the r03 order, for A/B)
  if (fp.late_mask && fp.early > 0 && fp.cols.size() <= 3 && !getenv("LK_NO_EARLY_FIRST")) {
    std::swap(fp.dev_of[0], fp.dev_of[size_t(fp.early)]);
    uint32_t m = 0;
    for (size_t i = 0; i < fp.cols.size(); i++)
      if ((fp.late_mask >> i) & 1u) m |= 1u << fp.dev_of[i];
    fp.late_mask = m;
  }
  fp.lead = fp.dev_of[0] == 0 ? 0 : int(std::find(fp.dev_of.begin(), fp.dev_of.end(), 0) - fp.dev_of.begin());   // strs index at device 0
  // vleaf needs scan_lean's shape: the early column alone, or with <= 2 late columns (setup_scan's lean_shape)
  fp.vleaf_shape = fp.vleaf && !fp.truth.empty() &&
                           (fp.cols.size() == 1 || (fp.cols.size() <= 3 && fp.late_mask == ((1u << fp.cols.size()) - 2u)));
}

}  // namespace lk
