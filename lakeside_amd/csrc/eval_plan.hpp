// Host planning of an aggregate evaluation (eval_plan.cpp): the stages between the parsed request and the first
// launch, each a function over the structs below.  A stage reads the earlier stages' structs and fills its own.
#pragma once
#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "engine.hpp"
#include "evalutil.hpp"
#include "kernels.hpp"
#include "numgroup_agree.hpp"
#include "plan.hpp"

namespace lk {

// Metrics timestamps off the step grid: the scan is re-run at millisecond granularity (evaluate()).
struct MetricsUnaligned {};
// Merged MIN with an all-NaN partial cell: the scan is re-run with per-glob cells (cell_policy).
struct MinNanApart {};
enum Redo : unsigned { REDO_METRICS_RAW = 1u, REDO_MIN_APART = 2u };

// internal evaluation flag: per-glob rows of a distributed call (rank 0 receives them), for evaluate_metrics_pct
constexpr unsigned kEvalDistPerGlob = 1u << 30;
// internal evaluation flag (evaluate_keep_device, the operands of lk_eval_formula): merged rows finalized into a device
// buffer the result owns (lk_result::dev_rows) instead of the host block -- no speculative finalize, no small-table
// epilogue, no key_bits / ts_runs host expansion, no device->host copy.  Distributed: rank 0 keeps the merged rows
// whichever reduce path the tables took, the other ranks keep nothing.  Off for every C ABI entry point but
// lk_eval_formula and lk_eval_formula_dist.
constexpr unsigned kEvalKeepDevice = 1u << 29;
// internal evaluation flag (the operands of lk_eval_formula_dist): the caller holds Engine::comm_mu for a whole sequence
// of distributed evaluations, so evaluate_once does not take it
constexpr unsigned kEvalCommHeld = 1u << 27;
// internal evaluation flag: the per-glob MAX rows of a metrics `p<NN>` (evaluate_metrics_pct), which takes no numeric
// groupBy (plan_numeric_group_bys)
constexpr unsigned kEvalMetricsPct = 1u << 28;

// One evaluation with its re-runs (eval.cpp); the composed evaluations of eval_compose.cpp call it per part.
int evaluate_req(Engine& E, const std::shared_ptr<const Request>& Rp, const char* const* paths, size_t n_paths,
                 int glob_size, unsigned flags, const int32_t* shard, bool dist, lk_result* res);
bool mixed_steps(const Request& R, int glob_size);
int evaluate_metrics_pct(Engine& E, const std::string& json, const Request& R, const char* const* paths, size_t n_paths,
                         int glob_size, unsigned flags, const int32_t* shard, bool dist, lk_result* res);
int evaluate_mixed_steps(Engine& E, const std::string& json, const Request& R, const char* const* paths, size_t n_paths,
                         int glob_size, unsigned flags, const int32_t* shard, bool dist, lk_result* res);

// The public evaluation (eval.cpp: metrics percentiles and mixed steps composed, else evaluate_req), and the two
// operand evaluations of lk_eval_formula (formula_eval.cpp): merged rows kept on the device; a host-assembled operand
// of a distributed formula, under the comm_mu its caller holds.
int evaluate(Engine& E, const std::string& json, const char* const* paths, size_t n_paths, int glob_size,
             unsigned flags, const int32_t* shard, bool dist, lk_result* res);
int evaluate_keep_device(Engine& E, const std::shared_ptr<const Request>& Rp, const char* const* paths, size_t n_paths,
                         int glob_size, const int32_t* shard, bool dist, lk_result* res);
int evaluate_comm_held(Engine& E, const std::string& json, const char* const* paths, size_t n_paths, int glob_size,
                       const int32_t* shard, lk_result* res);

// The call: its arguments and context, fixed while it runs.
struct EvalCall {
  Engine& E;
  CallCtx& X;
  const Request& R;
  const char* const* paths;
  size_t n_paths;
  int glob_size;
  unsigned flags;
  const int32_t* shard;
  bool dist;
  unsigned redo;
  lk_result* res;
  std::chrono::steady_clock::time_point t_start;
};

// What the request asks for (the shape gate): depends on the request and flags alone.
struct QueryShape {
  bool per_glob_rows = false, merged = false;
  bool tagq = false, fchart = false, sketch = false, ces = false;
  bool no_value_col = false;   // the SQL references no value column: tag queries (COUNT(*)), metrics `ces` (1.0 per row)
  bool metrics = false;        // raw-timestamp buckets (a tag query groups no timestamps)
  int agg = 0;
  double fscale = 0.0;         // field chart: the divisor (0.0: none)
  double quantile = 0.0;
  std::string vcol;
  std::vector<const FilterNode*> all_leaves;
  std::vector<std::string> nums;   // numeric query columns: the filter's, then the numeric groupBys not among them
  bool numeric = false;
  bool num_leaves = false;         // the filter holds gt / ge / lt / le leaves (numeric: or a numeric groupBy)
  // groupBys over columns stored as numbers (plan_numeric_group_bys): numeric group dimensions, DESIGN §7.7
  std::vector<std::string> numgbs;
  int numgb_index(const std::string& name) const {
    const auto it = std::find(numgbs.begin(), numgbs.end(), name);
    return it == numgbs.end() ? -1 : int(it - numgbs.begin());
  }
};

// The filter over string columns and numbered leaves, and its truth tables.
struct FilterPlan : LeafNumbering {
  std::vector<LeafCol> cols;       // name first, then leaf keys, then groupBys (DimPlan::dims runs parallel)
  std::vector<std::string> gbs;    // the groupBys, once each
  std::vector<uint8_t> bad_regex;  // per leaf: a pattern RE2 rejects
  // truth tables (plan_truth)
  bool vleaf = false;              // numeric leaves on the value column alone, tested per passing row (scan_lean; in
                                   //   COUNT / p<NN> / ces calls scan_tiles too)
  uint32_t vtab = 0;
  std::vector<uint32_t> truth, truth_early, truth_late, truth_x;   // truth_x: the general row scan's (vleaf)
  uint32_t late_mask = 0;
  int early = -1;                  // the column of the single-column early conjuncts, when there is one
  std::vector<int> dev_of;         // device order of the columns (query column 2 + dev_of[s])
  int lead = 0;                    // the column at device position 0
  bool vleaf_shape = false;
  int col_index(const std::string& name) const {
    for (size_t i = 0; i < cols.size(); i++)
      if (cols[i].name == name) return int(i);
    return -1;
  }
};

struct GlobInfo {
  std::vector<int> segs;                  // request indices
  bool skip = false;                      // Binder-error glob or no segments here
  uint32_t leaf_false = 0;
  int64_t win_lo = 0, win_hi = 0;
  int64_t step = 0;
  std::vector<std::pair<std::string, std::string>> query_tags;   // glob head's queryTags
};

// The segments this process evaluates and the globs' agreed column unions.  Owns the segments and the FieldTab lock
// for the call's duration.
struct GlobPlan {
  int world = 1, rank = 0;
  std::vector<std::shared_ptr<Segment>> segs;
  std::vector<uint8_t> seg_bad;
  std::string bad_msg;    // the first unreadable segment (stats)
  int load_err = 0;       // a rank-local failure, carried to the glob agreement
  std::string load_msg;
  bool tag_numeric = false;   // a tag query over a numeric tag column: the call takes the TAGNUM row scan
  std::set<std::string> fset;
  std::vector<std::string> probe_cols;   // columns whose existence matters
  // [globs x np exists | globs fail | globs value-type rank | value NULLs | numeric tag column |
  //  globs: a numeric file of the chart field | globs: a VARCHAR file of it |
  //  candidate groupBys x globs: the column's class (GbClass, 3 bytes)]
  std::vector<uint8_t> exists;
  std::vector<GlobInfo> globs;
  bool value_nulls = false;
  bool ftext_any = false;     // field chart: some glob's chart field is VARCHAR
  // the groupBys that may be numeric (the request alone decides) and [candidate][glob] their agreed classes
  std::vector<std::string> gb_cands;
  std::vector<GbClass> gb_class;
  // numeric groupBys: [numgb][glob] the column's union_by_name type over the glob's files on every rank, from the
  // agreed classes (Parquet type; -1: no file of the glob has it)
  std::vector<std::vector<int>> num_ut;
  size_t nfailed = 0;
  int64_t step = -1;
  std::shared_ptr<FieldTab> ftab;
  std::unique_lock<std::mutex> ftab_guard;
  uint32_t ftab_n = 0;
  size_t np() const { return probe_cols.size(); }
  const uint8_t* gvrank() const { return exists.data() + globs.size() * (np() + 1); }
  const uint8_t* gftext() const { return exists.data() + globs.size() * (np() + 3) + 2; }
  bool has(size_t gi, const std::string& c) const {
    const size_t k = size_t(std::find(probe_cols.begin(), probe_cols.end(), c) - probe_cols.begin());
    return exists[gi * np() + k] != 0;
  }
};

// A string column as a group dimension.
struct DimCol {
  bool is_dim = false;
  bool restricted = false;
  bool numeric = false;                   // a numeric group dimension: restricted, `cand` = the discovered values' texts
  std::vector<std::string> cand;          // restricted dims: candidate values (dim id = position)
  uint32_t ndim = 1;
  uint32_t dim_null = 0;
  uint64_t stride = 0;
  uint32_t dict_n = 0;                    // snapshot of the global dictionary size
  // distributed, unrestricted dim: the agreed union of every rank's value keys (dims.cpp; dim id = position)
  bool exchanged = false;
  std::shared_ptr<DimUnion> uni;
  // the value of dim id d (d != dim_null); `gd` is this column's engine dictionary (caller holds its lock).  A union
  // dim's null-like values read as "" (their tag drops either way).
  std::string_view dim_value(uint32_t d, const GlobalDict& gd) const {
    if (restricted) return cand[d];
    if (!exchanged) return gd[d];
    const char* t = (*uni->text)[d];
    return t ? std::string_view(t) : std::string_view();
  }
  // engine global id -> dim id of an exchanged dim
  uint32_t exchanged_dim(uint32_t gid) const { return (*uni->dim_of_gid)[gid]; }
};

// Which cells share a table entry, and the cell key space (glob slot, bucket, group); the table mode.
struct CellSpace {
  bool min_max_nulls = false, collapse_in_table = false, per_glob_cells = false;
  bool collapse = false;      // merged rows without groupBys: one row per bucket
  int64_t max_hi = INT64_MIN;
  int64_t bucket_base = 0;
  uint64_t nbuckets = 0;
  std::vector<std::vector<uint32_t>> fold_maps;   // dims whose null-like values fold after per-glob finalization
  bool rekey = false;
  uint32_t nslots = 1;
  uint64_t ncells = 0;
  bool hash_mode = false;
  uint64_t cap = 0, cap_max = 0;   // hash table: first size and bound
};

// The numeric group dimensions' device tables (eval.cpp: discover_numdims), read by the aggregate scan.
struct NumDimTables {
  uint64_t cap = 0;           // slots per (glob, column)
  int attempts = 0;
  double ms = 0;
  double exchange_ms = 0;     // distributed: the value sets' all-gather and union (this rank)
  uint64_t exchange_bytes = 0;
  unsigned long long* d_keys = nullptr;
  uint32_t* d_ids = nullptr;
  uint32_t* d_ones = nullptr;
  uint32_t* d_flags = nullptr;
  const uint32_t* d_seg_glob = nullptr;
};

struct DimPlan {
  std::vector<DimCol> dims;   // parallel to FilterPlan::cols, then one per QueryShape::numgbs (least significant)
  NumDimTables nd;
  uint64_t ngroups = 1;
  double dims_ms = 0;         // distributed group-dim agreement (stats)
  int dims_rebuilt = 0;
  std::vector<std::vector<uint32_t>> tabs;   // lookup tables: global id -> leaf bits << 24 | dim id
  std::vector<char> need_tab;
  std::vector<uint32_t> name_rank;
};

// Per-segment query descriptors: `qsegs` for the fused kernels, `gsegs` for the general row scan.
struct SegPlan {
  std::vector<QSeg> qsegs, gsegs;
  std::vector<uint32_t> gseg_glob;   // the glob of every gseg (QSeg::glob_slot is 0 where globs share cells)
  std::vector<uint32_t> seg_begin;
  uint32_t total_tiles = 0, max_tiles = 0, gmax_tiles = 0;
  uint64_t rows_scanned = 0, alg_bytes = 0;
  // QParams::exact_sum: every bound value column integral (HostCol::int_abs_max), its largest magnitude, their rows
  bool vals_integral = true;
  double vals_abs_max = 0.0, vals_rows = 0.0;
  bool all_lean = true;       // every fused-kernel tile is scan_lean's (the general kernel need not run)
  // scan_clu's segments (QSeg::clu set by plan_segments, kept by plan_cluster): the last n_clu of qsegs; the kernels
  // before it see only qsegs[0 .. size - n_clu)
  uint32_t n_clu = 0;
  int local_err = 0;         // distributed: a rank-local failure, agreed on with the other ranks after the scan
  std::string local_msg;
};

struct Plan {
  QueryShape qs;
  FilterPlan fp;
  GlobPlan gp;
  CellSpace cs;
  DimPlan dp;
  SegPlan sg;
  // group dimension s (DimPlan::dims): its column, and the dimension of a column
  const std::string& dim_name(size_t s) const { return s < fp.cols.size() ? fp.cols[s].name : qs.numgbs[s - fp.cols.size()]; }
  int dim_index(const std::string& name) const {
    const int k = qs.numgb_index(name);
    return k >= 0 ? int(fp.cols.size()) + k : fp.col_index(name);
  }
};

// The stages, in call order.  shape_gate .. plan_filter read no segment.
void shape_gate(const EvalCall& C, QueryShape& qs);
// The two answers that read no segment (no segments; a field chart without fieldType): true when *C.res is written.
bool answer_without_segments(const EvalCall& C, const QueryShape& qs);
void plan_filter(const EvalCall& C, const QueryShape& qs, FilterPlan& fp);
void load_segments(const EvalCall& C, const QueryShape& qs, GlobPlan& gp);
// Which groupBys are numeric group dimensions (reads the loaded segments' schemas; before plan_filter).
void plan_numeric_group_bys(const EvalCall& C, QueryShape& qs, const GlobPlan& gp);
// Distributed calls: the groupBys that may be numeric; whether the agreed classes of plan_globs ask for a second pass
// (shape -> filter -> globs) and its decision from them, the same on every rank; the glob plan emptied for that pass.
std::vector<std::string> numeric_gb_candidates(const EvalCall& C, const QueryShape& qs);
bool dist_numeric_replan(const EvalCall& C, const QueryShape& qs, const GlobPlan& gp);
void decide_numeric_group_bys(const EvalCall& C, QueryShape& qs, const std::vector<std::string>& cands,
                              const std::vector<GbClass>& cls);
void reset_glob_plan(GlobPlan& gp);
void plan_globs(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, GlobPlan& gp);   // collective: globs
void cell_policy(const EvalCall& C, const QueryShape& qs, const GlobPlan& gp, CellSpace& cs);
void plan_dims(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, DimPlan& dp);     // collective: dims
void plan_strides(DimPlan& dp);   // strides and the group space from the dims' sizes
void plan_tables(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, const GlobPlan& gp, const CellSpace& cs,
                 DimPlan& dp);
void plan_cells(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, const GlobPlan& gp, const DimPlan& dp,
                CellSpace& cs);
void plan_truth(const EvalCall& C, const QueryShape& qs, FilterPlan& fp);
void plan_segments(const EvalCall& C, const QueryShape& qs, const FilterPlan& fp, const GlobPlan& gp, const CellSpace& cs,
                   SegPlan& sg);
void plan_table_mode(const QueryShape& qs, const SegPlan& sg, CellSpace& cs);
// After the table mode is known: the segments scan_clu takes whole go to the end of qsegs (sg.n_clu of them); a
// hash-mode table keeps every segment on the other kernels.
void plan_cluster(const CellSpace& cs, SegPlan& sg);

// A value leaf as the fused kernels read it (QParams::vl; vleaf.hpp states the test).
inline VLeaf vleaf_of(const NumLeaf& nl) { return VLeaf{nl.dlo, nl.dhi, nl.lo_incl, nl.hi_incl, nl.nan_pass, 0u}; }

// The pure part of the filter planning (filter_plan.cpp: the request and the shape alone, no Engine, no HIP call):
// shape_gate's leaf loop (all_leaves, nums, numeric), and what plan_filter / plan_truth do for a call.
void shape_leaves(const Request& R, QueryShape& qs);
void shape_aggregation(const Request& R, QueryShape& qs);   // agg, sketch, ces, no_value_col (qs.tagq is set)
// p<NN> / ces charts take numeric leaves only as value leaves (FilterPlan::vleaf); LK_ERR_UNSUPPORTED otherwise.  The
// gate plans a scratch filter from the request alone; the check reads the call's own plan (after plan_truth).
void sketch_leaf_gate(const Request& R, const QueryShape& qs);
void sketch_leaf_check(const QueryShape& qs, const FilterPlan& fp);
void plan_filter(const Request& R, const QueryShape& qs, FilterPlan& fp);
void plan_truth(const Request& R, const QueryShape& qs, FilterPlan& fp);

// The result's tag columns (eval_rows.cpp).
void label_rows(const EvalCall& C, const Plan& pl, uint32_t nrows_out);

}  // namespace lk
