// The row scan's planning stages (exemplar.cpp), shared with the tag-name route (tagnames.cpp): the structs a stage
// returns and the stages both routes run -- filter, globs and their union_by_name schemas, per-segment descriptors,
// device staging, the gather of the selected rows' columns and their text.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "engine.hpp"
#include "eval_plan.hpp"
#include "evalutil.hpp"
#include "ex_select.hpp"
#include "hostutil.hpp"
#include "kernels.hpp"
#include "layout.hpp"

namespace lk {

// A pinned host block from the engine's pool for the length of a transfer (returned to the pool on scope exit).
struct PinnedTmp {
  HostBlock b;
  explicit PinnedTmp(size_t n) : b(pinned_acquire(n)) {}
  ~PinnedTmp() { pinned_release(b); }
  PinnedTmp(const PinnedTmp&) = delete;
  PinnedTmp& operator=(const PinnedTmp&) = delete;
  void* p() const { return b.p; }
};

// What the request asks for: depends on the request and flags alone.
struct XShape {
  bool tagnum = false, logs = false, desc = true, per_glob_rows = false;
  bool star = false;   // SELECT * alone (tag names): no projection ahead of the union's columns
  uint64_t limit = 0;
  std::string numtag;
  std::vector<const FilterNode*> all_leaves;
  std::vector<std::string> nums;   // numeric comparison columns (gt/ge/lt/le, BaseExpr.scala:488-498)
  // numeric tag: its leaves (query-api's `exists` on the tag) are numeric IS NOT NULL leaves; the tag column is a
  // numeric column of the scan either way
  bool num_col(const FilterNode* l) const { return numeric_op(l->op) || (tagnum && l->k == numtag); }
};

// The filter columns (string dictionaries) and the Kleene program.
struct XFilter : LeafNumbering {
  std::vector<LeafCol> strs;
};

struct XGlob : XSel {
  std::vector<int> segs;
  bool skip = false;
  uint32_t leaf_false = 0;
  std::vector<std::string> cols;          // output columns: projection, then the union (file order)
  std::map<std::string, int> types;       // union type per column
  int type_or(const std::string& name, int dflt) const {
    const auto it = types.find(name);
    return it == types.end() ? dflt : it->second;
  }
};

struct XGlobs {
  std::vector<std::shared_ptr<Segment>> segs;
  std::vector<uint8_t> seg_bad;
  std::vector<XGlob> globs;
};

// Per-segment descriptors: `qsegs` goes to the device as it is, `meta` runs parallel to it.
struct XSegMeta {
  const Segment* seg;
  uint32_t pos;    // segment position in the glob
  uint32_t glob;
};
struct XSegs {
  std::vector<QSeg> qsegs;
  std::vector<XSegMeta> meta;
  uint64_t rows_scanned = 0;
  uint32_t max_tiles = 0;
};

// The per-glob range words of the staged block, [4][ng]: a HIST pass reads all four, TAGNUM and EMIT the range only.
struct XRanges {
  int64_t* w = nullptr;
  size_t ng = 0;
  int64_t& rlo(size_t g) const { return w[g]; }
  int64_t& rhi(size_t g) const { return w[ng + g]; }
  int64_t& hbase(size_t g) const { return w[2 * ng + g]; }
  int64_t& hwidth(size_t g) const { return w[3 * ng + g]; }
  void range(size_t g, bool live, int64_t lo, int64_t hi) const {
    rlo(g) = live ? lo : 0;
    rhi(g) = live ? hi : 0;
  }
};

// The query staged for the device: one pinned block and its device copy, the scan parameters pointing into it.
struct XDev {
  hipStream_t st = nullptr;
  uint8_t *hbuf = nullptr, *dbuf = nullptr;
  size_t stage_bytes = 0, o_rng = 0, o_n = 0;
  XRanges rng;                 // host side
  uint32_t* hist = nullptr;    // host side: the histogram read back each pass
  uint32_t* d_hist = nullptr;
  XParams P{};
  float scan_ms = 0.f;
  // the scan between the two events, its time added to scan_ms once the caller has synchronized
  void scan(CallCtx& X) {
    HIP_TRY(hipEventRecord(X.ev_scan0, st));
    HIP_TRY(launch_ex_scan(P, st));
    HIP_TRY(hipEventRecord(X.ev_scan1, st));
  }
  void scanned(CallCtx& X) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, X.ev_scan0, X.ev_scan1));
    scan_ms += ms;
  }
};

struct Cand {
  int64_t ts;
  uint32_t qseg;
  uint32_t pos;       // segment position in the glob
  uint64_t row;       // row in the file
  unsigned long long ref;
};

// Every output column of the selected rows: raw values [nsel][ncols] and their non-NULL flags.
struct XGathered {
  std::vector<std::string> out_cols;
  std::vector<unsigned long long> val;
  std::vector<uint8_t> ok;
};

// ---- the stages both routes run, in call order ----
// The filter's leaves and numeric columns into qs (the operators the row scan evaluates; others: PlanError).
void x_leaves(const Request& R, XShape& qs);
// No segments: the sentinel DataPoint(-1, -1, {}) (Commons.scala:393-396).
void sentinel_row(const EvalCall& C, const XShape& qs);
XFilter x_filter(const EvalCall& C, const XShape& qs);
XGlobs x_globs(const EvalCall& C, const XShape& qs, const XFilter& fp);
std::vector<std::vector<uint32_t>> x_tables(Engine& E, const XFilter& fp);
XSegs x_segments(const XShape& qs, const XFilter& fp, XGlobs& gp);
XDev x_stage(const EvalCall& C, const XShape& qs, const XFilter& fp, const std::vector<std::vector<uint32_t>>& tabs,
             const XSegs& sg, size_t ng);
XGathered gather_columns(const EvalCall& C, const XGlobs& gp, const XSegs& sg, hipStream_t st,
                         const std::vector<const Cand*>& stream);
// Rows: timestamp, getDouble(value column) (SQL NULL -> 0.0), tags as JDBC getString text.  The value column is
// "_cardinalhq.value", or with `second_col` the second column of the row's glob (SELECT *: the union's U[1]).
// keep ([nsel][ncols], or null: every column): the columns a row may carry as tags.
void write_rows(const EvalCall& C, const XGlobs& gp, const XSegs& sg, const std::vector<const Cand*>& stream,
                const XGathered& G, bool second_col = false, const std::vector<uint8_t>* keep = nullptr);

}  // namespace lk
