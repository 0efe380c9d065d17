// Tag-name queries (isTagQuery without a tagDataType), the pure part: what the request and the globs' schemas decide
// (tn_gate) and the fold of the per-column first keys into rows (tn_rows).  No HIP and no engine include: the evaluator
// (tagnames.cpp) and the host-only test hooks (tagnames_sim.cpp) call the same functions.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "plan.hpp"

namespace lk {

constexpr const char* kTnPrefix = "tag queries without a tagDataType: ";
constexpr unsigned long long TN_NONE = ~0ull;   // a column without a first key

// One file's columns in file order: (name, Parquet physical type; -1: a nested group).
using TnSchema = std::vector<std::pair<std::string, int>>;
// A glob's readable files in list order.
using TnGlob = std::vector<TnSchema>;

[[noreturn]] inline void tn_refuse(const std::string& why) { throw PlanError(LK_ERR_UNSUPPORTED, kTnPrefix + why); }

// The union schema of read_parquet([...], union_by_name=True): files in list order, each file's columns in their own
// order, a name's first appearance fixes its place.
inline std::vector<std::string> tn_union(const TnGlob& g) {
  std::vector<std::string> u;
  for (auto& f : g)
    for (auto& c : f)
      if (std::find(u.begin(), u.end(), c.first) == u.end()) u.push_back(c.first);
  return u;
}

// The request alone.
inline void tn_gate_request(const Request& R, bool dist) {
  if (dist) tn_refuse("lk_eval_pushdown_dist does not evaluate them");
  if (R.has_extract || R.has_compute) tn_refuse("extract / compute are not on the hot path");
  if (R.has_chart) tn_refuse("the request carries a chart (query-api's evaluateTagQuery sends none)");
  if (!R.tag_name_compression)
    tn_refuse("processor.tagNameCompressionEnabled is not set (the reference then streams every passing row)");
  if (R.reset_value_to_field) tn_refuse("processor.resetValueToField is set");
}

// One glob's schemas: branch T (the union's first column is the timestamp) with a second column getDouble reads as a
// number of one type.  Returns the union.
inline std::vector<std::string> tn_gate_glob(const TnGlob& g, size_t gi) {
  const std::vector<std::string> u = tn_union(g);
  const std::string at = " of glob " + std::to_string(gi);
  if (u.empty()) return u;
  if (u[0] != "_cardinalhq.timestamp")
    tn_refuse("the first column" + at + " is " + u[0] + ", not _cardinalhq.timestamp (every row would be emitted whole)");
  if (u.size() < 2) tn_refuse("the union" + at + " has no second column for the value");
  int vt = -2;
  for (auto& f : g)
    for (auto& c : f) {
      if (c.first != u[1]) continue;
      if (c.second != 1 && c.second != 2 && c.second != 4 && c.second != 5)   // INT32, INT64, FLOAT, DOUBLE
        tn_refuse("the second column " + u[1] + at + " is not INT32 / INT64 / FLOAT / DOUBLE (getDouble of it is unpinned)");
      if (vt != -2 && vt != c.second)
        tn_refuse("the second column " + u[1] + at + " has different numeric types in the glob's files");
      vt = c.second;
    }
  return u;
}

// Everything the request and the schemas decide; the unions per glob.
inline std::vector<std::vector<std::string>> tn_gate(const Request& R, bool dist, const std::vector<TnGlob>& globs) {
  tn_gate_request(R, dist);
  std::vector<std::vector<std::string>> us;
  for (size_t gi = 0; gi < globs.size(); gi++) us.push_back(tn_gate_glob(globs[gi], gi));
  return us;
}

// The emitted rows: the distinct first keys in ascending order (the stand-in row order: glob, file position, tile, row),
// each with the columns whose first key it is, ascending.
struct TnRow {
  unsigned long long key;
  std::vector<uint32_t> cols;
};
inline std::vector<TnRow> tn_rows(const unsigned long long* first, size_t n) {
  std::vector<std::pair<unsigned long long, uint32_t>> kc;
  for (size_t k = 0; k < n; k++)
    if (first[k] != TN_NONE) kc.emplace_back(first[k], uint32_t(k));
  std::sort(kc.begin(), kc.end());
  std::vector<TnRow> rows;
  for (auto& p : kc) {
    if (rows.empty() || rows.back().key != p.first) rows.push_back(TnRow{p.first, {}});
    rows.back().cols.push_back(p.second);
  }
  return rows;
}

}  // namespace lk
