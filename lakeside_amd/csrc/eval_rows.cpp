// The result's tag columns: how a row's group id decodes to its tag strings.
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "engine.hpp"
#include "eval_plan.hpp"
#include "evalutil.hpp"

namespace lk {

void label_rows(const EvalCall& C, const Plan& pl, uint32_t nrows_out) {
  // ---- tags: "name", groupBys (as written), then queryTags keys (rows whose own tags are all absent) ----
  std::vector<int> col_str;   // tag column -> string column index
  C.res->tag_names.push_back(pl.qs.tagq ? C.R.tag_name : std::string("name"));
  col_str.push_back(0);
  if (!pl.qs.tagq)
    for (auto& g : C.R.group_bys) {
      C.res->tag_names.push_back(g);
      col_str.push_back(pl.dim_index(g));   // a string column, or a numeric group dimension
    }
  const size_t nreg = C.res->tag_names.size();
  std::vector<std::string> qt_keys;
  for (auto& g : pl.gp.globs)
    for (auto& kv : g.query_tags)
      if (!pl.qs.tagq && !pl.qs.sketch && !pl.qs.ces && std::find(qt_keys.begin(), qt_keys.end(), kv.first) == qt_keys.end()) qt_keys.push_back(kv.first);
  for (auto& k : qt_keys) C.res->tag_names.push_back(k);
  // Per tag column: how a row's group id decodes to the tag string (lk_result::tag; nullptr: tag dropped,
  // Commons.scala:433).  Strings local to this call (filter candidates, the distributed union) move into the
  // result once; engine-dictionary strings are read in place (stable addresses, StableStrs).
  C.res->per_glob = pl.qs.per_glob_rows;
  C.res->tcols.resize(nreg);
  for (size_t c = 0; c < nreg; c++) {
    const DimCol& sc = pl.dp.dims[size_t(col_str[c])];
    const std::string& name = pl.dim_name(size_t(col_str[c]));
    lk_result::TagCol& tc = C.res->tcols[c];
    tc.stride = sc.stride ? sc.stride : 1;
    tc.ndim = sc.ndim;
    tc.dim_null = sc.dim_null;
    tc.col = name;
    if (!sc.numeric) {   // (a numeric dimension's strings are this result's own: `local` + `owned` below)
      GlobalDict& gd = C.E.dict(name);
      std::lock_guard<std::mutex> g(gd.mu);
      tc.dict_keep = gd.vals;   // this generation's block stays alive with the result
      tc.dict = tc.dict_keep.get();
      tc.engine = &C.E;
      tc.engine_life = C.E.life;
      tc.dict_n = sc.dict_n;
    }
    if (sc.exchanged) {   // the agreed union's text table, shared (no copy): 10M-value dims cost nothing here
      tc.shared = sc.uni->text;
      tc.keep = sc.uni;
      continue;
    }
    if (!sc.restricted) continue;
    auto& m = tc.local;
    bool shared = false;
    for (size_t c2 = 0; c2 < c && !shared; c2++)   // a groupBy listed twice shares the first column's strings
      if (col_str[c2] == col_str[c] && !C.res->tcols[c2].local.empty()) {
        m = C.res->tcols[c2].local;
        shared = true;
      }
    if (shared) continue;
    m.assign(sc.ndim, nullptr);
    for (uint32_t d = 0; d < sc.ndim; d++) {
      if (d == sc.dim_null) continue;
      const std::string& v = sc.cand[d];
      if (null_like(v)) continue;
      C.res->owned.push_back(v);                                 // a few filter candidates: copied
      m[d] = C.res->owned.back().c_str();
    }
  }
  if (pl.qs.sketch && pl.fp.gbs.empty()) {   // key tags {"_cardinalhq.name": ""} (getOrElse(NAME, ""): see sketch_rows, eval.cpp)
    C.res->tag_names[0] = kName;
    lk_result::TagCol& tc = C.res->tcols[0];
    tc = lk_result::TagCol{};    // one dim id, whose text is ""
    tc.ndim = 1;
    tc.dim_null = 1;
    C.res->owned.push_back(std::string());
    tc.local.assign(1, C.res->owned.back().c_str());
  }
  if (pl.qs.sketch && !pl.fp.gbs.empty()) C.res->tcols[0].hidden = true;     // key tags: the groupBys only
  if (pl.qs.ces)   // the HLL SketchInput carries no tags (Aggregator.scala:58)
    for (auto& tc : C.res->tcols) tc.hidden = true;
  if (pl.qs.tagq) {
    // Tag-query rows (Commons.toDataPoint, Commons.scala:406-423): every column becomes a tag -- the tag and
    // "count" (COUNT(*) via getString) -- then NoisyTagsDropper.remove (NoisyTagsDropper.scala) drops hidden
    // tag names and NULL / "" / "null" values; timestamp = System.currentTimeMillis(), value 0.0 in the
    // reference (unused downstream: the payload is the tag map, QueryEngineV2.scala:473-477).  Here `value`
    // carries the count.
    C.res->tcols[0].hidden = noisy_tag(C.R.tag_name);
    C.res->tag_names.push_back("count");
    C.res->count_col = int(C.res->tag_names.size() - 1);
    C.res->count_str.reserve(nrows_out);
    const int64_t now_ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                               std::chrono::system_clock::now().time_since_epoch()).count();
    for (size_t r = 0; r < nrows_out; r++) {
      C.res->ts[r] = now_ms;
      C.res->count_str.push_back(std::to_string((unsigned long long)C.res->val[r]));
    }
  }
  C.res->qt_of_glob.resize(pl.gp.globs.size());
  for (size_t gi = 0; gi < pl.gp.globs.size() && !pl.qs.sketch && !pl.qs.ces; gi++)
    for (auto& kv : pl.gp.globs[gi].query_tags) {
      size_t c = nreg + size_t(std::find(qt_keys.begin(), qt_keys.end(), kv.first) - qt_keys.begin());
      C.res->owned.push_back(kv.second);
      C.res->qt_of_glob[gi].emplace_back(c, C.res->owned.back().c_str());
    }
}

}  // namespace lk
