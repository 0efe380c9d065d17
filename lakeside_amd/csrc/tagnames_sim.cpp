// Host-only test hooks (include/lakeside_text.h): the rules of tagnames.hpp as the evaluator calls them -- the gate with
// parse_request in place of the engine's request cache and the globs' schemas given as JSON, the row fold over first keys
// given as an array.
#include <cstring>
#include <string>

#include "../../include/lakeside_gpu.h"
#include "../../include/lakeside_text.h"
#include "formula_join.hpp"   // dump_json
#include "tagnames.hpp"

namespace {
using namespace lk;

int put(const std::string& s, int code, char* out, size_t cap) {
  if (!out || s.size() + 1 > cap) return LK_ERR_MEMORY;
  memcpy(out, s.c_str(), s.size() + 1);
  return code;
}
}  // namespace

extern "C" int lk_tagnames_gate_sim(const char* request_json, const char* schemas_json, int dist, char* out, size_t cap) {
  if (out && cap) out[0] = 0;
  try {
    const Request R = parse_request(request_json);
    const Json top = Json::parse(schemas_json);
    std::vector<TnGlob> globs;
    for (auto& gj : top.arr) {
      globs.emplace_back();
      for (auto& fj : gj.arr) {
        globs.back().emplace_back();
        for (auto& cj : fj.arr) globs.back().back().emplace_back(cj.arr[0].str, int(cj.arr[1].as_i64()));
      }
    }
    const std::vector<std::vector<std::string>> us = tn_gate(R, dist != 0, globs);
    std::string o = "{\"unions\":[";
    for (size_t g = 0; g < us.size(); g++) {
      o += g ? ",[" : "[";
      for (size_t k = 0; k < us[g].size(); k++) {
        Json j;
        j.kind = Json::String;
        j.str = us[g][k];
        if (k) o += ",";
        dump_json(j, o);
      }
      o += "]";
    }
    return put(o + "]}", LK_OK, out, cap);
  } catch (const PlanError& e) {
    (void)put(e.what(), e.code, out, cap);
    return e.code;
  } catch (const std::exception& e) {
    (void)put(e.what(), LK_ERR_ARG, out, cap);
    return LK_ERR_ARG;
  }
}

extern "C" long lk_tagnames_rows_sim(const uint64_t* first, size_t n, uint64_t* keys, uint32_t* row_of_col, size_t cap) {
  const std::vector<TnRow> rows = tn_rows(reinterpret_cast<const unsigned long long*>(first), n);
  if (rows.size() > cap) return LK_ERR_MEMORY;
  for (size_t k = 0; k < n; k++) row_of_col[k] = 0xffffffffu;
  for (size_t i = 0; i < rows.size(); i++) {
    keys[i] = rows[i].key;
    for (uint32_t k : rows[i].cols) row_of_col[k] = uint32_t(i);
  }
  return long(rows.size());
}
