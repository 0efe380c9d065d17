// Host-only test hook (include/lakeside_text.h): the filter planning of filter_plan.cpp for one request, in the order
// evaluate_once runs it -- the shape's leaf loop, the numeric groupBys as plan_numeric_group_bys leaves them,
// plan_filter, plan_truth -- written out as JSON (lk_filter_plan_sim); and the value leaves' rule of vleaf.hpp over the
// plan of a request that passed the shape gate's rule for p<NN> / ces charts (lk_vleaf_sim).
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/lakeside_text.h"
#include "eval_plan.hpp"
#include "hostutil.hpp"
#include "vleaf.hpp"

namespace {
std::string hex_words(const std::vector<uint32_t>& w) {
  std::string o = "[";
  char b[16];
  for (size_t i = 0; i < w.size(); i++) {
    snprintf(b, sizeof(b), "%s\"%08x\"", i ? "," : "", w[i]);
    o += b;
  }
  return o + "]";
}
int put(const std::string& s, int code, char* out, size_t cap) {
  if (!out || s.size() + 1 > cap) return LK_ERR_MEMORY;
  memcpy(out, s.c_str(), s.size() + 1);
  return code;
}
}  // namespace

extern "C" int lk_filter_plan_sim(const char* request_json, const char* const* numeric_group_bys, size_t n, char* out,
                                  size_t cap) {
  using namespace lk;
  if (out && cap) out[0] = 0;
  try {
    const Request R = parse_request(request_json);
    QueryShape qs;
    qs.tagq = R.is_tag_query && !R.tag_name.empty();
    qs.vcol = value_column(R);
    shape_leaves(R, qs);
    for (size_t i = 0; i < n; i++) {   // plan_numeric_group_bys: a groupBy some loaded file stores as a number
      const std::string gb = numeric_group_bys[i];
      qs.numgbs.push_back(gb);
      if (std::find(qs.nums.begin(), qs.nums.end(), gb) == qs.nums.end()) qs.nums.push_back(gb);
      qs.numeric = true;
    }
    FilterPlan fp;
    plan_filter(R, qs, fp);
    plan_truth(R, qs, fp);
    std::string o = "{\"cols\":[";
    for (size_t s = 0; s < fp.cols.size(); s++) o += std::string(s ? "," : "") + "\"" + json_escape(fp.cols[s].name) + "\"";
    o += "],\"leaves\":[";
    for (size_t i = 0; i < fp.leaves.size(); i++) {
      const LeafInfo& l = fp.leaves[i];
      o += std::string(i ? "," : "") + "{\"col\":" + std::to_string(l.str) + ",\"op\":\"" + json_escape(l.node->op) +
           "\",\"index\":" + std::to_string(l.index) + ",\"k\":\"" + json_escape(l.node->k) + "\"}";
    }
    o += "],\"nums\":[";
    for (size_t i = 0; i < qs.nums.size(); i++) o += std::string(i ? "," : "") + "\"" + json_escape(qs.nums[i]) + "\"";
    o += "],\"nleaves\":[";
    for (size_t i = 0; i < fp.nleaves.size(); i++) {
      const NumLeaf& nl = fp.nleaves[i];
      o += std::string(i ? "," : "") + "{\"col\":" + std::to_string(nl.col) + ",\"leaf\":" + std::to_string(nl.leaf) +
           ",\"lo_incl\":" + std::to_string(nl.lo_incl) + ",\"hi_incl\":" + std::to_string(nl.hi_incl) +
           ",\"nan_pass\":" + std::to_string(nl.nan_pass) + "}";
    }
    o += "],\"prog\":[";
    for (size_t i = 0; i < fp.prog.size(); i++) o += std::string(i ? "," : "") + std::to_string(unsigned(fp.prog[i]));
    o += "],\"truth\":" + hex_words(fp.truth) + ",\"truth_x\":" + hex_words(fp.truth_x) +
         ",\"truth_early\":" + hex_words(fp.truth_early) + ",\"truth_late\":" + hex_words(fp.truth_late) +
         ",\"vtab\":" + std::to_string(fp.vtab) + ",\"vleaf\":" + (fp.vleaf ? "1" : "0") +
         ",\"vleaf_shape\":" + (fp.vleaf_shape ? "1" : "0") + ",\"early\":" + std::to_string(fp.early) +
         ",\"late_mask\":" + std::to_string(fp.late_mask) + ",\"dev_of\":[";
    for (size_t i = 0; i < fp.dev_of.size(); i++) o += std::string(i ? "," : "") + std::to_string(fp.dev_of[i]);
    o += "],\"lead\":" + std::to_string(fp.lead) + "}";
    return put(o, LK_OK, out, cap);
  } catch (const PlanError& e) {
    const int rc = put(e.what(), e.code, out, cap);
    return rc == LK_ERR_MEMORY ? e.code : rc;
  } catch (const std::exception& e) {
    (void)put(e.what(), LK_ERR_ARG, out, cap);
    return LK_ERR_ARG;
  }
}

extern "C" int lk_vleaf_sim(const char* request_json, const uint8_t* valid, const double* vals, size_t n, int* vleaf,
                            uint8_t* pass, char* msg, size_t cap) {
  using namespace lk;
  if (msg && cap) msg[0] = 0;
  try {
    const Request R = parse_request(request_json);
    QueryShape qs;   // shape_gate's steps that the filter planning reads
    qs.tagq = R.is_tag_query && !R.tag_name.empty();
    shape_aggregation(R, qs);
    qs.metrics = R.dataset == "metrics" && !qs.tagq;
    qs.vcol = value_column(R);
    shape_leaves(R, qs);
    sketch_leaf_gate(R, qs);
    FilterPlan fp;
    plan_filter(R, qs, fp);
    plan_truth(R, qs, fp);
    sketch_leaf_check(qs, fp);
    if (vleaf) *vleaf = fp.vleaf ? 1 : 0;
    VLeaf vl[VLEAF_MAX] = {};
    const uint32_t nvl = fp.vleaf ? uint32_t(fp.nleaves.size()) : 0u;   // setup_scan fills QParams::vl the same way
    for (uint32_t k = 0; k < nvl; k++) vl[k] = vleaf_of(fp.nleaves[k]);
    for (size_t i = 0; i < n && pass; i++) pass[i] = fp.vleaf ? uint8_t(vleaf_pass(vl, nvl, fp.vtab, valid[i] != 0, vals[i])) : 0;
    return LK_OK;
  } catch (const PlanError& e) {
    (void)put(e.what(), e.code, msg, cap);
    return e.code;
  } catch (const std::exception& e) {
    (void)put(e.what(), LK_ERR_ARG, msg, cap);
    return LK_ERR_ARG;
  }
}
