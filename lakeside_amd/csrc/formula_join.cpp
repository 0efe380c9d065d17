// lk_eval_formula's rules over the request and over the operands' dimension texts (formula_join.hpp).  No HIP, no
// engine: formula_eval.cpp calls them between its device stages, liblakeside_text.so exports them to the CPU tests.
#include "formula_join.hpp"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <unordered_map>

#include "../../include/lakeside_gpu.h"

namespace lk {

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

namespace {

[[noreturn]] void refuse(const std::string& why) { throw PlanError(LK_ERR_UNSUPPORTED, "formula: " + why); }

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

// The expressions the program names, in the order of `expressions`; the program's leaves renumbered over them.
std::vector<FxExpr> referenced(const std::vector<std::string>& names, FxProgram& prog) {
  std::vector<int> leaf_of(names.size(), -1);
  std::vector<FxExpr> out;
  for (size_t v = 0; v < names.size(); v++) {
    bool used = false;
    for (int i = 0; i < prog.n; i++) used = used || (prog.ops[i].op == FX_LEAF && prog.ops[i].leaf == int32_t(v));
    if (!used) continue;
    leaf_of[v] = int(out.size());
    out.emplace_back();
    out.back().var = names[v];
  }
  for (int i = 0; i < prog.n; i++)
    if (prog.ops[i].op == FX_LEAF) prog.ops[i].leaf = leaf_of[size_t(prog.ops[i].leaf)];
  if (out.size() > size_t(FX_MAXLEAF))
    throw PlanError(LK_ERR_UNSUPPORTED, "formula: more than " + std::to_string(FX_MAXLEAF) + " expressions referenced");
  return out;
}

// One expression's request, paths and shard; the rules that read this request alone.  Returns its pushDown.
const Json& read_expression(const Json& ex, bool dist, int world, const FxParseRequest& parse, FxExpr& o) {
  const Json* pd = ex.get("pushDown");
  if (!pd || !pd->is_obj()) throw PlanError(LK_ERR_ARG, "formula: expression " + o.var + " has no pushDown");
  dump_json(*pd, o.push_down);
  o.R = parse(o.push_down);
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
  if (R.aggregation.size() > 1 && R.aggregation[0] == 'p' && R.dataset == "metrics" && !R.field_chart())
    refuse("expression " + o.var + ": metrics percentiles are assembled per row on the host");
  return *pd;
}

}  // namespace

FxCall fx_gate(const std::string& json, bool dist, int world, const FxParseRequest& parse) {
  const Json top = Json::parse(json);
  const Json* ftext = top.get("formula");
  const Json* exprs = top.get("expressions");
  if (!ftext || !ftext->is_str()) throw PlanError(LK_ERR_ARG, "formula: missing \"formula\"");
  if (!exprs || !exprs->is_obj()) throw PlanError(LK_ERR_ARG, "formula: missing \"expressions\"");
  std::vector<std::string> names;
  for (auto& kv : exprs->obj) names.push_back(kv.first);
  FxCall c;
  {
    std::string err;
    const int rc = parse_formula(ftext->str, names, c.prog, err);
    if (rc) throw PlanError(rc, err);
  }
  c.exprs = referenced(names, c.prog);
  for (size_t k = 0; k < c.exprs.size(); k++) {
    FxExpr& o = c.exprs[k];
    const Json& pd = read_expression(*exprs->get(o.var), dist, world, parse, o);
    const Request& R = *o.R;
    std::vector<std::string> gb = R.group_bys;
    std::sort(gb.begin(), gb.end());
    gb.erase(std::unique(gb.begin(), gb.end()), gb.end());
    if (k == 0) c.key_cols = gb;
    else if (gb != c.key_cols) refuse("expressions " + c.exprs[0].var + " and " + o.var + " have different groupBy sets");
    for (auto& s : R.segments) {
      if (s.step <= 0) throw PlanError(LK_ERR_ARG, "formula: expression " + o.var + ": stepInMillis must be positive");
      if (c.step && s.step != c.step) throw PlanError(LK_ERR_ARG, "formula: the expressions' steps differ");
      c.step = s.step;
    }
    o.xform = transformer_of(R, *pd.get("baseExpr"), o.var);
    const bool pct = R.aggregation.size() > 1 && R.aggregation[0] == 'p';
    o.uploaded = pct || R.aggregation == "ces" || (R.rollup.find("ces") != std::string::npos && R.dataset != "metrics");
  }
  if (c.key_cols.size() > size_t(FX_MAXCOL)) refuse("more than " + std::to_string(FX_MAXCOL) + " groupBy columns");
  c.secs = double(c.step / 1000);
  // evaluated in ascending byte order of the variable names: the order of a distributed call's collectives must not
  // depend on how a rank's caller ordered the JSON object (leaf numbers and a constant's tags keep reading `expressions`)
  c.order.resize(c.exprs.size());
  for (size_t k = 0; k < c.order.size(); k++) c.order[k] = k;
  std::sort(c.order.begin(), c.order.end(), [&](size_t a, size_t b) { return c.exprs[a].var < c.exprs[b].var; });
  return c;
}

namespace {

// Union ids of one key column: 0 = absent (nullptr, ""), equal texts equal ids.  A table column numbers its texts from
// 1 in order of first appearance; an identity column reads the dictionary and numbers what it lacks past ndim.
struct UnionCol {
  const FxIdentity* ident = nullptr;
  std::unordered_map<std::string, uint32_t> extra;
  uint32_t id(const char* s) {
    if (!s || !*s) return 0;
    if (ident) {
      const uint32_t d = ident->dict_id(s);
      if (d != FX_NO_ID && d + 1 < ident->ndim) return d + 1;   // a dim id of the dictionary (not dim_null)
    }
    auto it = extra.find(s);
    if (it != extra.end()) return it->second;
    const uint32_t nid = (ident ? ident->ndim : 0u) + 1u + uint32_t(extra.size());
    extra.emplace(s, nid);
    return nid;
  }
  unsigned long long size() const { return (unsigned long long)extra.size() + 1 + (ident ? ident->ndim : 0u); }
};

// The name dimension's ranks (2 * place in string order + 4); returns the sorted distinct texts.
std::vector<std::string> rank_names(const FxDim& nc, std::vector<uint32_t>& name_rank) {
  std::vector<std::string> texts;
  std::vector<const char*> nt(size_t(nc.ndim), nullptr);
  for (uint32_t d = 0; d < uint32_t(nc.ndim); d++) {
    nt[d] = nc.text(d);
    if (nt[d]) texts.emplace_back(nt[d]);
  }
  std::sort(texts.begin(), texts.end());
  texts.erase(std::unique(texts.begin(), texts.end()), texts.end());
  name_rank.assign(size_t(nc.ndim), FX_RANK_ABSENT);
  for (uint32_t d = 0; d < uint32_t(nc.ndim); d++)
    if (nt[d])
      name_rank[d] = 2u * uint32_t(std::lower_bound(texts.begin(), texts.end(), std::string(nt[d])) - texts.begin()) + 4u;
  return texts;
}

// A row whose own tags are all absent takes its glob's queryTags (Commons.scala:450-452; merged rows: the first
// glob's): its key reads the groupBy columns there, and its rank is its sorted tag list's place among the lists of the
// named rows of that key (2 * place + 3), or past the key's row without a name tag (formula_cell.hpp).
void key_query_tags(const std::vector<std::string>& key_cols, const FxOperandDims& o, const std::vector<std::string>& texts,
                    std::vector<UnionCol>& cols, FxOperandJoin& out) {
  TagList qt = o.query_tags;
  std::sort(qt.begin(), qt.end());
  TagList rest;   // the groupBy tags a named row of that key carries
  for (size_t j = 0; j < key_cols.size(); j++) {
    std::string v;
    for (auto& kv : qt)
      if (kv.first == key_cols[j]) v = kv.second;
    out.qt_ids[j] = cols[j].id(v.c_str());
    if (!v.empty()) rest.emplace_back(o.key[j].tag, v);
  }
  std::sort(rest.begin(), rest.end());
  bool noname_last = false;   // as fx_scatter ranks the key's row without a name tag
  for (auto& kv : rest) noname_last = noname_last || kv.first > o.name.tag;
  uint32_t place = 0;   // (no queryTags: the empty list sorts first)
  for (auto& nm : texts) {
    if (qt.empty()) break;
    TagList l = rest;
    l.emplace_back(o.name.tag, nm);
    std::sort(l.begin(), l.end());
    if (l < qt) place++;
  }
  out.qt_rank = 2u * place + 3u;
  if (!rest.empty()) {
    if (!noname_last && place == 0 && qt < rest) out.qt_rank = 0u;
    if (noname_last && place == texts.size() && rest < qt) out.qt_rank = FX_RANK_NONAME_LAST + 1u;
  }
}

}  // namespace

FxUnion fx_union_space(const std::vector<std::string>& key_cols, const std::vector<FxOperandDims>& ops,
                       const std::vector<FxIdentity>& ident) {
  const size_t nk = key_cols.size();
  std::vector<UnionCol> cols(nk);
  for (size_t j = 0; j < nk; j++)
    if (ident[j].on) cols[j].ident = &ident[j];
  FxUnion un;
  un.ops.resize(ops.size());
  for (size_t k = 0; k < ops.size(); k++) {
    const FxOperandDims& o = ops[k];
    FxOperandJoin& out = un.ops[k];
    out.map.resize(nk);
    out.qt_ids.assign(nk, 0);
    if (!o.has_rows) continue;   // (an expression without rows -- no segments, an empty glob -- is absent everywhere)
    for (size_t j = 0; j < nk; j++) {
      if (o.key[j].tag > o.name.tag) out.after_name |= 1u << j;
      if (ident[j].on) continue;
      if (o.key[j].ndim > 0xffffffffull) refuse("group dimension too large");
      out.map[j].resize(size_t(o.key[j].ndim));
      for (uint32_t d = 0; d < uint32_t(o.key[j].ndim); d++) out.map[j][d] = cols[j].id(o.key[j].text(d));
    }
    const std::vector<std::string> texts = rank_names(o.name, out.name_rank);
    key_query_tags(key_cols, o, texts, cols, out);
  }
  un.ustride.assign(nk, 1);
  for (size_t j = nk; j-- > 0;) {
    un.ustride[j] = un.U;
    const unsigned long long n = cols[j].size();
    if (un.U > (~0ull) / n) refuse("the union group space does not fit in 64 bits");
    un.U *= n;
  }
  for (FxOperandJoin& out : un.ops)
    for (size_t j = 0; j < nk; j++) out.qt_u += (unsigned long long)out.qt_ids[j] * un.ustride[j];
  return un;
}

FxCells fx_cell_space(int64_t base, int64_t last, int64_t step, unsigned long long U) {
  FxCells c;
  c.nbuckets = (unsigned long long)((last - base) / step) + 1;
  if (c.nbuckets > (1ull << 26)) refuse("more than 2^26 buckets");
  if (U > (~0ull - 1) / c.nbuckets) refuse("the cell key (buckets x union groups) does not fit in 64 bits");
  c.nkeys = c.nbuckets * U;
  return c;
}

}  // namespace lk
