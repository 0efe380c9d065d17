// Host-only test hooks (include/lakeside_text.h): the rules of formula_join.hpp as evaluate_formula calls them, JSON in
// and JSON out -- the gate with parse_request in place of the engine's request cache, the union group space over
// dimension texts given as arrays, an identity column's dictionary given as an object.
#include <cstring>
#include <string>

#include "../../include/lakeside_gpu.h"
#include "../../include/lakeside_text.h"
#include "formula_join.hpp"

namespace {
using namespace lk;

int put(const std::string& s, int code, char* out, size_t cap) {
  if (!out || s.size() + 1 > cap) return LK_ERR_MEMORY;
  memcpy(out, s.c_str(), s.size() + 1);
  return code;
}
std::string quoted(const std::string& s) {
  Json j;
  j.kind = Json::String;
  j.str = s;
  std::string o;
  dump_json(j, o);
  return o;
}
template <class V, class F>
std::string list(const V& v, F item) {
  std::string o = "[";
  for (size_t i = 0; i < v.size(); i++) o += (i ? "," : "") + item(v[i]);
  return o + "]";
}
template <class V>
std::string numbers(const V& v) {
  return list(v, [](auto x) { return std::to_string(x); });
}
// Runs `body` into out; a refusal's code is returned with its message in out.
template <class F>
int guarded(char* out, size_t cap, F body) {
  if (out && cap) out[0] = 0;
  try {
    return put(body(), LK_OK, out, cap);
  } catch (const PlanError& e) {
    (void)put(e.what(), e.code, out, cap);
    return e.code;
  } catch (const std::exception& e) {
    (void)put(e.what(), LK_ERR_ARG, out, cap);
    return LK_ERR_ARG;
  }
}

FxDim dim_of(const Json& j) {
  FxDim d;
  d.tag = j.get("tag")->str;
  if (const Json* a = j.get("dims")) {
    d.ndim = a->arr.size();
    d.text = [a](uint32_t i) { return a->arr[i].is_str() ? a->arr[i].str.c_str() : nullptr; };
  } else {   // a dimension that must not be walked (an identity column's)
    d.ndim = (unsigned long long)j.get("ndim")->as_i64();
    d.text = [](uint32_t) -> const char* { throw PlanError(LK_ERR_DEVICE, "internal: identity column walked"); };
  }
  return d;
}
}  // namespace

extern "C" int lk_formula_gate_sim(const char* formula_json, int dist, int world, char* out, size_t cap) {
  return guarded(out, cap, [&] {
    const FxCall c = fx_gate(formula_json, dist != 0, world,
                             [](const std::string& pd) { return std::make_shared<const Request>(parse_request(pd)); });
    static const char* const xf[] = {"none", "mul", "div"};
    std::string o = "{\"program\":" + quoted(formula_program_text(c.prog)) + ",\"operands\":";
    o += list(c.exprs, [](const FxExpr& e) {
      return "{\"var\":" + quoted(e.var) + ",\"paths\":" + list(e.paths, quoted) + ",\"shard\":" + numbers(e.shard) +
             ",\"uploaded\":" + (e.uploaded ? "true" : "false") + ",\"xform\":\"" + xf[e.xform] + "\"}";
    });
    o += ",\"order\":" + list(c.order, [&](size_t k) { return quoted(c.exprs[k].var); });
    o += ",\"key_cols\":" + list(c.key_cols, quoted) + ",\"step\":" + std::to_string(c.step) +
         ",\"secs\":" + std::to_string((long long)c.secs) + "}";
    return o;
  });
}

extern "C" int lk_formula_union_sim(const char* spec_json, char* out, size_t cap) {
  return guarded(out, cap, [&] {
    const Json top = Json::parse(spec_json);
    std::vector<std::string> key_cols;
    for (auto& k : top.get("key_cols")->arr) key_cols.push_back(k.str);
    std::vector<FxIdentity> ident(key_cols.size());
    if (const Json* ids = top.get("ident"))
      for (size_t j = 0; j < ident.size(); j++) {
        const Json& d = ids->arr[j];
        if (d.is_null()) continue;
        ident[j].on = true;
        ident[j].ndim = uint32_t(d.get("ndim")->as_i64());
        const Json* dict = d.get("dict");
        ident[j].dict_id = [dict](const char* s) {
          const Json* v = dict->get(s);
          return v ? uint32_t(v->as_i64()) : FX_NO_ID;
        };
      }
    std::vector<FxOperandDims> ops;
    for (auto& oj : top.get("operands")->arr) {
      ops.emplace_back();
      if (oj.is_null()) continue;   // an expression without rows
      FxOperandDims& o = ops.back();
      o.has_rows = true;
      o.name = dim_of(*oj.get("name"));
      for (auto& kj : oj.get("keys")->arr) o.key.push_back(dim_of(kj));
      for (auto& kv : oj.get("query_tags")->arr) o.query_tags.emplace_back(kv.arr[0].str, kv.arr[1].str);
    }
    const FxUnion un = fx_union_space(key_cols, ops, ident);
    std::string o = "{\"U\":" + std::to_string(un.U) + ",\"ustride\":" + numbers(un.ustride) + ",\"operands\":";
    o += list(un.ops, [](const FxOperandJoin& j) {
      return "{\"maps\":" + list(j.map, numbers<std::vector<uint32_t>>) + ",\"name_rank\":" + numbers(j.name_rank) +
             ",\"after_name\":" + std::to_string(j.after_name) + ",\"qt_ids\":" + numbers(j.qt_ids) +
             ",\"qt_u\":" + std::to_string(j.qt_u) + ",\"qt_rank\":" + std::to_string(j.qt_rank) + "}";
    });
    if (const Json* c = top.get("cells")) {
      const FxCells cs = fx_cell_space(c->get("base")->as_i64(), c->get("last")->as_i64(), c->get("step")->as_i64(), un.U);
      o += ",\"nbuckets\":" + std::to_string(cs.nbuckets) + ",\"nkeys\":" + std::to_string(cs.nkeys);
    }
    return o + "}";
  });
}
