// The rules of lk_eval_formula that read no segment and no device (formula_join.cpp): the parser call and the gate, the
// union group space with the collapse ranks, the cell space.  Free of HIP and of engine types, so that the CPU tests
// drive them through liblakeside_text.so (lk_formula_gate_sim, lk_formula_union_sim; formula_join_sim.cpp);
// formula_eval.cpp feeds them from the engine (parse_cached, lk_result::TagCol, GlobalDict).
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "formula.hpp"
#include "json.hpp"
#include "plan.hpp"

namespace lk {

void dump_json(const Json& j, std::string& o);

// ---- parse and gate: everything a call decides from its request alone ----
// One referenced expression, in the order of `expressions` (= its leaf number).
struct FxExpr {
  std::string var;
  std::string push_down;              // the pushDown object's text, as the evaluator parses it
  std::shared_ptr<const Request> R;
  std::vector<std::string> paths;
  std::vector<int32_t> shard;         // distributed: the rank of every path ("shard"); empty: i % world
  bool uploaded = false;              // values assembled on the host (p<NN>, ces): evaluated as usual, then uploaded
  int xform = FX_XF_NONE;             // ASTUtils.getTransformerFunc as one IEEE operation (FxXform)
};
struct FxCall {
  FxProgram prog;                     // leaves renumbered over the referenced expressions
  std::vector<FxExpr> exprs;
  std::vector<size_t> order;          // evaluation order: ascending byte order of the names
  std::vector<std::string> key_cols;  // the groupBy set, sorted (toGroupByKey sorts, ASTUtils.scala:87-89)
  int64_t step = 0;
  double secs = 0;                    // the Long quotient stepInMillis / 1000 (ASTUtils.scala:192)
};
using FxParseRequest = std::function<std::shared_ptr<const Request>(const std::string& push_down)>;
// Parses the call's JSON ({"formula", "expressions"}) and applies every rule that precedes the first collective: a
// PlanError / JsonError names the rule.  Unreferenced expressions are not read.  dist: the "shard" keys are read and
// checked against `world`.
FxCall fx_gate(const std::string& json, bool dist, int world, const FxParseRequest& parse);

// ---- union group space and collapse ranks ----
using TagList = std::vector<std::pair<std::string, std::string>>;
// A tag column's dimension as the join reads it: dim id -> text (nullptr: the tag is absent) for ids below ndim.
struct FxDim {
  std::string tag;                    // the column's tag name in the rows' tag lists
  unsigned long long ndim = 0;
  std::function<const char*(uint32_t)> text;
};
struct FxOperandDims {
  bool has_rows = false;              // an expression without rows is absent everywhere: nothing else is read
  FxDim name;                         // not part of the key: its rank, by text, decides the collapse
  std::vector<FxDim> key;             // per key column (an identity column's is not walked)
  TagList query_tags;                 // the first glob's queryTags (tag name, value): the tags of the all-absent row
};
// A key column every operand reads through one dictionary generation: union id = dictionary id + 1 without a table,
// however large the column.  Texts met outside the ids below ndim - 1 (queryTags) take ids past ndim.
constexpr uint32_t FX_NO_ID = 0xffffffffu;
struct FxIdentity {
  bool on = false;
  uint32_t ndim = 0;                                // the largest ndim among the operands (its last id reads absent)
  std::function<uint32_t(const char*)> dict_id;     // text -> dictionary id, FX_NO_ID when the dictionary lacks it
  uint32_t nl0 = FX_NO_ID, nl1 = FX_NO_ID;          // the dictionary's ids of "" and "null": absent too (the device's)
};
struct FxOperandJoin {
  std::vector<std::vector<uint32_t>> map;   // per key column: dim id -> union id (0: absent); empty: identity column
  std::vector<uint32_t> name_rank;          // name dim id -> 2 * (place in string order) + 4, FX_RANK_ABSENT
  uint32_t after_name = 0;                  // bit j: key column j's tag name sorts after the name column's
  std::vector<uint32_t> qt_ids;             // the all-absent row: its union id per key column (queryTags) ...
  unsigned long long qt_u = 0;              // ... their dot product with ustride ...
  uint32_t qt_rank = 1;                     // ... and its rank among the rows of that key
};
struct FxUnion {
  std::vector<FxOperandJoin> ops;
  std::vector<unsigned long long> ustride;  // row-major, the last column fastest
  unsigned long long U = 1;                 // product over the columns of (distinct texts + 1)
};
FxUnion fx_union_space(const std::vector<std::string>& key_cols, const std::vector<FxOperandDims>& ops,
                       const std::vector<FxIdentity>& ident);

// ---- cell space: buckets x union groups ----
struct FxCells {
  unsigned long long nbuckets = 0, nkeys = 0;
};
FxCells fx_cell_space(int64_t base, int64_t last, int64_t step, unsigned long long U);

}  // namespace lk
