// Plan helpers shared by the aggregate evaluator (eval_plan.cpp, eval.cpp) and the exemplar path (exemplar.cpp);
// defined in eval_plan.cpp unless noted (the filter tree's: filter_plan.cpp).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <unordered_set>
#include <vector>

#include "../../include/lakeside_gpu.h"
#include "engine.hpp"
#include "kernels.hpp"
#include "plan.hpp"
#include "regex.hpp"

namespace lk {

struct LeafInfo {
  const FilterNode* node;
  int str;      // string column index
  int index;    // global leaf index
};

// A string filter column: its leaves and their bits in the global leaf numbering.
struct LeafCol {
  std::string name;
  std::vector<const FilterNode*> leaves;
  uint32_t lbase = 0, lmask = 0, hmask = 0;
};
// The numbered leaves of a filter: string leaves column by column, then the numeric ones; the Kleene program.
struct LeafNumbering {
  std::vector<LeafInfo> leaves;
  std::vector<NumLeaf> nleaves;
  std::vector<std::string> bad_literal;   // fields whose numeric literal fails the SQL (per glob where they exist)
  std::vector<uint8_t> prog;
};

// One leaf on one dictionary value (BaseExpr.scala:470-501).
bool leaf_eval(const FilterNode& f, const std::string& s, re::Regex* re, const std::unordered_set<std::string>* set);
// regexp_matches(label, p, 'i') / contains' '.*p.*' as an RE2-semantics matcher (PlanError on a bad pattern).
re::Regex compile_leaf_regex(const FilterNode& l);
// Postfix Kleene program of the filter over numbered leaves.
void postfix(const FilterNode* n, const std::vector<LeafInfo>& leaves, std::vector<uint8_t>& prog);
void collect_leaves(const FilterNode* n, std::vector<const FilterNode*>& out);
// Truth table of a postfix program over L leaves: bit (T | F << L) = TRUE.
std::vector<uint32_t> truth_table(const std::vector<uint8_t>& prog, uint32_t L);
bool null_like(const std::string& s);
bool null_like(std::string_view s);
// Conjuncts of the filter's top-level AND chain (a AND (b AND c) -> a, b, c).
void conjuncts(const FilterNode* n, std::vector<const FilterNode*>& out);
// NoisyTagsDropper: tag names dropped from tag-query rows
bool noisy_tag(const std::string& t);
double ms_since(std::chrono::steady_clock::time_point t0);

// Exemplar queries (no chart): exemplar.cpp.
// numtag: a tag query (isTagQuery) whose tag column is numeric -- the same row scan planning (filter, globs,
// union_by_name types), counting passing rows per canonical tag value instead of selecting rows (ex_scan TAGNUM).
// dist: every rank evaluates the segments of its shard (shard[i] == rank; default i % world) as the worker of its pod
// would, and rank 0 folds the ranks' streams (exemplar: Akka mergeSorted in rank order, then query-api's take(limit);
// numeric tag: counts summed per tag text).
int evaluate_exemplar(Engine& E, CallCtx& X, const Request& R, const char* const* paths, size_t n_paths,
                      int glob_size, unsigned flags, bool dist, lk_result* res, const std::string& numtag = std::string(),
                      const int32_t* shard = nullptr);
// Tag-name queries (isTagQuery without a tagDataType): tagnames.cpp.  Local calls only (dist: LK_ERR_UNSUPPORTED).
int evaluate_tagnames(Engine& E, CallCtx& X, const Request& R, const char* const* paths, size_t n_paths, int glob_size,
                      unsigned flags, bool dist, lk_result* res);
// Numeric comparison leaves (numleaf.cpp): gt / ge / lt / le; the normalized literal (PlanError(LK_ERR_ARG) where the
// reference's SQL fails); the leaf's interval on numeric filter column `col`.
bool numeric_op(const std::string& op);
double normalized_value(const FilterNode& f);
NumLeaf make_num_leaf(const FilterNode& f, uint32_t col, uint32_t leaf, bool& bad);
// Numbers the leaves of `cols` (lbase / lmask / hmask), then the leaves `is_num` takes -- a comparison (make_num_leaf), or
// any other operator as IS NOT NULL (NUMLEAF_NOTNULL: the exemplar path's numeric tag) -- on their column of `nums`, and
// compiles the filter; refuses more than LEAF_BITS leaves on a column and a program beyond MAXPROG.
template <class Col, class IsNum>
LeafNumbering number_leaves(const FilterNode* filter, const std::vector<const FilterNode*>& all_leaves, IsNum is_num,
                            const std::vector<std::string>& nums, std::vector<Col>& cols) {
  LeafNumbering n;
  for (size_t s = 0; s < cols.size(); s++) {
    LeafCol& sc = cols[s];
    if (sc.leaves.size() > size_t(LEAF_BITS)) throw PlanError(LK_ERR_UNSUPPORTED, "too many leaves on one column");
    sc.lbase = uint32_t(n.leaves.size());
    for (const FilterNode* l : sc.leaves) {
      const uint32_t idx = uint32_t(n.leaves.size());
      n.leaves.push_back(LeafInfo{l, int(s), int(idx)});
      sc.lmask |= 1u << idx;
      if (l->op == "has" || l->op == "exists") sc.hmask |= 1u << idx;
    }
  }
  for (auto* l : all_leaves)
    if (is_num(l)) {
      const uint32_t idx = uint32_t(n.leaves.size());
      n.leaves.push_back(LeafInfo{l, -1, int(idx)});
      const uint32_t col = uint32_t(std::find(nums.begin(), nums.end(), l->k) - nums.begin());
      bool bad = false;
      NumLeaf nl{};
      if (numeric_op(l->op)) {
        nl = make_num_leaf(*l, col, idx, bad);
      } else {   // "<tag>" IS NOT NULL
        nl.col = col;
        nl.leaf = idx;
        nl.pad = NUMLEAF_NOTNULL;
      }
      n.nleaves.push_back(nl);
      if (bad) n.bad_literal.push_back(l->k);
    }
  postfix(filter, n.leaves, n.prog);
  if (n.prog.size() > size_t(MAXPROG)) throw PlanError(LK_ERR_UNSUPPORTED, "filter too large");
  return n;
}

// Leaf outcomes over a column's dictionary values [0, dict_n) (immutable: StableStrs), cached per (column, leaves) in
// the engine and extended here over the values added since: a regex runs once per distinct value.  skip[j] != 0: leaf
// j's pattern is not compiled and its bit stays 0; without `skip` a pattern RE2 rejects throws.  Returns the entry
// with its lock held.
struct LockedLeafBits {
  std::shared_ptr<LeafBits> lb;
  std::unique_lock<std::mutex> guard;
};
LockedLeafBits extend_leaf_bits(Engine& E, const LeafCol& sc, const GlobalDict& gd, uint32_t dict_n,
                                const std::vector<char>* skip = nullptr);

// Java 17 Double.toString / Float.toString text (jdtoa.cpp).
std::string java_text(double d);
std::string java_text(float f);
// JDBC getString text of a raw value of Parquet physical type `pt` read as union_by_name type `ut`; a raw 64-bit word
// of type `ptype` as a double (numgroup_agree.cpp).
std::string value_text(unsigned long long raw, int pt, int ut);
double raw_as_double(unsigned long long raw, int ptype);
// A test knob of the environment, read on every call (exemplar.cpp).
uint64_t env_u64(const char* name, uint64_t dflt, uint64_t floor);

}  // namespace lk
