// Numeric groupBys: the two rules every rank of a distributed evaluation applies to agreed data, free of
// device and communicator types.  numgroup_agree.cpp; liblakeside_text.so exposes them (lk_numgroup_classes_sim,
// lk_numgroup_values_sim) and the evaluator calls the same functions, sharded or not.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace lk {

// What the files of one glob say about one groupBy column, as three bytes whose element-wise max over files -- and
// over ranks -- is union_by_name: a VARCHAR file, a BOOLEAN file, the largest value_rank of a numeric file
// (INTEGER 1 < BIGINT 2 < FLOAT 3 < DOUBLE 4; 0: none).
struct GbClass {
  uint8_t text = 0, boolean = 0, rank = 0;
  bool numeric() const { return boolean || rank; }
};
constexpr size_t kGbClassBytes = 3;
int value_rank(int ptype);            // 0: not a numeric type a value column can have
int value_type_of_rank(int r);        // -1 for rank 0
// One file's column (Parquet physical type; a string column whatever its type) into the glob's class.
void gb_class_add(GbClass& c, bool is_string, int ptype);
GbClass gb_class_max(const GbClass& a, const GbClass& b);

enum GbRefusal : int { GB_OK = 0, GB_TEXT_WITH_NUMBER = 1, GB_BOOLEAN_WITH_NUMBER = 2 };
// The glob's union_by_name type of the column from its class: the Parquet physical type of the numeric union, BOOLEAN
// alone, BYTE_ARRAY for VARCHAR alone, -1 when no file has the column; or the union this engine does not restate.
GbRefusal gb_class_union(const GbClass& c, int* union_type);

// JDBC getString text of the canonical key `key` (ex_kernels.hip: tag_key) of a glob whose union type is `ut`.
std::string numdim_key_text(int ut, unsigned long long key);
// Sorted union of the ranks' text sets: a dimension's id is a text's position in it.
std::vector<std::string> numdim_text_union(const std::vector<std::vector<std::string>>& per_rank);
// (the text must be in the union)
uint32_t numdim_id_of(const std::vector<std::string>& uni, const std::string& text);

// Byte encoding of text lists for the exchange: count (4) then per text length (4) + bytes.  get_* throws PlanError on
// a short blob and advances `at`.
void put_texts(std::string& blob, const std::vector<std::string>& texts);
std::vector<std::string> get_texts(const std::string& blob, size_t& at);

}  // namespace lk
