// Numeric groupBys, the rules over agreed data (numgroup_agree.hpp): a glob's union_by_name class of a groupBy column
// from per-file / per-rank class bytes, the text of a canonical key, the ids of a dimension from the ranks' text sets.
// Host-only; also built into liblakeside_text.so for the CPU tests (lk_numgroup_classes_sim / lk_numgroup_values_sim).
#include "numgroup_agree.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/lakeside_gpu.h"
#include "../../include/lakeside_text.h"
#include "evalutil.hpp"
#include "parquet.hpp"
#include "plan.hpp"

namespace lk {

// union_by_name over a glob's files unifies a numeric column to the widest of its physical types in DuckDB's order
// INTEGER < BIGINT < FLOAT < DOUBLE (the same rule exemplar.cpp's union_type applies to tag text).  Rank 0: not a
// numeric type a value column can have.
int value_rank(int ptype) {
  switch (ptype) {
    case pq::INT32: return 1;
    case pq::INT64: return 2;
    case pq::FLOAT: return 3;
    case pq::DOUBLE: return 4;
    default: return 0;
  }
}
int value_type_of_rank(int r) {
  static const int t[5] = {-1, pq::INT32, pq::INT64, pq::FLOAT, pq::DOUBLE};
  return t[r < 0 || r > 4 ? 0 : r];
}

// A raw 64-bit word of Parquet physical type `ptype` as a double: DOUBLE / FLOAT bit patterns, INT32 / INT64 values.
double raw_as_double(unsigned long long raw, int ptype) {
  switch (ptype) {
    case pq::DOUBLE: {
      double d;
      memcpy(&d, &raw, 8);
      return d;
    }
    case pq::INT64: return double(int64_t(raw));
    case pq::INT32: return double(int32_t(uint32_t(raw)));
    case pq::FLOAT: {
      float f;
      const uint32_t u = uint32_t(raw);
      memcpy(&f, &u, 4);
      return double(f);
    }
    default: throw PlanError(LK_ERR_UNSUPPORTED, "exemplar value column of a non-numeric type");
  }
}

// JDBC getString text of a raw value of physical type `pt` read as union type `ut`.
std::string value_text(unsigned long long raw, int pt, int ut) {
  int64_t iv = 0;
  float fv = 0.0f;
  switch (pt) {
    case pq::INT64: iv = int64_t(raw); fv = float(iv); break;
    case pq::INT32: iv = int32_t(uint32_t(raw)); fv = float(iv); break;
    case pq::DOUBLE: break;
    case pq::FLOAT: fv = float(raw_as_double(raw, pt)); break;
    case pq::BOOLEAN: return raw ? "true" : "false";
    default: throw PlanError(LK_ERR_UNSUPPORTED, "exemplar column of an undecoded type");
  }
  switch (ut) {
    case pq::INT64:
    case pq::INT32: return std::to_string(iv);
    case pq::FLOAT: return java_text(fv);
    default: return java_text(raw_as_double(raw, pt));
  }
}

void gb_class_add(GbClass& c, bool is_string, int ptype) {
  if (is_string) c.text = 1;
  else if (ptype == pq::BOOLEAN) c.boolean = 1;
  else c.rank = std::max<uint8_t>(c.rank, uint8_t(value_rank(ptype)));
}

GbClass gb_class_max(const GbClass& a, const GbClass& b) {
  GbClass m;
  m.text = std::max(a.text, b.text);
  m.boolean = std::max(a.boolean, b.boolean);
  m.rank = std::max(a.rank, b.rank);
  return m;
}

GbRefusal gb_class_union(const GbClass& c, int* union_type) {
  if (union_type) *union_type = -1;
  // union_by_name of VARCHAR and a number is VARCHAR, the numbers printed by DuckDB's cast; BOOLEAN with a number does
  // not unify as the numeric classes do
  if (c.text && c.numeric()) return GB_TEXT_WITH_NUMBER;
  if (c.boolean && c.rank) return GB_BOOLEAN_WITH_NUMBER;
  if (union_type) *union_type = c.text ? int(pq::BYTE_ARRAY) : (c.boolean ? int(pq::BOOLEAN) : value_type_of_rank(c.rank));
  return GB_OK;
}

std::string numdim_key_text(int ut, unsigned long long key) {
  if (ut != pq::BOOLEAN && !value_rank(ut)) throw PlanError(LK_ERR_DEVICE, "internal: numeric groupBy value in a glob without the column");
  return value_text(key, ut, ut);
}

std::vector<std::string> numdim_text_union(const std::vector<std::vector<std::string>>& per_rank) {
  std::vector<std::string> u;
  for (auto& r : per_rank) u.insert(u.end(), r.begin(), r.end());
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  return u;
}

uint32_t numdim_id_of(const std::vector<std::string>& uni, const std::string& text) {
  const auto it = std::lower_bound(uni.begin(), uni.end(), text);
  if (it == uni.end() || *it != text) throw PlanError(LK_ERR_DEVICE, "internal: a numeric groupBy text outside the agreed union");
  return uint32_t(it - uni.begin());
}

void put_texts(std::string& blob, const std::vector<std::string>& texts) {
  const uint32_t n = uint32_t(texts.size());
  blob.append(reinterpret_cast<const char*>(&n), 4);
  for (auto& t : texts) {
    const uint32_t l = uint32_t(t.size());
    blob.append(reinterpret_cast<const char*>(&l), 4);
    blob += t;
  }
}

std::vector<std::string> get_texts(const std::string& blob, size_t& at) {
  auto u32 = [&]() {
    if (at + 4 > blob.size()) throw PlanError(LK_ERR_DEVICE, "internal: short numeric groupBy value exchange");
    uint32_t v;
    memcpy(&v, blob.data() + at, 4);
    at += 4;
    return v;
  };
  const uint32_t n = u32();
  std::vector<std::string> out;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = u32();
    if (at + l > blob.size()) throw PlanError(LK_ERR_DEVICE, "internal: short numeric groupBy value exchange");
    out.emplace_back(blob, at, l);
    at += l;
  }
  return out;
}

}  // namespace lk

extern "C" int lk_numgroup_classes_sim(const uint8_t* classes, size_t n_ranks, int* union_type) {
  lk::GbClass c;
  for (size_t r = 0; r < n_ranks; r++)
    c = lk::gb_class_max(c, lk::GbClass{classes[r * lk::kGbClassBytes], classes[r * lk::kGbClassBytes + 1], classes[r * lk::kGbClassBytes + 2]});
  if (c.rank > 4) {
    if (union_type) *union_type = -1;
    return LK_ERR_ARG;
  }
  return int(lk::gb_class_union(c, union_type));
}

extern "C" int lk_numgroup_file_class(int is_string, int ptype, uint8_t* out3) {
  lk::GbClass c;
  lk::gb_class_add(c, is_string != 0, ptype);
  out3[0] = c.text;
  out3[1] = c.boolean;
  out3[2] = c.rank;
  return 0;
}

extern "C" long lk_numgroup_values_sim(const int32_t* union_types, const uint64_t* keys, const size_t* counts, size_t n_ranks,
                                       uint32_t* ids, char* out, size_t cap) {
  if (out && cap) out[0] = 0;
  try {
    std::vector<std::vector<std::string>> per_rank(n_ranks);
    std::vector<std::string> text;
    size_t at = 0;
    for (size_t r = 0; r < n_ranks; r++)
      for (size_t i = 0; i < counts[r]; i++, at++) {
        text.push_back(lk::numdim_key_text(union_types[at], keys[at]));
        per_rank[r].push_back(text.back());
      }
    const std::vector<std::string> uni = lk::numdim_text_union(per_rank);
    for (size_t i = 0; i < text.size(); i++) ids[i] = lk::numdim_id_of(uni, text[i]);
    std::string o;
    for (size_t i = 0; i < uni.size(); i++) o += (i ? "\n" : "") + uni[i];
    if (!out || o.size() + 1 > cap) return LK_ERR_MEMORY;
    memcpy(out, o.c_str(), o.size() + 1);
    return long(uni.size());
  } catch (const lk::PlanError& e) {
    if (out && cap) snprintf(out, cap, "%s", e.what());
    return e.code;
  }
}
