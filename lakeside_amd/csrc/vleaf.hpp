// The rule that decides whether a row's value passes the numeric comparison leaves on the value column (`gt` / `ge` /
// `lt` / `le`, BaseExpr.scala:488-498, in conjuncts of their own: FilterPlan::vleaf), stated once and pinned on the
// CPU (tests/test_vleaf_cpu.py through lk_vleaf_sim, filter_plan_sim.cpp).  Plain C++ over layout.hpp's VLeaf: the
// kernels inline it, the host hook compiles it as is.  It touches no memory but the leaves it is handed.
// Callers: scan_tiles' consume (COUNT instantiations: COUNT, p<NN>, ces).  scan_lean's row still writes the same
// lines out (lean_kernel.hpp): through a shared function that kernel's register allocation has changed before
// (on bucket_row), and its tiles hold no NULL value, so it needs no `valid`.
#pragma once
#include <stdint.h>

#include "layout.hpp"

#if defined(__HIPCC__)
#define LK_VL_HD __host__ __device__ __attribute__((always_inline))
#else
#define LK_VL_HD
#endif

namespace lk {

// One leaf on one non-NULL value: NaN (DuckDB orders it greatest) passes iff nan_pass; any other value by the bounds.
LK_VL_HD inline bool vleaf_one(const VLeaf& l, double v) {
  return v != v ? l.nan_pass != 0u
                : ((v > l.lo || (l.lo_incl && v == l.lo)) && (v < l.hi || (l.hi_incl && v == l.hi)));
}

// The value-leaf conjuncts of a row.  A NULL value (`!valid`) fails: every leaf of a value-only conjunct is UNKNOWN,
// and Kleene and / or / not over nothing but UNKNOWN is UNKNOWN, which WHERE drops.  Otherwise bit k of the index is
// leaf k's outcome and bit `index` of vtab decides (plan_truth builds vtab from the numeric conjuncts' truth table).
// nvl <= VLEAF_MAX, so the index stays below 32.  The loop is rolled on purpose: a kernel hands `vl` as a pointer
// into its kernarg segment, and an unrolled loop would hold every leaf's bounds in SGPRs.
LK_VL_HD inline bool vleaf_pass(const VLeaf* vl, uint32_t nvl, uint32_t vtab, bool valid, double v) {
  if (!valid) return false;
  uint32_t bits = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t k = 0; k < nvl; k++) bits |= uint32_t(vleaf_one(vl[k], v)) << k;
  return (vtab >> bits) & 1u;
}

}  // namespace lk
