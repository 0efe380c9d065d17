// The reduction of one code's range of a pinned tile of the name-clustered value copy (layout.hpp, CluTile), stated
// once: scan_clu (clu_kernel.hpp) runs it over a pinned tile's passing ranges when it streams them, and clu_build
// (clu_kernels.hip) runs it at load over every code's range to fill the tile's `cagg` entries, which scan_clu then
// merges instead of streaming.  One function, so the stored aggregates are what the stream hands global_merge, bit
// for bit: lane l accumulates elements l, l + 64, l + 128, ... in that order (TwoSum per add), then the wave combines
// through the __shfl_xor tree (TwoSum of the partial sums, lo + ol + e); MIN / MAX over dbl_order.
#pragma once
#include "device_common.hpp"

namespace lk {

struct CluRed {                 // uniform after the tree (every lane holds the wave's result)
  uint32_t cnt;
  double hi, lo;                // SUM
  unsigned long long omin, omax;   // MIN / MAX: dbl_order extremes (~0 / 0 of an empty range)
  bool nan;                     // MIN: a NaN was seen (wave-wide)
};

// The elements [s, s + n) of the value words behind `rv`, U loads per lane in flight.  SUM / MIN / MAX choose what is
// computed (scan_clu: its aggregate; clu_build: all three in one pass); `exact` is QParams::exact_sum (plain adds: the
// same `hi` as the compensated form, whose sum is fl(a + b) too, and no `lo`).
template <bool SUM, bool MIN, bool MAX, uint32_t U>
__device__ __forceinline__ CluRed clu_reduce_pinned(__amdgpu_buffer_rsrc_t rv, uint32_t s, uint32_t n, uint32_t lane,
                                                    bool exact) {
  CluRed r;
  r.cnt = 0u;
  r.hi = r.lo = 0.0;
  r.omin = ~0ull;
  r.omax = 0ull;
  bool nan_seen = false;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u * U) {
    v2u x[U];
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t i = i0 + 64u * u + lane;
      x[u] = __builtin_amdgcn_raw_buffer_load_b64(rv, i < n ? (s + i) * 8u : OOB, 0, 0);
    }
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t i = i0 + 64u * u + lane;
      const double v = __longlong_as_double((long long)(((uint64_t)x[u].y << 32) | x[u].x));
      if (i >= n) continue;
      r.cnt += 1u;
      if (SUM) {
        if (exact) {
          r.hi += v;
        } else {
          double sm, e;
          two_sum(r.hi, v, sm, e);
          r.hi = sm;
          r.lo += e;
        }
      }
      if (MIN || MAX) {
        if (MIN && v != v) nan_seen = true;
        const unsigned long long o = dbl_order(v);
        if (MIN) r.omin = o < r.omin ? o : r.omin;
        if (MAX) r.omax = o > r.omax ? o : r.omax;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    r.cnt += __shfl_xor(r.cnt, off, 64);
    if (SUM) {
      const double oh = __shfl_xor(r.hi, off, 64);
      if (exact) {
        r.hi += oh;
      } else {
        const double ol = __shfl_xor(r.lo, off, 64);
        double sm, e;
        two_sum(r.hi, oh, sm, e);
        r.hi = sm;
        r.lo = r.lo + ol + e;
      }
    }
    if (MIN) {
      const unsigned long long o = __shfl_xor(r.omin, off, 64);
      r.omin = o < r.omin ? o : r.omin;
    }
    if (MAX) {
      const unsigned long long o = __shfl_xor(r.omax, off, 64);
      r.omax = o > r.omax ? o : r.omax;
    }
  }
  r.nan = MIN && __ballot(nan_seen) != 0ull;
  return r;
}

}  // namespace lk
