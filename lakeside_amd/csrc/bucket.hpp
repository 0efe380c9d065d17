// The rule that turns a row's timestamp into a bucket (BaseExpr.scala:159-165 window and `ts - ts % step`, 376-394
// metrics), stated once and pinned on the CPU (tests/test_bucket_cpu.py through bucket_sim.cpp).  Plain C++ with no
// engine header: the kernels inline it, the host hook compiles it as is.  It touches no memory: a caller raises
// FLAG_METRICS_UNALIGNED / FLAG_CELL_RANGE itself from the status it gets back.
// Callers: bucket_mono -- the zone maps, direct-table spans and split tiles of scan_lean and scan_tiles, and the
// non-metrics arm of their row paths; bucket_row -- ex_scan.  scan_tiles' consume and scan_lean's row still write
// bucket_row's steps out (same arithmetic, same order, flags raised in place): through the function the compiler
// allocated their registers differently, and those are the two hottest loops of the engine.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LK_BK_HD __host__ __device__ __attribute__((always_inline))
#else
#define LK_BK_HD
#endif

namespace lk {

// The bucket of `ts`, monotone in ts and unchecked: metrics, the raw timestamp's distance from the base in steps
// (truncating); otherwise `ts - ts % step` (truncating remainder, as the JVM's) from the base in steps.  Zone maps,
// direct-table spans and split tiles bound a tile's buckets with it.
LK_BK_HD inline int64_t bucket_mono(int64_t ts, int64_t step, int64_t base, bool metrics) {
  if (metrics) return (ts - base) / step;
  return ((ts - ts % step) - base) / step;
}

struct BucketRule {        // QParams' bucket fields, by value
  int64_t step, base;
  uint64_t nbuckets;
  double inv_step;         // 1.0 / step
  bool metrics;
  bool fast_div;           // the host guarantees 0 <= ts - base < 2^32 for every row inside a window, and step < 2^31
};

enum BucketStatus : uint32_t {
  BUCKET_IN = 0,           // b is the row's bucket
  BUCKET_OUTSIDE,          // ts outside [win_lo, win_hi): no row (b unspecified)
  BUCKET_UNALIGNED,        // metrics: inside the window but off the step grid
  BUCKET_RANGE             // inside the window, b < 0 or b >= nbuckets
};

struct RowBucket {
  int64_t b;
  BucketStatus st;
};

// One row.  fast_div: the quotient of d = ts - base (< 2^32 inside a window) from the double reciprocal.  double(d) is
// exact and inv_step is within half an ulp of 1 / step, so the product, rounded once more, is within about
// d / step * 2^-52 < 2^-20 of the true quotient before truncation: the truncated q is off by at most one, which the
// remainder's sign or size shows and one step corrects (tests/test_bucket_cpu.py meets the short side, at multiples
// of the step).  The bucket is computed before the window verdict (rows outside get a garbage q that is never used),
// and "unaligned" is reported only for rows inside the window.  Non-metrics, q is the bucket only for ts >= 0, where
// `ts - ts % step` floors; the evaluator's bases are epoch times.
LK_BK_HD inline RowBucket bucket_row(int64_t ts, int64_t win_lo, int64_t win_hi, const BucketRule r) {
  const bool in = ts >= win_lo && ts < win_hi;
  int64_t b = 0;
  bool unaligned = false;
  if (r.fast_div) {
    const uint32_t step32 = uint32_t(r.step);
    const uint32_t d = uint32_t(ts - r.base);
    uint32_t q = uint32_t(double(d) * r.inv_step);
    int64_t rm = int64_t(d) - int64_t(q) * step32;
    q = rm < 0 ? q - 1 : (rm >= int64_t(step32) ? q + 1 : q);
    rm = int64_t(d) - int64_t(q) * step32;
    unaligned = r.metrics && rm != 0;
    b = q;
  } else if (in) {
    if (r.metrics) {
      const int64_t d = ts - r.base;
      b = d / r.step;
      unaligned = d - b * r.step != 0;
    } else {
      b = bucket_mono(ts, r.step, r.base, false);
    }
  }
  if (!in) return RowBucket{b, BUCKET_OUTSIDE};
  if (unaligned) return RowBucket{b, BUCKET_UNALIGNED};
  if (b < 0 || uint64_t(b) >= r.nbuckets) return RowBucket{b, BUCKET_RANGE};
  return RowBucket{b, BUCKET_IN};
}

}  // namespace lk
