// Host-only test hook (include/lakeside_text.h): the row -> bucket rule of bucket.hpp as the kernels call it.
#include "../../include/lakeside_text.h"
#include "bucket.hpp"

extern "C" void lk_bucket_sim(const int64_t* ts, size_t n, int64_t win_lo, int64_t win_hi, int64_t step, int64_t base,
                              uint64_t nbuckets, int metrics, int fast_div, int64_t* bucket, uint8_t* status,
                              int64_t* mono) {
  using namespace lk;
  const BucketRule r{step, base, nbuckets, 1.0 / double(step), metrics != 0, fast_div != 0};   // inv_step: eval.cpp
  for (size_t i = 0; i < n; i++) {
    const RowBucket rb = bucket_row(ts[i], win_lo, win_hi, r);
    bucket[i] = rb.b;
    status[i] = uint8_t(rb.st);
    mono[i] = bucket_mono(ts[i], step, base, metrics != 0);
  }
}
