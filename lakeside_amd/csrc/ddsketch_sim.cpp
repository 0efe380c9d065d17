// Host-only test hook (include/lakeside_text.h): the host DDSketch of ddsketch.cpp as the evaluator drives it.
#include <cstring>

#include "../../include/lakeside_text.h"
#include "ddsketch.hpp"
#include "layout.hpp"

namespace {
// accept over vals[0..n) then add_bin over the n_bins pairs; false when a value was rejected (*rejected = its position,
// nothing after it is fed) or a bin id lies outside the kernels' key space
bool fill(lk::dd::Sketch& s, const double* vals, size_t n, const uint32_t* bins, const double* counts, size_t n_bins,
          size_t base, long* rejected, bool* bad_bin) {
  for (size_t i = 0; i < n; i++)
    if (!s.accept(vals[i])) {
      *rejected = long(base + i);
      return false;
    }
  for (size_t i = 0; i < n_bins; i++) {
    if (bins[i] >= lk::DD_NBINS) {
      *bad_bin = true;
      return false;
    }
    s.add_bin(bins[i], counts[i]);
  }
  return true;
}
}  // namespace

extern "C" long lk_dd_sim(const double* vals, size_t n, const uint32_t* bins, const double* counts, size_t n_bins,
                          const double* mvals, size_t mn, const uint32_t* mbins, const double* mcounts, size_t mn_bins,
                          const double* qs, size_t nq, double* quantiles, long* rejected, double* consts,
                          double* total, uint8_t* out, size_t cap) {
  using namespace lk;
  const dd::Mapping& m = dd::mapping();
  if (consts) {
    const double c[8] = {m.gamma, m.multiplier, m.relative_accuracy, m.min_indexable, m.max_indexable,
                         double(DD_BIAS), double(DD_HALF), double(DD_NBINS)};
    memcpy(consts, c, sizeof c);
  }
  dd::Sketch a, b;
  bool bad_bin = false;
  *rejected = -1;
  if (fill(a, vals, n, bins, counts, n_bins, 0, rejected, &bad_bin) &&
      fill(b, mvals, mn, mbins, mcounts, mn_bins, n, rejected, &bad_bin))
    a.merge(b);
  if (bad_bin) return -1;
  for (size_t i = 0; i < nq; i++) quantiles[i] = a.quantile(qs[i]);
  if (total) *total = a.count();
  const std::string s = a.serialize();
  if (s.size() > cap) return -5;
  memcpy(out, s.data(), s.size());
  return long(s.size());
}
