// Host-only test hook (include/lakeside_text.h): the exemplar row selection of ex_select.hpp, driven as
// exemplar.cpp's select() drives it, with a CPU histogram in place of the ex_scan HIST launch.
#include <vector>

#include "../../include/lakeside_text.h"
#include "ex_select.hpp"
#include "kernels.hpp"   // XBINS

extern "C" int lk_ex_select_sim(const int64_t* ts, size_t n, int64_t win_lo, int64_t win_hi, const int64_t* tiles,
                                size_t ntiles, uint64_t limit, int desc, uint64_t cand_cap, uint64_t probe_rows,
                                int64_t* elo, int64_t* ehi, uint64_t* count, int* passes) {
  using namespace lk;
  XSel s;
  s.win_lo = win_lo;
  s.win_hi = win_hi;
  s.start(limit);
  s.open = limit != 0 && win_lo < win_hi;   // the evaluator opens no other glob
  *passes = 0;
  if (s.open) {
    std::vector<XTile> zt(ntiles);
    for (size_t i = 0; i < ntiles; i++) zt[i] = XTile{tiles[3 * i], tiles[3 * i + 1], uint64_t(tiles[3 * i + 2])};
    s.probes = probe_boundaries(zt, win_lo, win_hi, desc != 0, probe_rows);
  }
  std::vector<uint32_t> hist(XBINS);
  while (s.open) {
    const XPass p = next_pass(s, desc != 0, XBINS);
    std::fill(hist.begin(), hist.end(), 0u);
    for (size_t i = 0; i < n; i++) {   // ex_scan HIST (ex_kernels.hip): the range test, then the clamped bin
      if (ts[i] < p.rlo || ts[i] >= p.rhi) continue;
      int64_t b = (ts[i] - p.hbase) / p.hwidth;
      b = b < 0 ? 0 : (b >= int64_t(XBINS) ? int64_t(XBINS) - 1 : b);
      hist[size_t(b)]++;
    }
    ++*passes;
    narrow(s, hist.data(), p.nb, p.hwidth, desc != 0, cand_cap);
  }
  // a glob that was never opened emits nothing: the empty range at the ordered end
  *elo = limit == 0 && desc ? s.ehi : s.elo;
  *ehi = limit == 0 && !desc ? s.elo : s.ehi;
  *count = s.count;
  return 0;
}
