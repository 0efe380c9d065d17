// Exemplar row selection (exemplar.cpp): the host arithmetic between ex_scan HIST passes, free of device and engine
// types so that it also runs against a CPU histogram (lk_ex_select_sim, ex_select_sim.cpp).  Per glob, passes narrow
// the window to a range holding its top `limit` rows: probe_boundaries lists zone-map ranges to try first, next_pass
// says what one pass counts, narrow reads the pass's histogram.  `bins` is the device's XBINS.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace lk {

struct XSel {
  int64_t win_lo = 0, win_hi = 0;
  bool open = false;                      // another HIST pass is needed
  std::vector<int64_t> probes;            // ordered-end-first ranges to try before the whole window (zone maps)
  size_t probe = 0;
  int64_t hlo = 0, hhi = 0;               // range still being narrowed
  uint64_t need = 0, above = 0;           // rows still wanted from [hlo, hhi); rows certainly in beyond it
  int64_t elo = 0, ehi = 0;               // final emit range
  uint64_t count = 0;                     // rows in the emit range
  void start(uint64_t limit) {            // limit == above + need from here on
    hlo = elo = win_lo;
    hhi = ehi = win_hi;
    need = limit;
  }
};

struct XTile {   // a tile's zone map
  int64_t ts_min, ts_max;
  uint64_t nrows;
};

// Ordered end first: segments are written in time order, so the newest (DESC) rows sit in a few tiles.  From the
// zone maps, candidate boundaries covering the last probe_rows, 8 * probe_rows, ... rows of the glob; a HIST pass over
// [boundary, window end) that already counts `limit` passing rows holds the whole top `limit` (every row before
// the boundary is older than all of them); otherwise the next, wider boundary is tried.
inline std::vector<int64_t> probe_boundaries(const std::vector<XTile>& tiles, int64_t win_lo, int64_t win_hi, bool desc,
                                             uint64_t probe_rows) {
  std::vector<std::pair<int64_t, int64_t>> tl;   // (ordered key, other end)
  std::vector<uint64_t> tr;
  for (const XTile& t : tiles) {
    if (t.ts_max < win_lo || t.ts_min >= win_hi) continue;
    tl.emplace_back(desc ? -t.ts_max : t.ts_min, desc ? t.ts_min : t.ts_max);
    tr.push_back(t.nrows);
  }
  std::vector<size_t> ord(tl.size());
  for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return tl[a].first < tl[b].first; });
  std::vector<int64_t> probes;
  uint64_t rows = 0, goal = probe_rows;
  int64_t edge = desc ? INT64_MAX : INT64_MIN;
  for (size_t i : ord) {
    rows += tr[i];
    edge = desc ? std::min(edge, tl[i].second) : std::max(edge, tl[i].second + 1);
    if (rows >= goal) {
      const int64_t b = desc ? std::max(edge, win_lo) : std::min(edge, win_hi);
      if ((desc && b > win_lo) || (!desc && b < win_hi)) probes.push_back(b);
      goal *= 8;
    }
  }
  return probes;
}

// What one HIST pass asks of the device for one glob: rows with rlo <= ts < rhi count in bin
// clamp((ts - hbase) / hwidth, 0, bins - 1); the first nb bins cover the range.  A closed glob asks for nothing.
struct XPass {
  int64_t rlo, rhi, hbase, hwidth;
  uint32_t nb;
};
inline XPass next_pass(XSel& s, bool desc, uint32_t bins) {
  if (s.open && s.probe < s.probes.size()) {   // probing: [boundary, end) (DESC) / [start, boundary) (ASC)
    s.hlo = desc ? s.probes[s.probe] : s.win_lo;
    s.hhi = desc ? s.win_hi : s.probes[s.probe];
  }
  const int64_t span = s.open ? s.hhi - s.hlo : 0;
  const int64_t w = span > 0 ? (span + bins - 1) / bins : 1;
  return XPass{s.open ? s.hlo : 0, s.open ? s.hhi : 0, s.hlo, w, span > 0 ? uint32_t((span + w - 1) / w) : 0u};
}

// Reads the pass's histogram h[0..nb) of bin width w: a failed probe moves to the next boundary (or the whole window);
// otherwise the bins are walked from the ordered end until `need` rows are covered, and the range closes on the split
// bin or narrows to it.  `s` stays open when another pass is needed.
inline void narrow(XSel& s, const uint32_t* h, uint32_t nb, int64_t w, bool desc, uint64_t cand_cap) {
  if (s.probe < s.probes.size()) {
    uint64_t tot = 0;
    for (uint32_t k = 0; k < nb; k++) tot += h[k];
    if (tot < s.need) {   // not enough rows past this boundary: a wider one, or the whole window
      if (++s.probe >= s.probes.size()) {
        s.hlo = s.win_lo;
        s.hhi = s.win_hi;
      }
      return;
    }
    s.probe = s.probes.size();   // the top `limit` lies in the probed range: narrow it as usual
  }
  uint64_t cum = 0;
  int64_t split = -1;
  for (uint32_t k = 0; k < nb; k++) {
    const uint32_t b = desc ? nb - 1 - k : k;
    if (cum + h[b] >= s.need) {
      split = int64_t(b);
      break;
    }
    cum += h[b];
  }
  if (split < 0) {   // fewer rows than wanted: every row of the range
    s.count = s.above + cum;
    if (desc) s.elo = s.hlo;
    else s.ehi = s.hhi;
    s.open = false;
    return;
  }
  const int64_t blo = s.hlo + split * w, bhi = std::min(s.hhi, blo + w);
  // the split bin is taken whole when the rows it adds beyond the `need` still wanted stay under the cap (or it
  // is one millisecond wide: those rows are tied and all listed)
  if (cum + h[split] - s.need <= cand_cap || w == 1) {
    s.count = s.above + cum + h[split];
    if (desc) s.elo = blo;
    else s.ehi = bhi;
    s.open = false;
  } else {
    s.above += cum;
    s.need -= cum;
    s.hlo = blo;
    s.hhi = bhi;
  }
}

// One step of Akka's mergeSorted fold: the left head when it is strictly less under the ordering, else the right head.
template <class T, class Less>
std::vector<T> merge_sorted(std::vector<T>& left, std::vector<T>& right, Less less) {
  std::vector<T> m;
  m.reserve(left.size() + right.size());
  size_t i = 0, j = 0;
  while (i < left.size() && j < right.size()) {
    if (less(left[i], right[j])) m.push_back(std::move(left[i++]));
    else m.push_back(std::move(right[j++]));
  }
  while (i < left.size()) m.push_back(std::move(left[i++]));
  while (j < right.size()) m.push_back(std::move(right[j++]));
  return m;
}

}  // namespace lk
