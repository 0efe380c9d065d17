// Host-only test hook (include/lakeside_text.h): the clustered copy's tile rule of clu.hpp as scan_clu and the host
// call it.
#include "../../include/lakeside_text.h"
#include "clu.hpp"

extern "C" void lk_clu_sim(const int64_t* ts_min, const int64_t* ts_max, const uint8_t* sorted, size_t n, int64_t win_lo,
                           int64_t win_hi, int64_t step, int64_t base, uint64_t nbuckets, int split_ok, uint8_t* kind,
                           int64_t* b0, uint32_t* nsb) {
  using namespace lk;
  for (size_t i = 0; i < n; i++) {
    const CluClass c = clu_classify(ts_min[i], ts_max[i], win_lo, win_hi, step, base, nbuckets, sorted[i] != 0, split_ok != 0);
    kind[i] = uint8_t(c.kind);
    b0[i] = c.b0;
    nsb[i] = c.nsb;
  }
}

extern "C" uint64_t lk_clu_block_bytes(uint32_t nrows, uint32_t dict_n, uint32_t* agg_off, uint32_t* vals_off,
                                       uint64_t* rows_off) {
  if (agg_off) *agg_off = lk::CLU_AGG_OFF;
  if (vals_off) *vals_off = lk::clu_vals_off(dict_n);
  if (rows_off) *rows_off = lk::clu_rows_off(nrows, dict_n);
  return lk::clu_block_bytes(nrows, dict_n);
}

extern "C" uint32_t lk_clu_sub_bytes(uint32_t nrows, uint32_t dict_n, uint32_t c, uint32_t j, uint32_t* nsub,
                                     uint32_t* sub_rows, uint32_t* sub_max, uint32_t* sagg_off, uint32_t* csub_off,
                                     uint32_t* nan_off) {
  if (nsub) *nsub = lk::clu_nsub(nrows);
  if (sub_rows) *sub_rows = lk::CLU_SUB_ROWS;
  if (sub_max) *sub_max = lk::CLU_SUB_MAX;
  if (sagg_off) *sagg_off = lk::clu_sub_sagg_off(c, j);
  if (csub_off) *csub_off = lk::clu_sub_csub_off(dict_n);
  if (nan_off) *nan_off = lk::clu_sub_nan_off(dict_n);
  return lk::clu_sub_bytes(dict_n);
}

extern "C" uint32_t lk_clu_sub_sim(uint32_t nrows, const uint32_t* sb, uint32_t nsb, uint32_t* cls) {
  using namespace lk;
  const uint32_t n = clu_nsub(nrows);
  for (uint32_t j = 0; j < n; j++) cls[j] = clu_sub_class(j, nrows, sb, nsb);
  return n;
}

extern "C" int lk_clu_samples_sim(const int64_t* ts, uint32_t nrows, int64_t* table) {
  using namespace lk;
  if (nrows == 0 || nrows > TILE_ROWS) return -1;
  for (uint32_t s = 0; s < CLU_SAMP_N; s++) table[s] = ts[clu_samp_row(s, nrows)];
  return int(CLU_SAMP_N);
}

extern "C" uint64_t lk_clu_samp_layout(uint32_t tile, uint32_t* samp_bytes) {
  if (samp_bytes) *samp_bytes = lk::CLU_SAMP_BYTES;
  return lk::clu_samp_tile_off(tile);
}

extern "C" int lk_clu_count_sim(uint32_t nrows, const uint16_t* rows, uint32_t n, const uint32_t* sb, uint32_t nsb,
                                int use_sub, uint32_t* cnt) {
  using namespace lk;
  if (nrows == 0 || nrows > TILE_ROWS || n > nrows || nsb > CLU_SPLIT_MAX) return -1;
  for (uint32_t i = 0; i < n; i++)
    if (rows[i] >= nrows || (i && rows[i] <= rows[i - 1])) return -1;
  // the code's elements lie at [s, s + n) of the tile, other codes' before and after; csub as clu_build writes it
  const uint32_t s = (nrows - n) / 2u, e = s + n;
  uint32_t csub[CLU_SUB_MAX + 1u];
  uint32_t i = 0;
  for (uint32_t j = 0; j <= CLU_SUB_MAX; j++) {
    while (i < n && uint32_t(rows[i]) < CLU_SUB_ROWS * j) i++;
    csub[j] = s + i;   // past the tile's sub-blocks: e
  }
  for (uint32_t k = 0; k <= CLU_SPLIT_MAX; k++) cnt[k] = 0u;
  clu_count_split(rows, s, e, csub, nrows, sb, nsb, use_sub != 0, cnt);
  return int(CLU_SPLIT_MAX + 1u);
}

extern "C" int lk_clu_segment_taken(int all_copies_sorted, int64_t widest, int64_t step) {
  return lk::clu_segment_taken(all_copies_sorted != 0, widest, step) ? 1 : 0;
}
