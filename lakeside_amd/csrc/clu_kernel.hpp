// scan_clu<AGG> (SUM, MIN, MAX, COUNT; dense tables): the name-filter scan over the name-clustered value copy
// (layout.hpp, CluTile; built at load by clu_build, clu_kernels.hip).  Included by the scan_<agg>_clu_d.hip units
// through scan_inst.hpp.  The host (eval_plan.cpp, plan_cluster) hands it the segments whose every tile clu_tile takes,
// so neither scan_lean nor scan_tiles runs over them.  An AVG chart arrives as AGG_SUM with the table's `rows` plane
// kept (setup_scan: LEAN_NO_CNT without LEAN_SUM_EXISTS): global_merge adds the element counts the SUM paths pass.
//
// COUNT reads no value at all (its code is guarded with `if constexpr`; the other instantiations compile to what they
// were): a pinned tile's count of code c is cpref[c + 1] - cpref[c], whatever LK_NO_CLU_AGG says; of a split tile, a
// whole sub-block's is csub[c][j + 1] - csub[c][j] and only a straddling sub-block's crows (2 B per element) are
// streamed and classed -- clu.hpp's clu_count_split, mirrored line for line.  No cvals, cagg, sagg or NaN mask.
//
// Per tile: the passing-code mask exactly as scan_lean computes it (remap -> strtab -> T / F bits -> truth word,
// leaf_false included).  A pinned tile's elements all land in one bucket, and what its passing codes contribute --
// each code's (hi, lo, count) or extreme -- was fixed when the segment was loaded: lane c merges the tile's stored
// aggregate cagg[c] (built by clu_build with clu_reduce_pinned, clu_reduce.hpp) through global_merge itself and the
// tile moves no value.  A split tile streams, for each passing code c, the contiguous range cvals[cpref[c] ..
// cpref[c + 1]) with coalesced 8-B loads and crows (the element's row within the tile), and takes each element's class
// from its row index against boundary rows found with scan_lean's two-round timestamp search (256 samples, then the
// sample gap holding each boundary): the wave reduces per (code, class) and lane 0 merges once per (tile, code, class).
// Of a split tile only the 4,096-row sub-blocks that hold a boundary row are streamed (clu.hpp, clu_sub_class: at most
// three): a sub-block that holds none lies in one class whatever the query, and what its passing codes contribute was
// stored at load in the segment's sub-block area (csub / sagg, clu.hpp): lane j loads code c's csub[c][j], csub[c][j + 1]
// and sagg[c][j] in one round and starts its per-class accumulators with them; the streamed elements are added on top,
// then the one shuffle tree and the one merge per (tile, code, class).  LK_NO_CLU_SUB=1 (SPLIT_OK_NO_CLU_SUB), or a
// segment without the area, streams the ranges whole: bit for bit the same MIN, MAX and integral sums, real sums within
// the suite's bar (the double-double partials combine in another order).
// The search's first round does not wait behind the filter chain: the 256 sampled timestamps lie in the tile's sample
// table in front of the sub-block area (clu.hpp; copied at load by clu_samp_build), 16 consecutive lines that the
// wave loads in four coalesced rounds as soon as CluTile has arrived and classes behind the truth word's ballot; the
// first passing code's csub / sagg entries are issued before the search as well, so they share its round trips.  The
// gap round reads the timestamp column itself.  LK_NO_CLU_SAMP=1 (SPLIT_OK_NO_CLU_SAMP), or a segment without the table
// (cluster_samples off), samples the column as before -- 256 lines 2 KB apart in a full tile: the same timestamps, so
// the same boundaries and rows bit for bit.  QSeg's fields of the area are read with its other fields at the top.
// No run staging, no chunk table, no row list, no LDS.  global_merge honours the LEAN_* flags, the -0.0 empty marker,
// exact_sum and FLAG_MIN_NAN.  LK_NO_CLU_AGG=1 (SPLIT_OK_NO_CLU_AGG) streams pinned tiles too, with clu_reduce_pinned
// (one merge per (tile, code)): the same rows bit for bit, the A/B and the tests' proof of which path ran.
//
// Shape: one wave per tile, four tiles per 256-thread workgroup, no barrier.  A pinned tile is a chain of dependent
// loads (QSeg -> TileDesc / CluTile / TileCol -> remap, cpref, cagg -> strtab -> truth word) and a few atomics; at a
// 1 m step three of C2's four tiles are pinned.  A split tile adds the boundary search (the sample table beside the
// chain above, then the gap rows) and its codes' sub-block entries and straddlers.  A split tile of C2 has about 4,096 passing values (32 KB): a wave
// holds 8 loads per lane of values and of rows in flight; the stream is latency-bound, so what counts is bytes in flight
// per CU, and a wave per tile needs no cross-wave reduction.  Measured: C2's scan 0.159 -> 0.101 ms in the
// kernel trace with the aggregates (1.114 ms before the copy), plan bytes 0.585 -> 0.165 GB.  A workgroup per tile and
// several tiles per wave were not measured (DESIGN §9 lists the comparison as open).
#pragma once
#include <type_traits>

#include "clu.hpp"
#include "clu_reduce.hpp"
#include "device_common.hpp"

namespace lk {

constexpr int CLU_WAVES = BLOCK / 64;   // tiles per workgroup
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

template <int AGG>
__global__ __launch_bounds__(BLOCK) void scan_clu(QParams P) {
  static_assert(AGG == AGG_SUM || AGG == AGG_MIN || AGG == AGG_MAX || AGG == AGG_COUNT, "scan_clu: SUM, MIN, MAX, COUNT");
  const uint32_t lane = threadIdx.x & 63u;
  const QSeg* Sp = P.segs + blockIdx.y;
  const uint32_t t = uni(blockIdx.x * uint32_t(CLU_WAVES) + (threadIdx.x >> 6));
  if (t >= Sp->ntiles) return;
  const TileDesc* tdp = Sp->tiles + t;
  const CluClass cc = clu_tile(P, Sp, t);
  if (cc.kind == CLU_NONE) return;   // zone map: outside the glob window
  if (cc.kind == CLU_UNTAKEN) {      // the host hands over only segments whose tiles are all taken (clu_segment_taken)
    if (lane == 0) atomicOr(P.flags, FLAG_CELL_RANGE);
    return;
  }
  // QSeg's fields of the sub-block area, read here with its other fields: a read behind the tests that need it is one
  // more dependent round trip of the tile's chain
  const uint8_t* const sub_base = uni_ptr(Sp->clu_sub);
  const uint32_t sub_stride = uni(Sp->clu_sub_stride), samp_back = uni(Sp->clu_samp_back);
  const CluTile d = Sp->clu[t];
  const TileCol* tc0 = Sp->cols[0].tcols + t;
  const TileCol* tc2 = Sp->cols[2].tcols + t;
  const uint32_t nrows = d.nrows < tdp->nrows ? d.nrows : tdp->nrows;
  const uint32_t dict_n = tc2->dict_n < 64u ? tc2->dict_n : 64u;
  const bool count_plan = P.plan_bytes != nullptr;
  uint64_t pbytes = 0;
  const uint8_t* blk = Sp->clu_base + d.off;
  // a pinned tile merges the copy's per-code aggregates (LK_NO_CLU_AGG=1: it streams the ranges, as a split tile must;
  // COUNT has nothing to stream: a pinned tile's counts are cpref's differences whatever the switch says)
  const bool use_agg = AGG != AGG_COUNT && cc.kind == CLU_PINNED && !(P.split_ok & SPLIT_OK_NO_CLU_AGG) && d.nrows <= tdp->nrows;   // uniform

  // lane c: the code's range [cs, ce) of cvals / crows and, for a pinned tile, its aggregate.  Loaded for every code
  // beside the remap entry, before the truth word says which codes pass: the three depend on CluTile / TileCol alone,
  // so the tile's chain of dependent round trips is no longer for them.
  uint32_t cs, ce;
  CluAgg ag = CluAgg{0.0, 0.0, 0ull, 0ull};
  unsigned long long nanw = 0ull;
  {
    const uint32_t* cp = reinterpret_cast<const uint32_t*>(blk);
    cs = cp[lane];
    ce = cp[lane + 1u];
    if (use_agg) {
      if (lane < clu_dict_n(d.dict_n)) ag = reinterpret_cast<const CluAgg*>(blk + CLU_AGG_OFF)[lane];
      if (AGG == AGG_MIN) nanw = *reinterpret_cast<const unsigned long long*>(blk + CLU_NAN_OFF);
    }
  }
  // A split tile's 256 timestamp samples (the first round of the boundary search below) from the tile's sample table
  // (clu.hpp; QSeg::clu_samp_back bytes below the sub-block area): lane l holds samples l, l + 64, l + 128, l + 192 -- four coalesced loads, 16 lines.  They
  // depend on CluTile alone and are issued here, beside the filter chain, and consumed behind the truth word's ballot.
  // LK_NO_CLU_SAMP=1 (SPLIT_OK_NO_CLU_SAMP), or a segment without the table: the search samples the timestamp column.
  const bool use_samp = cc.kind == CLU_SPLIT && sub_base != nullptr && !(P.split_ok & SPLIT_OK_NO_CLU_SAMP) &&
                        d.nrows <= tdp->nrows && clu_samp_tile_off(t) + CLU_SAMP_BYTES <= samp_back;   // uniform
  v2u tsamp[CLU_SAMP_N / 64u];
#pragma unroll
  for (uint32_t j = 0; j < CLU_SAMP_N / 64u; j++) tsamp[j] = v2u{0u, 0u};
  if (use_samp) {
    const __amdgpu_buffer_rsrc_t rsm =
        make_rsrc(sub_base - samp_back + clu_samp_tile_off(t), CLU_SAMP_BYTES);
#pragma unroll
    for (uint32_t j = 0; j < CLU_SAMP_N / 64u; j++)
      tsamp[j] = __builtin_amdgcn_raw_buffer_load_b64(rsm, (lane + 64u * j) * 8u, 0, 0);
  }

  // passing codes: one ballot over the chunk dictionary (Kleene: the leaves' T/F bits of the code), as scan_lean
  uint32_t lut = 0;
  bool pass = false;
  if (lane < dict_n) {
    const uint32_t g = (Sp->cols[2].remap + tc2->remap)[lane];
    const uint32_t* tab = P.strp[0].strtab;
    lut = tab ? tab[g] : g;
    const uint32_t lf = Sp->leaf_false;
    const uint32_t bits = (lut >> 24) << P.strp[0].lbase;
    const uint32_t lmask = P.strp[0].lmask;
    const uint32_t T = bits & lmask & ~lf, F = (~bits & lmask) | lf;
    const uint32_t ix = T | (F << P.nleaves);
    pass = (P.truth[ix >> 5] >> (ix & 31)) & 1u;
  }
  unsigned long long emask = __ballot(pass);
  if (count_plan && lane == 0) {
    atomicAdd(P.flags + 1, 1u);   // clustered_tiles
    pbytes += sizeof(TileDesc) + sizeof(CluTile) + sizeof(TileCol) + uint64_t(dict_n) * 8u +
              uint64_t((((1u << (2 * P.nleaves)) + 31) / 32) * 4u);
  }
  if (!emask) {   // no row of the tile passes
    if (pbytes) atomicAdd(P.plan_bytes, (unsigned long long)pbytes);
    return;
  }

  ce = ce < nrows ? ce : nrows;
  cs = cs < ce ? cs : ce;
  if (count_plan && lane == 0) pbytes += uint64_t(dict_n + 1u) * 4u;
  const uint32_t stride = P.strp[0].dim_stride;
  const unsigned long long glob_base = (unsigned long long)Sp->glob_slot * P.nbuckets;

  if constexpr (AGG == AGG_COUNT) {
    if (cc.kind == CLU_PINNED) {   // uniform: lane c's count is its code's clamped range, no further line is read
      if (pass && cs < ce) {
        const unsigned long long cell = (glob_base + (unsigned long long)cc.b0) * P.ngroups + (lut & DIM_MASK) * stride;
        global_merge<AGG_COUNT, false>(P, cell, ce - cs, ce - cs, 0.0, 0.0, 0ull);
      }
      if (pbytes) atomicAdd(P.plan_bytes, (unsigned long long)pbytes);
      return;
    }
  }
  if (use_agg) {   // uniform: every passing lane merges its own code (codes sharing a dim meet in the atomics)
    if (pass && cs < ce) {
      const unsigned long long cell = (glob_base + (unsigned long long)cc.b0) * P.ngroups + (lut & DIM_MASK) * stride;
      global_merge<AGG, false>(P, cell, ce - cs, ce - cs, ag.hi, ag.lo, AGG == AGG_MIN ? ag.omin : ag.omax);
    }
    if (AGG == AGG_MIN && (nanw & emask) && lane == 0) atomicOr(P.flags, FLAG_MIN_NAN);
    const unsigned long long mmask = count_plan ? __ballot(pass && cs < ce) : 0ull;
    if (count_plan && lane == 0) {   // the 128-B lines of the merged entries (the NaN mask lies in cpref's)
      unsigned long long lines = 0ull;
      for (unsigned long long m = mmask; m; m &= m - 1ull)
        lines |= 1ull << ((CLU_AGG_OFF + uint32_t(__builtin_ctzll(m)) * uint32_t(sizeof(CluAgg))) >> 7);
      pbytes += 128u * uint64_t(__popcll(lines));
      atomicAdd(P.plan_bytes, (unsigned long long)pbytes);
    }
    return;
  }
  const __amdgpu_buffer_rsrc_t rv = make_rsrc(blk + clu_vals_off(d.dict_n), nrows * 8u);
  const uint16_t* crows = reinterpret_cast<const uint16_t*>(blk + clu_rows_off(nrows, d.dict_n));

  const bool split = cc.kind == CLU_SPLIT;
  const uint32_t nsb = cc.nsb;
  // A split tile's sub-block area (clu.hpp): the whole sub-blocks of a passing code hand on their stored aggregates
  // (COUNT: their element counts), only the straddling ones are streamed.  LK_NO_CLU_SUB=1, or a segment without the
  // area: the range streams whole.
  const bool use_sub = split && sub_base != nullptr && !(P.split_ok & SPLIT_OK_NO_CLU_SUB) && d.nrows <= tdp->nrows &&
                       clu_sub_bytes(d.dict_n) <= sub_stride && dict_n <= clu_dict_n(d.dict_n);   // uniform
  const __amdgpu_buffer_rsrc_t rsub =
      make_rsrc(use_sub ? sub_base + uint64_t(t) * sub_stride : nullptr, use_sub ? clu_sub_bytes(d.dict_n) : 0u);
  const uint32_t nsub = clu_nsub(nrows);
  // lane j: code c's elements [a, b) of sub-block j (csub) and, but for COUNT, their aggregate (sagg: SUM hi, lo; MIN /
  // MAX the extreme; MIN also the code's NaN bits, a uint16 inside an aligned word), one round of loads through the
  // area's buffer resource (uniform base and entry offset, the lane's offset in one register).  They depend on c alone:
  // the first passing code's are issued before the boundary search below, whose round trips they then share.
  struct SubEnt {
    uint32_t a, b;
    v2u g0, g1;
    uint32_t snan;
  };
  auto load_sub = [&](uint32_t c) __attribute__((always_inline)) -> SubEnt {
    SubEnt en{0u, 0u, v2u{0u, 0u}, v2u{0u, 0u}, 0u};
    const bool sl = lane < nsub;
    const uint32_t co = clu_sub_csub_off(d.dict_n) + c * (CLU_SUB_MAX + 1u) * 4u;
    en.a = __builtin_amdgcn_raw_buffer_load_b32(rsub, sl ? lane * 4u : OOB, int(co), 0);
    en.b = __builtin_amdgcn_raw_buffer_load_b32(rsub, sl ? lane * 4u + 4u : OOB, int(co), 0);
    if (AGG != AGG_COUNT) {
      const uint32_t go = sl ? lane * uint32_t(sizeof(CluAgg)) : OOB;
      if (AGG == AGG_SUM) {
        const v4u g = __builtin_amdgcn_raw_buffer_load_b128(rsub, go, int(clu_sub_sagg_off(c, 0u)), 0);
        en.g0 = v2u{g.x, g.y};
        en.g1 = v2u{g.z, g.w};
      } else {
        en.g0 = __builtin_amdgcn_raw_buffer_load_b64(rsub, go, int(clu_sub_sagg_off(c, 0u) + (AGG == AGG_MIN ? 16u : 24u)), 0);
      }
      if (AGG == AGG_MIN) {
        const uint32_t no = clu_sub_nan_off(d.dict_n) + c * 2u;
        en.snan = (__builtin_amdgcn_raw_buffer_load_b32(rsub, 0u, int(no & ~3u), 0) >> ((no & 2u) * 8u)) & 0xffffu;
      }
    }
    return en;
  };
  SubEnt pre{0u, 0u, v2u{0u, 0u}, v2u{0u, 0u}, 0u};
  if (use_sub) pre = load_sub(uint32_t(__builtin_ctzll(emask)));   // uniform (emask != 0 here)

  // split tiles: boundary rows (scan_lean's search, per wave: four samples / gap rows per lane)
  uint32_t sb[CLU_SPLIT_MAX];
#pragma unroll
  for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++) sb[k] = 0xffffffffu;
  if (split) {   // uniform
    const int64_t win_lo = Sp->win_lo, win_hi = Sp->win_hi;
    const __amdgpu_buffer_rsrc_t rst = make_rsrc(Sp->base + tc0->vals, tc0->vals_len);
    const uint32_t vbt = tc0->vbase;
    auto cls_of = [&](int64_t ts) __attribute__((always_inline)) -> uint32_t {
      if (ts < win_lo) return 0u;
      if (ts >= win_hi) return nsb;
      return uint32_t(bucket_mono(ts, P.step, P.bucket_base, false) - cc.b0) + 1u;
    };
    auto sample = [&](uint32_t s) __attribute__((always_inline)) -> uint32_t {   // row of sample s (s = 256: nrows)
      return clu_samp_row(s, nrows);
    };
    auto ts_at = [&](uint32_t r, bool live) __attribute__((always_inline)) -> int64_t {
      const v2u x = __builtin_amdgcn_raw_buffer_load_b64(rst, live ? (vbt + r) * 8u : OOB, 0, 0);
      return int64_t(((uint64_t)x.y << 32) | x.x);
    };
    uint32_t scnt[CLU_SPLIT_MAX];   // per class boundary k: the samples below class k + 1 (uniform)
#pragma unroll
    for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++) scnt[k] = 0u;
    // the samples: the table's entries loaded above, or the column's rows they were copied from (the same timestamps)
    int64_t tss[CLU_SAMP_N / 64u];
    uint32_t samp_lines = CLU_SAMP_BYTES / 128u;   // plan bytes: the 128-B lines the samples touch
    if (use_samp) {   // uniform
#pragma unroll
      for (uint32_t j = 0; j < CLU_SAMP_N / 64u; j++) tss[j] = int64_t(((uint64_t)tsamp[j].y << 32) | tsamp[j].x);
    } else {
#pragma unroll
      for (uint32_t j = 0; j < CLU_SAMP_N / 64u; j++) tss[j] = ts_at(sample(lane + 64u * j), true);
      if (count_plan) {   // a line per sample whose line is not the sample's before (rows ascend)
        const uint32_t a0 = uint32_t(reinterpret_cast<uint64_t>(Sp->base + tc0->vals));
        samp_lines = 0u;
#pragma unroll
        for (uint32_t j = 0; j < CLU_SAMP_N / 64u; j++) {
          const uint32_t s = lane + 64u * j;
          const uint32_t ln = (a0 + (vbt + sample(s)) * 8u) >> 7, lp = (a0 + (vbt + sample(s ? s - 1u : 0u)) * 8u) >> 7;
          samp_lines += uint32_t(__popcll(__ballot(s == 0u || ln != lp)));
        }
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < CLU_SAMP_N / 64u; j++) {
      const uint32_t c = cls_of(tss[j]);
#pragma unroll
      for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++)
        if (k < nsb) scnt[k] += uint32_t(__popcll(__ballot(c < k + 1u)));
    }
    // boundary k + 1 lies in the sample gap (sample(n - 1), sample(n)] (n samples below it; none: row 0)
#pragma unroll
    for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++) {
      if (k >= nsb) continue;
      const uint32_t n = scnt[k];
      uint32_t b = 0u;
      if (n != 0u) {   // uniform
        const uint32_t lo = sample(n - 1u) + 1u, hi = sample(n);
        b = hi;   // the first sample at or above the class (n = 256: nrows, no such row)
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
          const uint32_t r = lo + lane + 64u * j;
          const bool live = r < hi;
          const bool f = cls_of(ts_at(r, live)) >= k + 1u && live;
          const unsigned long long bl = __ballot(f);
          if (bl) {
            const uint32_t first = lo + 64u * j + uint32_t(__builtin_ctzll(bl));
            b = first < b ? first : b;
          }
        }
      }
      sb[k] = b;
    }
    if (count_plan && lane == 0) pbytes += sizeof(TileCol) + 128u * (samp_lines + nsb * 2u);   // sample lines, gap lines (approx.)
  }
  auto split_class = [&](uint32_t r) __attribute__((always_inline)) -> uint32_t {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < CLU_SPLIT_MAX; k++) c += r >= sb[k] ? 1u : 0u;
    return c;
  };

  // COUNT of a split tile (pinned ones ended above): clu_count_split (clu.hpp) mirrored line for line -- lane j is its
  // sub-block iteration j, its element loops are spread over the wave -- with the shared clu_sub_class, clu_sub_clamp
  // and clu_split_class.  No value, aggregate or NaN bit is read: with the area, lane j loads the code's csub[c][j] and
  // csub[c][j + 1], a whole sub-block of an in-window class adds b - a, and only the straddling sub-blocks' crows are
  // streamed; without it (LK_NO_CLU_SUB=1, or no area) the code's whole crows range is.  crows: one 2-B load per lane
  // per step, eight steps in flight, as the SUM path loads them.  Counts are exact uint32 (a tile has <= 65,536 rows).
  if constexpr (AGG == AGG_COUNT) {
    uint32_t subc = CLU_SUB_STRADDLE;
    if (use_sub && lane < nsub) subc = clu_sub_class(lane, nrows, sb, nsb);
    constexpr uint32_t NK = CLU_SPLIT_MAX - 1u;   // the in-window classes 1 .. nsb - 1
    bool first = true;
    while (emask) {
      const uint32_t c = uint32_t(__builtin_ctzll(emask));
      emask &= emask - 1ull;
      SubEnt en = pre;   // the first passing code's entries were loaded before the search
      if (use_sub && !first) en = load_sub(c);   // uniform
      first = false;
      const uint32_t s = uni(__shfl(cs, int(c), 64)), e = uni(__shfl(ce, int(c), 64));
      if (s >= e) continue;   // the name is absent from the tile
      const uint32_t dim = (uni(__shfl(lut, int(c), 64)) & DIM_MASK) * stride;
      uint32_t cnt[NK];
#pragma unroll
      for (uint32_t k = 0; k < NK; k++) cnt[k] = 0u;
      // the elements [s0, s0 + n) of crows into the counters (s <= s0, s0 + n <= e <= nrows: inside the tile's crows)
      auto count_rows = [&](uint32_t s0, uint32_t n) __attribute__((always_inline)) {
        constexpr uint32_t U = 8u;
        for (uint32_t i0 = 0; i0 < n; i0 += 64u * U) {
          uint32_t r[U];
#pragma unroll
          for (uint32_t u = 0; u < U; u++) {
            const uint32_t i = i0 + 64u * u + lane;
            r[u] = i < n ? uint32_t(crows[s0 + i]) : 0u;
          }
#pragma unroll
          for (uint32_t u = 0; u < U; u++) {
            const bool live = i0 + 64u * u + lane < n;
            const uint32_t cl = clu_split_class(r[u], sb);
#pragma unroll
            for (uint32_t k = 0; k < NK; k++) cnt[k] += live && cl == k + 1u && k + 1u < nsb ? 1u : 0u;
          }
        }
        if (count_plan && lane == 0)   // the 128-B lines of the streamed row indices
          pbytes += 128u * uint64_t((((s0 + n) * 2u + 127u) >> 7) - ((s0 * 2u) >> 7));
      };
      if (!use_sub) {   // uniform
        count_rows(s, e - s);
      } else {
        const bool sl = lane < nsub;
        const uint32_t co = clu_sub_csub_off(d.dict_n) + c * (CLU_SUB_MAX + 1u) * 4u;
        uint32_t a = en.a, b = en.b;
        if (!sl) a = b = e;
        clu_sub_clamp(a, b, s, e);
        if (subc != CLU_SUB_STRADDLE && subc >= 1u && subc < nsb && a < b) {
#pragma unroll
          for (uint32_t k = 0; k < NK; k++)
            if (subc == k + 1u) cnt[k] = b - a;
        }
        // at most CLU_SPLIT_MAX - 1 sub-blocks hold a boundary inside the tile
        unsigned long long strad = __ballot(sl && subc == CLU_SUB_STRADDLE && a < b);
        while (strad) {   // uniform
          const int j = __builtin_ctzll(strad);
          strad &= strad - 1ull;
          const uint32_t qa = uni(__shfl(a, j, 64)), qb = uni(__shfl(b, j, 64));
          count_rows(qa, qb - qa);
        }
        if (count_plan && lane == 0)   // the 128-B lines of the csub entries read
          pbytes += 128u * uint64_t(((co + (nsub + 1u) * 4u + 127u) >> 7) - (co >> 7));
      }
#pragma unroll
      for (uint32_t k = 0; k < NK; k++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt[k] += __shfl_xor(cnt[k], off, 64);
        if (lane == 0 && cnt[k]) {
          const unsigned long long cell = (glob_base + (unsigned long long)(cc.b0 + int64_t(k))) * P.ngroups + dim;
          global_merge<AGG_COUNT, false>(P, cell, cnt[k], cnt[k], 0.0, 0.0, 0ull);
        }
      }
    }
    if (pbytes) atomicAdd(P.plan_bytes, (unsigned long long)pbytes);
    return;
  }

  bool nan_seen = false;

  // One loop over the passing codes per kind of tile, so that neither path's registers are live across the other's.
  // Pinned, streamed (LK_NO_CLU_AGG): the reduction the copy's aggregates were built with.
  while (!split && emask) {
    const uint32_t c = uint32_t(__builtin_ctzll(emask));
    emask &= emask - 1ull;
    const uint32_t s = uni(__shfl(cs, int(c), 64)), e = uni(__shfl(ce, int(c), 64));
    if (s >= e) continue;   // the name is absent from the tile
    const uint32_t dim = (uni(__shfl(lut, int(c), 64)) & DIM_MASK) * stride;
    const CluRed r = clu_reduce_pinned<AGG == AGG_SUM, AGG == AGG_MIN, AGG == AGG_MAX, 16u>(rv, s, e - s, lane, P.exact_sum != 0u);
    nan_seen = nan_seen || r.nan;
    if (lane == 0 && r.cnt) {
      const unsigned long long cell = (glob_base + (unsigned long long)cc.b0) * P.ngroups + dim;
      global_merge<AGG, false>(P, cell, r.cnt, r.cnt, r.hi, r.lo, AGG == AGG_MIN ? r.omin : r.omax);
    }
    if (count_plan && lane == 0) pbytes += 128u * uint64_t(((e * 8u + 127u) >> 7) - ((s * 8u) >> 7));
  }
  if (!split) {   // uniform
    if (AGG == AGG_MIN && __ballot(nan_seen) && lane == 0) atomicOr(P.flags, FLAG_MIN_NAN);
    if (pbytes) atomicAdd(P.plan_bytes, (unsigned long long)pbytes);
    return;
  }

  // lane j: sub-block j's class, CLU_SUB_STRADDLE when its rows' classes differ (the same for every code)
  uint32_t subc = CLU_SUB_STRADDLE;
  if (use_sub && lane < nsub) subc = clu_sub_class(lane, nrows, sb, nsb);

  // One passing code of a split tile: NK classes (the in-window classes 1 .. nsb - 1, at most CLU_SPLIT_MAX - 1) in
  // per-lane accumulators that the sub-blocks' aggregates and the streamed ranges share, reduced and merged once.
  constexpr uint32_t NK = CLU_SPLIT_MAX - 1u;
  double hi[NK], lo[NK];
  unsigned long long ext[NK];
  uint32_t cnt[NK];
  // the range [s, s + n) of cvals / crows into the accumulators, U loads per lane in flight
  auto stream = [&](auto uc, uint32_t s, uint32_t n) __attribute__((always_inline)) {
    constexpr uint32_t U = decltype(uc)::value;
    for (uint32_t i0 = 0; i0 < n; i0 += 64u * U) {
      v2u x[U];
      uint32_t r[U];
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        const uint32_t i = i0 + 64u * u + lane;
        x[u] = __builtin_amdgcn_raw_buffer_load_b64(rv, i < n ? (s + i) * 8u : OOB, 0, 0);
        r[u] = i < n ? uint32_t(crows[s + i]) : 0u;
      }
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        const uint32_t i = i0 + 64u * u + lane;
        const double v = __longlong_as_double((long long)(((uint64_t)x[u].y << 32) | x[u].x));
        const uint32_t c = split_class(r[u]);
        const bool live = i < n;
#pragma unroll
        for (uint32_t k = 0; k < NK; k++) {
          if (!live || c != k + 1u || k + 1u >= nsb) continue;
          cnt[k] += 1u;
          if (AGG == AGG_SUM) {
            if (P.exact_sum) {
              hi[k] += v;
            } else {
              double sm, e;
              two_sum(hi[k], v, sm, e);
              hi[k] = sm;
              lo[k] += e;
            }
          } else {
            if (AGG == AGG_MIN && v != v) nan_seen = true;
            const unsigned long long o = dbl_order(v);
            ext[k] = AGG == AGG_MIN ? (o < ext[k] ? o : ext[k]) : (o > ext[k] ? o : ext[k]);
          }
        }
      }
    }
    if (count_plan && lane == 0)   // the 128-B lines of the streamed range
      pbytes += 128u * uint64_t((((s + n) * 8u + 127u) >> 7) - ((s * 8u) >> 7)) +
                128u * uint64_t((((s + n) * 2u + 127u) >> 7) - ((s * 2u) >> 7));
  };
  // wave reduction per class, one merge per (tile, code, class)
  auto finish = [&](uint32_t dim) __attribute__((always_inline)) {
#pragma unroll
    for (uint32_t k = 0; k < NK; k++) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        cnt[k] += __shfl_xor(cnt[k], off, 64);
        if (AGG == AGG_SUM) {
          const double oh = __shfl_xor(hi[k], off, 64);
          if (P.exact_sum) {
            hi[k] += oh;
          } else {
            const double ol = __shfl_xor(lo[k], off, 64);
            double sm, e;
            two_sum(hi[k], oh, sm, e);
            hi[k] = sm;
            lo[k] = lo[k] + ol + e;
          }
        } else {
          const unsigned long long o = __shfl_xor(ext[k], off, 64);
          ext[k] = AGG == AGG_MIN ? (o < ext[k] ? o : ext[k]) : (o > ext[k] ? o : ext[k]);
        }
      }
      if (lane == 0 && cnt[k]) {
        const unsigned long long cell = (glob_base + (unsigned long long)(cc.b0 + int64_t(k))) * P.ngroups + dim;
        global_merge<AGG, false>(P, cell, cnt[k], cnt[k], hi[k], lo[k], ext[k]);
      }
    }
  };

  // Split tiles whose ranges stream whole (LK_NO_CLU_SUB=1, or no sub-block area): a loop of their own, as above.
  while (!use_sub && emask) {
    const uint32_t c = uint32_t(__builtin_ctzll(emask));
    emask &= emask - 1ull;
    const uint32_t s = uni(__shfl(cs, int(c), 64)), e = uni(__shfl(ce, int(c), 64));
    if (s >= e) continue;   // the name is absent from the tile
    const uint32_t dim = (uni(__shfl(lut, int(c), 64)) & DIM_MASK) * stride;
#pragma unroll
    for (uint32_t k = 0; k < NK; k++) {
      hi[k] = lo[k] = 0.0;
      ext[k] = AGG == AGG_MIN ? ~0ull : 0ull;
      cnt[k] = 0u;
    }
    stream(std::integral_constant<uint32_t, 8u>{}, s, e - s);
    finish(dim);
  }
  // Split tiles with the sub-block area.
  bool first = true;
  while (emask) {
    const uint32_t c = uint32_t(__builtin_ctzll(emask));
    emask &= emask - 1ull;
    SubEnt en = pre;   // the first passing code's entries were loaded before the search
    if (!first) en = load_sub(c);   // uniform
    first = false;
    const uint32_t s = uni(__shfl(cs, int(c), 64)), e = uni(__shfl(ce, int(c), 64));
    if (s >= e) continue;   // the name is absent from the tile
    const uint32_t dim = (uni(__shfl(lut, int(c), 64)) & DIM_MASK) * stride;
#pragma unroll
    for (uint32_t k = 0; k < NK; k++) {
      hi[k] = lo[k] = 0.0;
      ext[k] = AGG == AGG_MIN ? ~0ull : 0ull;
      cnt[k] = 0u;
    }
    // lane j: the code's elements [a, b) of sub-block j and their aggregate (load_sub)
    const bool sl = lane < nsub;
    uint32_t a = en.a, b = en.b;
    const v2u g0 = en.g0, g1 = en.g1;   // SUM: hi, lo; MIN / MAX: the extreme
    const uint32_t snan = en.snan;      // MIN: the code's NaN bits
    if (!sl) a = b = e;
    b = b < e ? b : e;   // clamped to the code's range, as cpref is clamped to the tile's rows
    b = b > s ? b : s;
    a = a > s ? a : s;
    a = a < b ? a : b;
    // a whole sub-block of an in-window class starts its lane's accumulators with the stored aggregate
    if (subc != CLU_SUB_STRADDLE && subc >= 1u && subc < nsb && a < b) {
#pragma unroll
      for (uint32_t k = 0; k < NK; k++) {
        if (subc != k + 1u) continue;
        cnt[k] = b - a;
        if (AGG == AGG_SUM) {
          hi[k] = __longlong_as_double((long long)(((uint64_t)g0.y << 32) | g0.x));
          lo[k] = __longlong_as_double((long long)(((uint64_t)g1.y << 32) | g1.x));
        } else {
          ext[k] = ((unsigned long long)g0.y << 32) | g0.x;
        }
      }
      if (AGG == AGG_MIN && ((snan >> lane) & 1u)) nan_seen = true;
    }
    // the straddling sub-blocks' elements (at most CLU_SPLIT_MAX - 1 sub-blocks hold a boundary inside the tile)
    // are streamed on top; their ranges are taken into uniform registers first, so a / b end here
    unsigned long long strad = __ballot(sl && subc == CLU_SUB_STRADDLE && a < b);
    uint32_t ja[CLU_SPLIT_MAX], jn[CLU_SPLIT_MAX];
#pragma unroll
    for (uint32_t q = 0; q < CLU_SPLIT_MAX; q++) {
      ja[q] = jn[q] = 0u;
      if (strad) {   // uniform
        const int j = __builtin_ctzll(strad);
        strad &= strad - 1ull;
        ja[q] = uni(__shfl(a, j, 64));
        jn[q] = uni(__shfl(b, j, 64)) - ja[q];
      }
    }
#pragma unroll 1
    for (uint32_t q = 0; q < CLU_SPLIT_MAX; q++) {
      const uint32_t qa = q == 0u ? ja[0] : q == 1u ? ja[1] : q == 2u ? ja[2] : ja[3];
      const uint32_t qn = q == 0u ? jn[0] : q == 1u ? jn[1] : q == 2u ? jn[2] : jn[3];
      if (qn) stream(std::integral_constant<uint32_t, 8u>{}, qa, qn);
    }
    if (count_plan && lane == 0) {   // the 128-B lines of the csub / sagg entries read (MIN: and of the code's NaN bits)
      const uint32_t o0 = clu_sub_csub_off(d.dict_n) + c * (CLU_SUB_MAX + 1u) * 4u;
      pbytes += 128u * uint64_t(((o0 + (nsub + 1u) * 4u + 127u) >> 7) - (o0 >> 7)) +
                128u * uint64_t((nsub * uint32_t(sizeof(CluAgg)) + 127u) >> 7) + (AGG == AGG_MIN ? 128u : 0u);
    }
    finish(dim);
  }
  if (AGG == AGG_MIN && __ballot(nan_seen) && lane == 0) atomicOr(P.flags, FLAG_MIN_NAN);
  if (pbytes) atomicAdd(P.plan_bytes, (unsigned long long)pbytes);
}

}  // namespace lk
