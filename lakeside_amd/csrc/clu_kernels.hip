// clu_build: the name-clustered value copy of a segment's eligible tiles (layout.hpp, CluTile), built once at load on
// the load stream (Engine::build_segment) from the name codes and values already in HBM.  One workgroup per tile: a
// stable counting sort of the tile's rows by chunk-dictionary code -- codes ascending, rows ascending within a code, so
// the layout is deterministic.  Not a hot kernel: every row's code is decoded twice (histogram, then placement), and a
// 256-row step ranks its rows by ballot within the wave and through per-wave counts in LDS across waves.
// Then the per-code aggregates (`cagg`, the NaN mask): a wave takes codes w, w + 4, ... and reduces each one's range
// of the cvals the workgroup has just written with clu_reduce_pinned (clu_reduce.hpp) -- the function scan_clu streams
// a pinned tile's range with, so the stored triple is what that stream hands global_merge, bit for bit.
// Then the segment's sub-block area (clu.hpp: csub, sagg, the per-code NaN bits), for scan_clu's split tiles: pass 2
// walks the rows in order, so at every step that opens a 4,096-row sub-block `next[c]` is code c's first element of
// that sub-block; behind the cagg pass' fences the (code, sub-block) ranges are reduced with the same function, spread
// over the four waves.
// Every global store is clamped to the tile's block or sub-block area, every stream read goes through a buffer resource.
#include <hip/hip_runtime.h>

#include "clu_reduce.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace lk {
namespace {

__global__ __launch_bounds__(BLOCK) void clu_build(CluBuild B) {
  constexpr uint32_t NW = BLOCK / 64;
  __shared__ LRun runs[RUN_CAP];
  __shared__ uint32_t next[64];        // histogram, then the next output position of every code
  __shared__ uint32_t wcnt[NW][64];    // the step's rows per (wave, code)
  __shared__ uint32_t cst[65];         // cpref (the aggregate pass reads the ranges from here)
  __shared__ unsigned long long nanm;  // bit c: a NaN among code c's values
  __shared__ uint32_t snan[64];        // per code, bit j: a NaN among its elements of sub-block j
  __shared__ uint32_t lsub[64][CLU_SUB_MAX + 1u];   // csub (the sub-block pass reads the ranges from here)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const uint32_t t = blockIdx.x;
  if (t >= B.ntiles) return;
  const CluTile d = B.desc[t];
  if (d.off == CLU_NO_COPY) return;    // uniform
  const TileCol* tn = B.name_tc + t;
  const TileCol* tv = B.val_tc + t;
  const uint32_t nrows = d.nrows < TILE_ROWS ? d.nrows : TILE_ROWS;
  const uint32_t dict_n = d.dict_n < 1u ? 1u : (d.dict_n > 64u ? 64u : d.dict_n);
  const uint32_t nr = tn->nruns < RUN_CAP ? tn->nruns : RUN_CAP;
  const int bw = int(tn->bw);
  const uint32_t vbn = tn->vbase, vbv = tv->vbase;
  const __amdgpu_buffer_rsrc_t rn = make_rsrc(B.base + tn->vals, tn->vals_len + 8u);   // (as every hybrid_get_buf caller)
  const __amdgpu_buffer_rsrc_t rvv = make_rsrc(B.base + tv->vals, tv->vals_len);
  uint8_t* blk = B.clu + d.off;
  uint32_t* cpref = reinterpret_cast<uint32_t*>(blk);
  unsigned long long* cvals = reinterpret_cast<unsigned long long*>(blk + clu_vals_off(dict_n));
  uint16_t* crows = reinterpret_cast<uint16_t*>(blk + clu_rows_off(nrows, dict_n));
  // the tile's sub-block area (clu.hpp): every store below is clamped to it
  const bool has_sub = B.sub != nullptr && clu_sub_bytes(dict_n) <= B.sub_stride;   // uniform
  uint8_t* sblk = has_sub ? B.sub + size_t(t) * B.sub_stride : nullptr;
  uint32_t* csub = has_sub ? reinterpret_cast<uint32_t*>(sblk + clu_sub_csub_off(dict_n)) : nullptr;
  const uint32_t nsub = clu_nsub(nrows);

  if (tid < 64u) snan[tid] = 0u;
  for (uint32_t i = tid; i < nr; i += BLOCK) {
    const RunDesc r = B.name_runs[tn->run_lo + i];
    runs[i] = LRun{r.start, r.off_lit, r.value};
  }
  if (tid < 64u) next[tid] = 0u;
  if (tid == 0u) nanm = 0ull;
  for (uint32_t i = tid; i < NW * 64u; i += BLOCK) (&wcnt[0][0])[i] = 0u;
  __syncthreads();
  if (nr == 0u) return;                // uniform (an eligible tile has runs)
  auto code_of = [&](uint32_t r) __attribute__((always_inline)) -> uint32_t {
    const uint32_t v = vbn + r;
    const uint32_t c = hybrid_get_buf(rn, runs[find_run(runs, int(nr), v)], v, bw);
    return c < dict_n ? c : dict_n - 1u;   // (codes were validated against the dictionary at load)
  };

  // pass 1: rows per code, then the exclusive prefix (cpref[c] = first element of code c; cpref[64] = rows)
  for (uint32_t r = tid; r < nrows; r += BLOCK) atomicAdd(&next[code_of(r)], 1u);
  __syncthreads();
  if (w == 0u) {
    const uint32_t n = next[lane];
    uint32_t inc = n;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
      const uint32_t o = __shfl_up(inc, dd, 64);
      if (int(lane) >= dd) inc += o;
    }
    next[lane] = inc - n;
    cpref[lane] = inc - n;
    cst[lane] = inc - n;
    if (lane == 63u) cpref[64] = cst[64] = inc;
  }
  __syncthreads();

  // pass 2: 256 rows per step, in row order
  for (uint32_t r0 = 0; r0 < nrows; r0 += BLOCK) {
    // a step that opens sub-block j: next[c] is code c's first element of a row >= CLU_SUB_ROWS * j, that is csub[c][j]
    if ((r0 & (CLU_SUB_ROWS - 1u)) == 0u && tid < dict_n) {
      const uint32_t j = r0 / CLU_SUB_ROWS;   // < CLU_SUB_MAX: r0 < nrows <= TILE_ROWS
      lsub[tid][j] = next[tid];
      if (has_sub) csub[tid * (CLU_SUB_MAX + 1u) + j] = next[tid];
    }
    const uint32_t r = r0 + tid;
    const bool valid = r < nrows;
    const uint32_t c = valid ? code_of(r) : 0u;
    const v2u x = __builtin_amdgcn_raw_buffer_load_b64(rvv, valid ? (vbv + r) * 8u : OOB, 0, 0);
    uint32_t rank = 0;
    unsigned long long rem = __ballot(valid);
    while (rem) {   // uniform: one trip per distinct code of the wave's rows
      const int l = __builtin_ctzll(rem);
      const uint32_t cl = uint32_t(__shfl(int(c), l, 64));
      const unsigned long long m = __ballot(valid && c == cl);
      if (valid && c == cl) {
        rank = uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
        if (int(lane) == l) wcnt[w][cl] = uint32_t(__popcll(m));
      }
      rem &= ~m;
    }
    __syncthreads();
    if (valid) {
      uint32_t pos = next[c] + rank;
      for (uint32_t ww = 0; ww < w; ww++) pos += wcnt[ww][c];
      if (pos < nrows) {
        cvals[pos] = ((unsigned long long)x.y << 32) | x.x;
        crows[pos] = uint16_t(r);
      }
    }
    __syncthreads();
    if (tid < 64u) {
      uint32_t s = 0;
#pragma unroll
      for (uint32_t ww = 0; ww < NW; ww++) {
        s += wcnt[ww][tid];
        wcnt[ww][tid] = 0u;
      }
      next[tid] += s;
    }
    __syncthreads();
  }

  if (tid < dict_n)   // csub's entries past the tile's sub-blocks repeat cpref[c + 1]
    for (uint32_t j = nsub; j <= CLU_SUB_MAX; j++) {
      lsub[tid][j] = cst[tid + 1u];
      if (has_sub) csub[tid * (CLU_SUB_MAX + 1u) + j] = cst[tid + 1u];
    }

  // pass 3: cagg.  The cvals were stored by other lanes: each thread's stores are fenced before the barrier, and the
  // reading waves fence again behind it before their buffer loads.
  __threadfence();
  __syncthreads();
  __threadfence();
  const __amdgpu_buffer_rsrc_t rcv = make_rsrc(reinterpret_cast<const uint8_t*>(cvals), nrows * 8u);
  CluAgg* cagg = reinterpret_cast<CluAgg*>(blk + CLU_AGG_OFF);
  for (uint32_t c = w; c < dict_n; c += NW) {   // uniform per wave
    uint32_t ce = cst[c + 1u], cs = cst[c];     // clamped as scan_clu clamps cpref
    ce = ce < nrows ? ce : nrows;
    cs = cs < ce ? cs : ce;
    const CluRed r = clu_reduce_pinned<true, true, true, 16u>(rcv, uni(cs), uni(ce - cs), lane, false);
    if (lane == 0u) {
      cagg[c] = CluAgg{r.hi, r.lo, r.omin, r.omax};
      if (r.nan) atomicOr(&nanm, 1ull << c);
    }
  }
  // pass 4: sagg, the (code, sub-block) ranges spread over the waves, reduced with the same function (behind the same
  // fences); sub-blocks past the tile's rows get the empty range's entry.  4 loads per lane in flight where cagg and
  // scan_clu use 16: a range here is about 256 elements, and the depth changes neither which elements a lane takes
  // (l, l + 64, ...) nor their order, so the result is the one any depth gives
  if (has_sub) {   // uniform
    CluAgg* sagg = reinterpret_cast<CluAgg*>(sblk);
    for (uint32_t p = w; p < dict_n * CLU_SUB_MAX; p += NW) {   // uniform per wave; p = c * CLU_SUB_MAX + j
      const uint32_t c = p / CLU_SUB_MAX, j = p % CLU_SUB_MAX;
      uint32_t se = lsub[c][j + 1u], ss = lsub[c][j];
      se = se < nrows ? se : nrows;
      ss = ss < se ? ss : se;
      if (j >= nsub) ss = se;
      const CluRed r = clu_reduce_pinned<true, true, true, 4u>(rcv, uni(ss), uni(se - ss), lane, false);
      if (lane == 0u) {
        sagg[p] = CluAgg{r.hi, r.lo, r.omin, r.omax};
        if (r.nan) atomicOr(&snan[c], 1u << j);
      }
    }
  }
  __syncthreads();
  if (tid == 0u) *reinterpret_cast<unsigned long long*>(blk + CLU_NAN_OFF) = nanm;
  if (has_sub && tid < dict_n) reinterpret_cast<uint16_t*>(sblk + clu_sub_nan_off(dict_n))[tid] = uint16_t(snan[tid]);
}

// clu_samp_build: the timestamp sample tables of a segment whose every tile has sorted PLAIN64 timestamps (clu.hpp):
// one workgroup per tile, thread s copies the raw timestamp of row clu_samp_row(s, nrows) to entry s of the tile's
// table.  The read goes through a buffer resource over the tile's stream, the store stays inside the tile's table.
__global__ __launch_bounds__(CLU_SAMP_N) void clu_samp_build(SampBuild B) {
  const uint32_t t = blockIdx.x, s = threadIdx.x;
  if (t >= B.ntiles || s >= CLU_SAMP_N) return;
  const uint32_t n = B.tiles[t].nrows;
  const uint32_t nrows = n < TILE_ROWS ? n : TILE_ROWS;
  const TileCol* tt = B.ts_tc + t;
  const __amdgpu_buffer_rsrc_t rts = make_rsrc(B.base + tt->vals, tt->vals_len);
  const v2u x = __builtin_amdgcn_raw_buffer_load_b64(rts, (tt->vbase + clu_samp_row(s, nrows)) * 8u, 0, 0);
  reinterpret_cast<unsigned long long*>(B.samp + clu_samp_tile_off(t))[s] = ((unsigned long long)x.y << 32) | x.x;
}

}  // namespace

hipError_t launch_clu_samp_build(const SampBuild& B, hipStream_t st) {
  if (B.ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(clu_samp_build, dim3(B.ntiles), dim3(CLU_SAMP_N), 0, st, B);
  return hipGetLastError();
}

hipError_t launch_clu_build(const CluBuild& B, hipStream_t st) {
  if (B.ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(clu_build, dim3(B.ntiles), dim3(BLOCK), 0, st, B);
  return hipGetLastError();
}

}  // namespace lk
