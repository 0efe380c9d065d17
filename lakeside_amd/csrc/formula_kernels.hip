// HIP kernels for gfx950 (MI355X): the keyed combine of a formula over DataExprs (lk_eval_formula, formula_eval.cpp).
//
// Every referenced expression's merged rows (timestamp, value, group id) sit on the device.  A cell is one
// (bucket, union group); it holds one 64-bit slot per leaf.
//   fx_scatter (one launch per operand): a thread per row computes the row's cell -- bucket from the timestamp, union
//     group from the operand's dim id -> union id tables -- and claims the cell's leaf slot with a 64-bit atomicMin on
//     (name rank << 32 | row): rows of one expression at one timestamp that share a group key collapse to the one with
//     the smallest sorted tag list (BaseExpr.eval keeps one result per toGroupByKey, BaseExpr.scala:689-690; the rule
//     is eval_merged_rows').  In hash mode the cell's key is inserted first with a 64-bit atomicCAS (linear probing).
//   fx_eval_count / fx_eval_write: a thread per cell gathers the winners' values, applies each leaf's chart
//     transformer twice (QueryEngineV2.evaluateFormula runs BaseExpr.eval on a leaf twice, QueryEngineV2.scala:344-371),
//     runs fx_eval_cell (formula_cell.hpp) and compacts the live cells: dense cells are bucket-major, so per-block
//     counts + finalize_scan + ballot / mbcnt positions give rows ascending in time; hash cells count per bucket, scan
//     the buckets and take a position from their bucket's cursor.
// Bandwidth-plus-atomics kernels: wave64, 256 threads.  Integer atomics only; the arithmetic is plain IEEE double
// (this unit is built with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "formula_kernels.hpp"

namespace lk {

constexpr int FXB = 256;
constexpr int FXITEMS = 8;

__global__ __launch_bounds__(FXB) void fx_fill(unsigned long long* p, unsigned long long n) {
  const unsigned long long i = (unsigned long long)blockIdx.x * FXB + threadIdx.x;
  if (i < n) p[i] = FX_EMPTY;
}

__device__ __forceinline__ unsigned long long fx_mix(unsigned long long x) {   // splitmix64 finalizer
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

__global__ __launch_bounds__(FXB) void fx_scatter(FxTable T, FxOperand O) {
  const uint32_t row = blockIdx.x * FXB + threadIdx.x;
  if (row >= O.nrows) return;
  const int64_t d = O.ts[row] - T.base;
  if (d < 0 || d % T.step != 0) {
    atomicOr(T.flags, uint32_t(FX_FLAG_OFFGRID));
    return;
  }
  const unsigned long long b = (unsigned long long)(d / T.step);
  if (b >= T.nbuckets) {
    atomicOr(T.flags, uint32_t(FX_FLAG_RANGE));
    return;
  }
  const unsigned long long g = O.gid[row];
  unsigned long long u = 0;
  uint32_t present = 0;
  for (int c = 0; c < O.ncols; c++) {
    const unsigned long long dim = (g / O.stride[c]) % O.ndim[c];
    const uint32_t uc = O.map[c] ? O.map[c][dim]
                                 : ((dim == O.dim_null[c] || dim == O.nl0[c] || dim == O.nl1[c]) ? 0u : uint32_t(dim) + 1u);
    u += (unsigned long long)uc * O.ustride[c];
    present |= uc ? (1u << c) : 0u;
  }
  uint32_t rank = O.name_rank[(g / O.name_stride) % O.name_ndim];
  if (rank == FX_RANK_ABSENT) {
    if (!present) {          // every own tag absent: the row takes its glob's queryTags (Commons.scala:450-452)
      u = O.qt_u;
      rank = O.qt_rank;
    } else {                 // no name tag: first when no present groupBy tag sorts after it, else last
      rank = (present & O.after_name) ? FX_RANK_NONAME_LAST : FX_RANK_NONAME_FIRST;
    }
  }
  if (u >= T.U) {
    atomicOr(T.flags, uint32_t(FX_FLAG_RANGE));
    return;
  }
  const unsigned long long key = b * T.U + u;
  unsigned long long cell = key;
  if (T.keys) {
    const unsigned long long mask = T.ncells - 1;
    unsigned long long h = fx_mix(key) & mask;
    unsigned long long probes = 0;
    for (;;) {
      const unsigned long long old = atomicCAS(&T.keys[h], FX_EMPTY, key);
      if (old == FX_EMPTY) {
        // three quarters full: the host regrows the table and scatters again
        if (atomicAdd(T.live, 1u) + 1u > (T.ncells >> 2) * 3u) atomicOr(T.flags, uint32_t(FX_FLAG_FULL));
        break;
      }
      if (old == key) break;
      h = (h + 1) & mask;
      if (++probes >= T.ncells) {
        atomicOr(T.flags, uint32_t(FX_FLAG_FULL));
        return;
      }
    }
    cell = h;
  }
  atomicMin(&T.slots[cell * (unsigned long long)T.nleaves + (unsigned long long)O.leaf],
            ((unsigned long long)rank << 32) | row);
}

struct FxRow {
  bool exists;
  double value;
  int32_t src;
  uint32_t gid;
  unsigned long long bucket;
};

__device__ __forceinline__ double fx_transform(double v, int xf, double secs) {
  if (xf == FX_XF_MUL) return (v * secs) * secs;
  if (xf == FX_XF_DIV) return (v / secs) / secs;
  return v;
}

__device__ FxRow fx_row(const FxEval& E, unsigned long long cell) {
  FxRow r{false, 0.0, FX_SRC_CONST, 0u, 0ull};
  const FxTable& T = E.T;
  unsigned long long key = cell;
  if (T.keys) {
    key = T.keys[cell];
    if (key == FX_EMPTY) return r;
  }
  uint8_t present[FX_MAXLEAF];
  double value[FX_MAXLEAF];
  int32_t src[FX_MAXLEAF];
  uint32_t rows[FX_MAXLEAF];
  bool any = false;
#pragma unroll
  for (int l = 0; l < FX_MAXLEAF; l++) {
    present[l] = 0;
    value[l] = 0.0;
    src[l] = l;
    rows[l] = 0;
    if (l < T.nleaves) {
      const unsigned long long s = T.slots[cell * (unsigned long long)T.nleaves + (unsigned long long)l];
      if (s != FX_EMPTY) {
        rows[l] = uint32_t(s);
        present[l] = 1;
        value[l] = fx_transform(E.val[l][rows[l]], E.xform[l], E.secs[l]);
        any = true;
      }
    }
  }
  if (!any) return r;
  const FxCell c = fx_eval_cell(E.ops, E.nops, present, value, src);
  if (!c.present) return r;
  r.exists = true;
  r.value = c.value;
  r.src = c.src;
  // a constant's tags: none without groupBys (ASTUtils.scala:50-53); with groupBys those of a row of this key and
  // timestamp (ASTUtils.scala:55-63) -- the first referenced expression present in the cell
  if (r.src == FX_SRC_CONST && E.has_group_bys) {
#pragma unroll
    for (int l = FX_MAXLEAF - 1; l >= 0; l--)
      if (present[l]) r.src = l;
  }
#pragma unroll
  for (int l = 0; l < FX_MAXLEAF; l++)
    if (r.src == l) r.gid = E.gid[l][rows[l]];
  r.bucket = key / T.U;
  return r;
}

__global__ __launch_bounds__(FXB) void fx_eval_count(FxEval E, uint32_t* block_counts) {
  __shared__ uint32_t ws[FXB / 64];
  uint32_t n = 0;
  const unsigned long long base = (unsigned long long)blockIdx.x * FXB * FXITEMS;
  for (int i = 0; i < FXITEMS; i++) {
    const unsigned long long cell = base + (unsigned long long)i * FXB + threadIdx.x;
    if (cell >= E.T.ncells) continue;
    const FxRow r = fx_row(E, cell);
    if (!r.exists) continue;
    n++;
    if (E.T.keys) atomicAdd(&E.bucket_count[r.bucket], 1u);
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < FXB / 64; w++) t += ws[w];
    block_counts[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(FXB) void fx_eval_write(FxEval E, const uint32_t* block_offsets, int64_t* out_ts,
                                                  double* out_val, int32_t* out_op, uint32_t* out_gid) {
  __shared__ uint32_t ws[FXB / 64];
  const unsigned long long base = (unsigned long long)blockIdx.x * FXB * FXITEMS;
  uint32_t off = block_offsets[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < FXITEMS; i++) {
    const unsigned long long cell = base + (unsigned long long)i * FXB + threadIdx.x;
    FxRow r{false, 0.0, FX_SRC_CONST, 0u, 0ull};
    if (cell < E.T.ncells) r = fx_row(E, cell);
    const unsigned long long m = __ballot(r.exists);
    if (lane == 0) ws[wave] = __popcll(m);
    __syncthreads();
    uint32_t wb = 0, tot = 0;
    for (int w = 0; w < FXB / 64; w++) {
      wb += (w < wave) ? ws[w] : 0;
      tot += ws[w];
    }
    if (r.exists) {
      uint32_t pos;
      if (E.T.keys) pos = E.bucket_count[r.bucket] + atomicAdd(&E.bucket_cursor[r.bucket], 1u);
      else pos = off + wb + __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
      out_ts[pos] = E.T.base + int64_t(r.bucket) * E.T.step;
      out_val[pos] = r.value;
      out_op[pos] = r.src;
      out_gid[pos] = r.gid;
    }
    off += tot;
    __syncthreads();
  }
}

// kernels.hip: the single-block exclusive scan of the finalize path (total at counts[n])
hipError_t launch_scan_counts(uint32_t* counts, uint32_t n, hipStream_t st);

uint32_t fx_blocks(unsigned long long ncells) { return uint32_t((ncells + FXB * FXITEMS - 1) / (FXB * FXITEMS)); }

hipError_t launch_fx_fill(unsigned long long* p, unsigned long long n, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fx_fill, dim3(uint32_t((n + FXB - 1) / FXB)), dim3(FXB), 0, st, p, n);
  return hipGetLastError();
}

hipError_t launch_fx_scatter(const FxTable& T, const FxOperand& O, hipStream_t st) {
  if (!O.nrows) return hipSuccess;
  hipLaunchKernelGGL(fx_scatter, dim3((O.nrows + FXB - 1) / FXB), dim3(FXB), 0, st, T, O);
  return hipGetLastError();
}

hipError_t launch_fx_eval_count(const FxEval& E, uint32_t* counts, hipStream_t st) {
  const uint32_t nb = fx_blocks(E.T.ncells);
  if (!nb) return hipMemsetAsync(counts, 0, sizeof(uint32_t), st);
  hipLaunchKernelGGL(fx_eval_count, dim3(nb), dim3(FXB), 0, st, E, counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_counts(counts, nb, st);
  if (e != hipSuccess) return e;
  if (E.T.keys) e = launch_scan_counts(E.bucket_count, uint32_t(E.T.nbuckets), st);
  return e;
}

hipError_t launch_fx_eval_write(const FxEval& E, const uint32_t* counts, int64_t* ts, double* val, int32_t* src_op,
                                uint32_t* src_gid, hipStream_t st) {
  const uint32_t nb = fx_blocks(E.T.ncells);
  if (!nb) return hipSuccess;
  hipLaunchKernelGGL(fx_eval_write, dim3(nb), dim3(FXB), 0, st, E, counts, ts, val, src_op, src_gid);
  return hipGetLastError();
}

}  // namespace lk
