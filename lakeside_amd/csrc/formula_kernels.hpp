// Host-visible interface of the formula kernels (formula_kernels.hip): the keyed combine of lk_eval_formula.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "formula_cell.hpp"

namespace lk {

constexpr unsigned long long FX_EMPTY = ~0ull;     // an unclaimed leaf slot / hash key
enum FxFlag : uint32_t { FX_FLAG_FULL = 1u, FX_FLAG_OFFGRID = 2u, FX_FLAG_RANGE = 4u };
// (FX_MAXCOL, the collapse ranks FX_RANK_* and FxXform: formula_cell.hpp, which the host's HIP-free rules include)

// The cell table: `nleaves` 64-bit slots per cell (name rank << 32 | row of the operand; FX_EMPTY: no row), dense
// (cell = bucket * U + union group) or open addressing on that 64-bit key.
struct FxTable {
  unsigned long long* slots;       // [ncells][nleaves]
  unsigned long long* keys;        // hash mode: [ncells] cell keys (FX_EMPTY: free); dense: null
  unsigned long long ncells;       // dense: nbuckets * U; hash: slots (a power of two)
  unsigned long long U;            // union group space
  unsigned long long nbuckets;
  int64_t base, step;              // bucket b = (ts - base) / step
  uint32_t* flags;                 // FxFlag bits
  uint32_t* live;                  // hash mode: claimed keys
  int nleaves;
};

// One referenced expression: its merged rows on the device and the tables that key them.
struct FxOperand {
  const int64_t* ts;
  const double* val;
  const uint32_t* gid;
  uint32_t nrows;
  int leaf;
  int ncols;                               // groupBy columns (the key tuple, in the formula's column order)
  unsigned long long stride[FX_MAXCOL];    // of the operand's group id
  unsigned long long ndim[FX_MAXCOL];
  unsigned long long ustride[FX_MAXCOL];   // of the union group id
  const uint32_t* map[FX_MAXCOL];          // dim id -> union id (0: the tag is absent, read as ""); null: every
                                           // operand reads this column through the same engine dictionary, so the
                                           // union id is dim id + 1 but for the absent ids below (no table)
  uint32_t dim_null[FX_MAXCOL];            // map == null: the dim ids that read as absent (NULL, "" and "null")
  uint32_t nl0[FX_MAXCOL], nl1[FX_MAXCOL];
  unsigned long long name_stride, name_ndim;
  const uint32_t* name_rank;               // name dim id -> collapse rank, 2 * (string order) + 4 (FX_RANK_ABSENT: no
                                           // name tag: ranked by `after_name`)
  uint32_t after_name;                     // bit c: groupBy column c's tag name sorts after the name column's
  unsigned long long qt_u;                 // a row whose own tags are all absent: its union group (queryTags) ...
  uint32_t qt_rank;                        // ... and rank
};

struct FxEval {
  FxTable T;
  int nops;
  int has_group_bys;
  FxOp ops[FX_MAXPROG];
  const double* val[FX_MAXLEAF];
  const uint32_t* gid[FX_MAXLEAF];
  int xform[FX_MAXLEAF];           // ASTUtils.getTransformerFunc, applied twice (see formula_eval.cpp)
  double secs[FX_MAXLEAF];
  // hash mode: rows ascending in time through per-bucket counts (scanned) and cursors
  uint32_t* bucket_count;          // [nbuckets + 1]
  uint32_t* bucket_cursor;         // [nbuckets]
};

hipError_t launch_fx_fill(unsigned long long* p, unsigned long long n, hipStream_t st);
hipError_t launch_fx_scatter(const FxTable& T, const FxOperand& O, hipStream_t st);
uint32_t fx_blocks(unsigned long long ncells);
// counts: fx_blocks(ncells) + 1 entries; the row total lands at counts[fx_blocks] (dense) or
// bucket_count[nbuckets] (hash) after the scan
hipError_t launch_fx_eval_count(const FxEval& E, uint32_t* counts, hipStream_t st);
hipError_t launch_fx_eval_write(const FxEval& E, const uint32_t* counts, int64_t* ts, double* val, int32_t* src_op,
                                uint32_t* src_gid, hipStream_t st);

}  // namespace lk
