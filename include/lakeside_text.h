/* Host-only test hook: the Java 17 Double.toString / Float.toString text the exemplar path prints for DOUBLE / FLOAT
 * columns (lakeside_amd/csrc/jdtoa.cpp; the reference gets it from DuckDB's JDBC getString, Commons.scala:428-459).
 * Built as lakeside_amd/liblakeside_text.so for the CPU differential tests; the evaluator links the same source.
 * Not part of the drop-in boundary (include/lakeside_gpu.h). */
#ifndef LAKESIDE_TEXT_H
#define LAKESIDE_TEXT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Writes the NUL-terminated text of x into buf; returns its length, or -1 when cap is too small (32 always fits). */
int lk_java_double_text(double x, char* buf, size_t cap);
int lk_java_float_text(float x, char* buf, size_t cap);

/* The double a field chart aggregates for the text s[0..n) of a VARCHAR chart field (lakeside_amd/csrc/fieldnum.cpp):
 * 1 and *out = the number when the whole text matches -?[0-9]+(\.[0-9]+)?([eE][-+]?[0-9]+)? and is finite; 0 when the
 * cast is NULL (the first byte is an ASCII letter other than i I n N); -1 for every other text, which the evaluator
 * refuses (LK_ERR_UNSUPPORTED) instead of guessing DuckDB's cast.  out may be NULL. */
int lk_field_number(const char* s, size_t n, double* out);

/* Formulas over DataExprs (lk_eval_formula, include/lakeside_gpu.h), the host-only parts (lakeside_amd/csrc/formula.cpp,
 * formula_cell.hpp).  lk_formula_plan parses `formula` over the n variables `names` and writes its postfix program into
 * out (NUL-terminated, truncated to cap): one token per operation, `$<i>` = variable names[i], a constant as Java's
 * Double.toString prints it, `+ - * /`.  Returns 0; -1 (LK_ERR_ARG: unknown variable, unbalanced parentheses, a single
 * term, malformed text) or -2 (LK_ERR_UNSUPPORTED: `^`, relational operators, unary signs) with the reason in out. */
int lk_formula_plan(const char* formula, const char* const* names, size_t n, char* out, size_t cap);
/* Runs the formula's program over ncells cells with the function the GPU kernels compile (fx_eval_cell).  Per cell c
 * and variable i (n <= 8): present[c * n + i] (0 / 1), value[c * n + i], src[c * n + i] (the tag source handed through).
 * Per cell: out_present, out_value, out_src (-1: a constant's tags).  Returns 0 or lk_formula_plan's error. */
int lk_formula_eval_cell(const char* formula, const char* const* names, size_t n, size_t ncells, const uint8_t* present,
                         const double* value, const int32_t* src, uint8_t* out_present, double* out_value,
                         int32_t* out_src);

/* What lk_eval_formula decides from its request alone, before it evaluates an operand or enters a collective
 * (lakeside_amd/csrc/formula_join.cpp, fx_gate, with the plain request parser in place of the engine's cache).
 * formula_json is lk_eval_formula's: {"formula", "expressions": {var: {"pushDown", "paths", "shard"?}}}.  dist = 0: a
 * local call, "shard" is not read (world is 1); dist != 0: lk_eval_formula_dist among `world` ranks.  Writes into out
 * (NUL-terminated) {"program": the postfix program as lk_formula_plan prints it, its leaves numbered over the
 * referenced expressions in the order of "expressions"; "operands": per referenced expression in that order {"var",
 * "paths", "shard" ([]: i % world), "uploaded" (values assembled on the host), "xform" ("none" / "mul" / "div": the
 * chart transformer)}; "order": the variables in evaluation order (ascending bytes); "key_cols": the sorted groupBy set;
 * "step"; "secs"}.  Returns 0, or the refusal's code (LK_ERR_ARG -1, LK_ERR_UNSUPPORTED -2) with its message in out; -5
 * when cap is too small. */
int lk_formula_gate_sim(const char* formula_json, int dist, int world, char* out, size_t cap);
/* The union group space, the collapse ranks and the cell space of a formula's join (formula_join.cpp, fx_union_space
 * and fx_cell_space) over operands described by their dimension texts.  spec_json: {"key_cols": [groupBy column],
 * "operands": [null (an expression without rows) | {"name": DIM, "keys": [DIM per key column], "query_tags": [[tag name,
 * value]] (the first glob's)}], "ident"?: [null | {"ndim", "dict": {text: dictionary id}} per key column],
 * "cells"?: {"base", "last", "step"}}, DIM = {"tag": the column's tag name, "dims": [text | null (absent) per dim id]}
 * or, for a column that must not be walked, {"tag", "ndim"}: asking for one of its texts fails the call.  An "ident"
 * entry makes its column an identity column: union id = dictionary id + 1 for ids below ndim - 1, texts outside them
 * numbered from ndim + 1 in order of first appearance.  Writes {"U", "ustride", "operands": [{"maps": [[union id per
 * dim id] per key column, [] for an identity column], "name_rank", "after_name", "qt_ids", "qt_u", "qt_rank"}]} and,
 * with "cells", "nbuckets" and "nkeys".  Returns as lk_formula_gate_sim does. */
int lk_formula_union_sim(const char* spec_json, char* out, size_t cap);

/* Runs the exemplar row selection (ex_select.hpp) for one glob over the n passing rows' timestamps ts[0..n), with a
 * CPU histogram standing in for ex_scan HIST: a row counts in a pass iff rlo <= ts < rhi, in bin
 * clamp((ts - hbase) / hwidth, 0, nb - 1).  tiles: ntiles x (ts_min, ts_max, nrows) zone maps for the probes
 * (ntiles = 0: no probing).  Writes the emit range [*elo, *ehi), the rows counted in it and the passes taken; limit = 0
 * (the evaluator opens no such glob): no pass, no rows, the empty range at the ordered end of the window. */
int lk_ex_select_sim(const int64_t* ts, size_t n, int64_t win_lo, int64_t win_hi, const int64_t* tiles, size_t ntiles,
                     uint64_t limit, int desc, uint64_t cand_cap, uint64_t probe_rows,
                     int64_t* elo, int64_t* ehi, uint64_t* count, int* passes);

/* Runs the row -> bucket rule the scan kernels inline (lakeside_amd/csrc/bucket.hpp) over ts[0..n): bucket_row with the
 * window [win_lo, win_hi), inv_step = 1.0 / step as the evaluator sets it, and fast_div as given (the caller keeps to
 * its domain, 0 <= ts - base < 2^32 and step < 2^31) into bucket[i] / status[i] (0 inside, 1 outside the window,
 * 2 metrics-unaligned, 3 out of range; the bucket of an outside row is unspecified), and bucket_mono into mono[i]. */
void lk_bucket_sim(const int64_t* ts, size_t n, int64_t win_lo, int64_t win_hi, int64_t step, int64_t base,
                   uint64_t nbuckets, int metrics, int fast_div, int64_t* bucket, uint8_t* status, int64_t* mono);

/* Runs the name-clustered value copy's tile rule (lakeside_amd/csrc/clu.hpp, clu_classify as scan_clu inlines it) over
 * n tiles given by their timestamp zone maps and sorted flags: kind[i] = 0 outside the window, 1 pinned to bucket b0[i],
 * 2 split (nsb[i] class boundaries, first bucket b0[i]), 3 inside the window but not taken.  lk_clu_segment_taken is
 * the host's rule for a whole segment (every tile has a copy and sorted timestamps; `widest` = the largest
 * ts_max - ts_min of its tiles): 1 when scan_clu takes the segment, so scan_lean need not run over it. */
void lk_clu_sim(const int64_t* ts_min, const int64_t* ts_max, const uint8_t* sorted, size_t n, int64_t win_lo,
                int64_t win_hi, int64_t step, int64_t base, uint64_t nbuckets, int split_ok, uint8_t* kind, int64_t* b0,
                uint32_t* nsb);
int lk_clu_segment_taken(int all_copies_sorted, int64_t widest, int64_t step);
/* The bytes of one tile block of the clustered copy (lakeside_amd/csrc/clu.hpp, clu_block_bytes: what the engine
 * allocates and charges per tile) for a tile of nrows rows whose name chunk dictionary has dict_n entries (taken as
 * 1 .. 64); the byte offsets within the block of the per-code aggregates, the values and the row indices go to
 * agg_off / vals_off / rows_off where non-NULL. */
uint64_t lk_clu_block_bytes(uint32_t nrows, uint32_t dict_n, uint32_t* agg_off, uint32_t* vals_off, uint64_t* rows_off);
/* The bytes of one tile's sub-block area (clu.hpp, clu_sub_bytes: a tile's stride when dict_n is its segment's largest)
 * for a tile of nrows rows (the area is sized for the most sub-blocks a tile can have, so nrows decides *nsub alone);
 * where non-NULL: nsub = the tile's sub-blocks, sub_rows / sub_max = the constants, sagg_off = the byte offset of code
 * c's aggregate of sub-block j (c, j as given), csub_off / nan_off = the offsets of the first code's csub entries and of
 * the first code's NaN mask. */
uint32_t lk_clu_sub_bytes(uint32_t nrows, uint32_t dict_n, uint32_t c, uint32_t j, uint32_t* nsub, uint32_t* sub_rows,
                          uint32_t* sub_max, uint32_t* sagg_off, uint32_t* csub_off, uint32_t* nan_off);
/* The whole-or-straddling rule of a split tile's sub-blocks (clu.hpp, clu_sub_class as scan_clu calls it): for a tile of
 * nrows rows with boundary rows sb[0 .. nsb) (ascending; sb[k] = the first row of class k + 1; nsb <= 4), cls[j] = the
 * class of every row of sub-block j, or 0xffffffff when the sub-block's rows must be streamed.  Returns the sub-blocks. */
uint32_t lk_clu_sub_sim(uint32_t nrows, const uint32_t* sb, uint32_t nsb, uint32_t* cls);
/* A tile's timestamp sample table as clu_build lays it out (clu.hpp, clu_samp_row): given the tile's timestamps
 * ts[0 .. nrows), table[s] = ts[(s * nrows) >> 8] for s = 0 .. 255, the rows scan_clu's boundary search samples (below
 * 256 rows they repeat).  Returns 256, or -1 for nrows outside 1 .. 65,536. */
int lk_clu_samples_sim(const int64_t* ts, uint32_t nrows, int64_t* table);
/* The byte offset of tile `tile`'s table in a segment's area of sample tables (clu.hpp, clu_samp_tile_off); where
 * non-NULL: samp_bytes = a table's size. */
uint64_t lk_clu_samp_layout(uint32_t tile, uint32_t* samp_bytes);
/* COUNT over a split tile needs no value (clu.hpp, clu_count_split, the arithmetic of scan_clu<AGG_COUNT>): the
 * per-class counts of one code of a tile of nrows rows (<= 65,536), given the rows within the tile of its n elements
 * (rows[0 .. n), strictly ascending: the code's crows) and the boundary rows sb[0 .. nsb) (ascending, nsb <= 4).  The
 * code's csub entries are built from the rows here.  use_sub != 0: whole sub-blocks add their csub difference to
 * their class and only the straddling ones' elements are classed one by one; 0: every element is.  cnt[0 .. 4] = the
 * elements of class 0 .. 4 (class k = k boundaries at or below the row; scan_clu merges classes 1 .. nsb - 1).
 * Returns 5, or -1 for arguments outside these bounds. */
int lk_clu_count_sim(uint32_t nrows, const uint16_t* rows, uint32_t n, const uint32_t* sb, uint32_t nsb, int use_sub,
                     uint32_t* cnt);

/* Drives the host DDSketch (lakeside_amd/csrc/ddsketch.cpp, dd::Sketch: the sketches of the metrics percentiles and the
 * assembly of the kernels' bins) with nothing restated.  Sketch A: accept over vals[0..n) in order, then add_bin over the
 * n_bins pairs (bins[i] = a kernel bin id of layout.hpp, below DD_NBINS; counts[i]); sketch B likewise from the m*
 * arguments; A.merge(B).  *rejected = the position of the first value accept refused (NaN, a magnitude beyond the
 * mapping's range), counted over vals then mvals, or -1: nothing after a refused value is fed and B is not merged.
 * Writes quantiles[i] = A.quantile(qs[i]), *total = A.count() and, where non-NULL, consts[0..8) = gamma, multiplier,
 * relative_accuracy, min_indexable, max_indexable, DD_BIAS, DD_HALF, DD_NBINS.  A.serialize() goes to out; returns its
 * length, -1 for a bin id outside the key space, -5 when cap is too small. */
long lk_dd_sim(const double* vals, size_t n, const uint32_t* bins, const double* counts, size_t n_bins,
               const double* mvals, size_t mn, const uint32_t* mbins, const double* mcounts, size_t mn_bins,
               const double* qs, size_t nq, double* quantiles, long* rejected, double* consts, double* total,
               uint8_t* out, size_t cap);

/* Plans the filter of a PushDownRequest as the evaluator does before it reads a segment (lakeside_amd/csrc/
 * filter_plan.cpp: the leaf loop of the shape gate, plan_filter, plan_truth); numeric_group_bys[0..n) are the groupBys
 * to take as columns stored as numbers (the evaluator learns them from the loaded files).  Writes a JSON object into out
 * (NUL-terminated): cols (the string columns' names), leaves ({col: string column or -1, op, index, k}), nums (the
 * numeric query columns), nleaves ({col, leaf, lo_incl, hi_incl, nan_pass}), prog (the postfix program's bytes), truth /
 * truth_x / truth_early / truth_late (32-bit words as hex text; bit T | F << L of a table = TRUE), vtab, vleaf,
 * vleaf_shape, early, late_mask, dev_of, lead.  Returns 0; a PlanError's code (LK_ERR_ARG -1, LK_ERR_UNSUPPORTED -2)
 * with its message in out; -5 when cap is too small for the plan.  Reads LK_NO_VLEAF / LK_NO_EARLY_FIRST as the
 * evaluator does. */
int lk_filter_plan_sim(const char* request_json, const char* const* numeric_group_bys, size_t n, char* out, size_t cap);

/* Numeric comparison leaves on a chart's value column (`value > 250`), as the fused kernels test them per passing row
 * (lakeside_amd/csrc/vleaf.hpp, vleaf_pass over QParams::vl / vtab as the evaluator fills them).  Plans the request as
 * the evaluator does before it reads a segment -- the shape's aggregate and leaf loop, the gate's rule for p<NN> / ces
 * charts (numeric leaves only as value leaves), plan_filter, plan_truth -- then tests the n values (valid[i] == 0: a NULL,
 * vals[i] ignored).  Returns 0 with *vleaf = the plan's vleaf (the value leaves are tested apart from the string
 * conjuncts) and, when it is 1, pass[i] = the value leaves' conjuncts are TRUE for value i (0 everywhere otherwise); or
 * a PlanError's code (the gate's LK_ERR_UNSUPPORTED -2 among them) with its message in msg (NUL-terminated; empty when
 * cap is too small).  Reads LK_NO_VLEAF as the evaluator does. */
int lk_vleaf_sim(const char* request_json, const uint8_t* valid, const double* vals, size_t n, int* vleaf,
                 uint8_t* pass, char* msg, size_t cap);

/* Numeric groupBys, the two rules the ranks of a distributed evaluation apply to agreed data (lakeside_amd/csrc/
 * numgroup_agree.cpp; the evaluator calls the same functions, sharded or not).
 * Classes.  A (groupBy column, glob) travels as 3 bytes per rank: a VARCHAR file, a BOOLEAN file, the largest value rank
 * of a numeric file (INT32 1 < INT64 2 < FLOAT 3 < DOUBLE 4; 0 none).  lk_numgroup_file_class writes the bytes of one
 * file's column (Parquet physical type; is_string: a VARCHAR column); a rank's bytes are the element-wise max over its
 * files.  lk_numgroup_classes_sim takes n_ranks x 3 bytes and returns 0 with *union_type = the glob's union_by_name type
 * as a Parquet physical type (BOOLEAN 0, INT32 1, INT64 2, FLOAT 4, DOUBLE 5, BYTE_ARRAY 6 for VARCHAR alone, -1 when no
 * file has the column), or the refused union: 1 VARCHAR with BOOLEAN / numeric files, 2 BOOLEAN with numeric files
 * (*union_type = -1); -1 (LK_ERR_ARG) for a rank byte above 4.
 * Values.  Per rank r, counts[r] entries (union type, canonical key: ex_kernels.hip tag_key) of one column, concatenated
 * in rank order.  Writes the sorted distinct JDBC getString texts, '\n'-separated and NUL-terminated, into out, and the
 * position of every entry's text into ids; returns the number of texts, -5 when cap is too small, or a PlanError's code
 * with its message in out. */
int lk_numgroup_file_class(int is_string, int ptype, uint8_t* out3);
int lk_numgroup_classes_sim(const uint8_t* classes, size_t n_ranks, int* union_type);
long lk_numgroup_values_sim(const int32_t* union_types, const uint64_t* keys, const size_t* counts, size_t n_ranks,
                            uint32_t* ids, char* out, size_t cap);

/* Tag-name queries (isTagQuery without a tagDataType; include/lakeside_gpu.h), the host-only rules
 * (lakeside_amd/csrc/tagnames.hpp, as the evaluator calls them).
 * lk_tagnames_gate_sim: what the call decides from the request and the globs' schemas alone.  schemas_json: per glob,
 * per readable file in list order, the file's columns in file order as [name, Parquet physical type].  dist != 0: the
 * call is lk_eval_pushdown_dist.  Returns 0 with {"unions": [the glob's union_by_name column order]} in out, or the
 * refusal's code (LK_ERR_ARG -1, LK_ERR_UNSUPPORTED -2) with its message in out; -5 when cap is too small.
 * lk_tagnames_rows_sim: the fold of the per-column first keys first[0..n) (all ones: the column has none) into the
 * emitted rows: keys[i] = the i-th distinct key ascending, row_of_col[k] = the row that carries column k as a tag
 * (0xffffffff: none).  Returns the rows, or -5 when they exceed cap. */
int lk_tagnames_gate_sim(const char* request_json, const char* schemas_json, int dist, char* out, size_t cap);
long lk_tagnames_rows_sim(const uint64_t* first, size_t n, uint64_t* keys, uint32_t* row_of_col, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
