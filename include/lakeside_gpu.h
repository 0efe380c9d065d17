/* lakeside_gpu.h — C ABI of the MI355X sealed-segment DataExpr evaluator.
 *
 * Drop-in for the worker's per-segment evaluator seam:
 *   Commons.evaluatePushDownRequest(queryId, localParquet, pushDownRequest)
 *     core/src/main/scala/com/cardinal/utils/Commons.scala:343-397
 *   whose native seam is Commons.toGlobResultSet + resultSetToSource (Commons.scala:200-254, 280-341),
 *   i.e. DuckDB's read_parquet + filter + hash GROUP BY + ORDER BY behind JDBC/JNI.
 * The Scala side binds these symbols through JNA exactly as the reference already binds lib-trigram.so
 * (core/src/main/scala/com/cardinal/utils/ast/queries/NLPUtils.scala:43-52); see INTEGRATION.md.
 *
 * Conventions: 0 = success, negative = error (message in lk_last_error(), thread-local).  Never throws or
 * aborts across the ABI.  Inputs are borrowed for the duration of the call.  Results are owned by the
 * library until lk_result_free.  Calls on one engine are thread-safe and re-entrant: each evaluation leases its
 * own context (HIP stream, workspaces; up to "max_calls" in flight), so calls from several threads run
 * concurrently, as the worker's glob queries do (Commons.scala:371-372); only distributed calls
 * (lk_eval_pushdown_dist, lk_eval_formula_dist) are serialised, to keep every rank's collectives in one order, and a dictionary
 * compaction (see lk_engine_create) runs between loads / evaluations, never under one.
 *
 * Errors: a failure that belongs to one glob's DuckDB query in the reference -- a missing or unreadable segment,
 * corrupt Parquet, a column type the query cannot bind, a regex RE2 rejects -- empties that glob only
 * (Commons.toGlobResultSet, Commons.scala:249-253); the call still succeeds ("failed_globs" in lk_result_stats).
 */
#ifndef LAKESIDE_GPU_H
#define LAKESIDE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lk_engine lk_engine;   /* one per process per GPU: device, streams, HBM segment cache, RCCL comm */
typedef struct lk_result lk_result;   /* rows of one evaluation */

enum {
  LK_OK = 0,
  LK_ERR_ARG = -1,          /* bad argument / malformed JSON */
  LK_ERR_UNSUPPORTED = -2,  /* query or file shape outside the implemented path */
  LK_ERR_IO = -3,           /* file read / Parquet parse */
  LK_ERR_DEVICE = -4,       /* HIP / RCCL failure, or no GPU */
  LK_ERR_MEMORY = -5,
  LK_ERR_EVICTED = -6       /* a key registered with lk_segment_put was evicted from the HBM cache: re-put it */
};

/* Flags of lk_eval_pushdown. */
#define LK_PER_GLOB_ROWS 1u   /* rows of every glob separately (the worker's output, S17) */
#define LK_MERGED 2u          /* cells merged across globs as query-api does (TimeGroupedSketchAggregator, S19) */
#define LK_PLAN_BYTES 4u      /* optional, with either: the scan kernel counts the bytes its plan reads
                                 (lk_result_stats "plan_bytes"; measurement only, costs ~5% of scan time) */

/* options_json: {"device": 0, "hbm_budget_bytes": N, "max_calls": 4, "dict_compact_min_dead": 1024,
 *                "load_threads": 0, "formula_dense_max_cells": 4194304, "formula_hash_slots": 0,
 *                "cluster_values": true}; NULL = defaults.
 * hbm_budget_bytes: weight bound of the HBM segment cache (the worker's Caffeine cache weight,
 * query-worker/.../WorkerApi.scala:53-64): inserting past it evicts least-recently-used segments; 0 (default) = no
 * bound, eviction only when HBM runs out.  max_calls: evaluations in flight (one stream each).
 * dict_compact_min_dead: engine dictionaries (one per column, value -> id) count the cached segments' references to
 * every id; once evictions leave at least max(live ids, this) ids unreferenced, the next load or evaluation renumbers
 * the live ids densely first, so group-dim spaces track the cached segments (results keep their strings).
 * load_threads: host threads of a segment load (page walk, decompression, staging copies); 0 (default) = the
 * process's OMP_NUM_THREADS share of the host's cores, at most 16.
 * cluster_values: a load also keeps, per tile, a copy of `_cardinalhq.value` grouped by `_cardinalhq.name` code (10 B
 * per row of eligible tiles and 32 B of aggregates per (tile, name code), counted in the cache weight), which
 * name-filtered SUM / MIN / MAX / AVG queries stream -- or, for tiles inside one time bucket, merge from the aggregates
 * -- instead of gathering values row by row, and from whose per-code element ranges name-filtered COUNT queries take
 * their counts without reading a value (AVG is the sum with those counts); false = no copy, for deployments that prefer
 * the cache capacity.
 * cluster_samples (default true): a load also keeps, per tile of a segment whose timestamps are sorted, the 256
 * timestamps that the search for a tile's bucket boundaries samples (2 KB per tile, counted in the cache weight, with
 * or without cluster_values); false = no tables, the search reads the timestamp column.
 * Replaces DuckDbConnectionFactory (core/.../utils/DuckDbConnectionFactory.scala:76-114). */
int lk_engine_create(const char* options_json, lk_engine** out);
void lk_engine_destroy(lk_engine* e);

/* HBM segment cache (replaces the worker's Caffeine disk cache, worker/WorkerApi.scala:53-77).
 * lk_segment_put: register Parquet bytes under `key` (e.g. the path Commons.toParquetFilePath builds,
 * Commons.scala:256-278) and upload them; lk_segment_load: read a local Parquet file into the cache.
 * Re-putting an existing key replaces it. */
int lk_segment_put(lk_engine* e, const char* key, const uint8_t* data, size_t size);
int lk_segment_load(lk_engine* e, const char* path);
int lk_segment_evict(lk_engine* e, const char* key);
size_t lk_segment_count(const lk_engine* e);
/* HBM bytes held by the cache. */
size_t lk_segment_bytes(const lk_engine* e);
/* Engine counters as JSON: {"segments", "segment_bytes", "clu_bytes" (the clustered value copies' share),
 * "clu_alloc_failed" (loads whose copy could not be allocated: those segments serve the other kernels), "evictions",
 * "dict_compactions",
 * "dictionaries": {column: {"size", "live", "generation"}}}; valid until the calling thread's next call. */
const char* lk_engine_stats(lk_engine* e);
/* Drops the engine's per-query caches -- parsed requests, per-(column, leaf) dictionary outcomes, value-key orders,
 * bulk-export pointer tables and distributed group-dim unions -- but keeps the cached segments and dictionaries: the
 * next evaluation of any request runs cold (the bench's cold_eval_ms).  Waits for in-flight evaluations. */
int lk_engine_drop_caches(lk_engine* e);

/* Mirrors one Commons.evaluatePushDownRequest call (Commons.scala:343-397).
 * push_down_json: PushDownRequest.toJson wire format (core/.../model/SegmentRequest.scala:30-60).
 * paths[i]: cache key (or local file, loaded on a miss) of segmentRequests[i].
 * glob_size: 10 for local Parquet, 5 for remote (Commons.scala:361); 0 = 10.
 * flags: LK_PER_GLOB_ROWS or LK_MERGED.
 * Numeric comparison leaves (gt / ge / lt / le) in a `p<NN>` or `ces` chart are evaluated when every one of them reads
 * the chart's value column and sits in a conjunct of numeric leaves only (at most 5 of them, 6 leaves in all): "p99 of
 * the requests slower than 250 ms".  A row whose value is NULL then fails the filter, and a NaN or infinite value the
 * leaves drop does not reach the sketch.  Any other numeric leaf in such a chart -- on another column, in a conjunct
 * with string leaves, beside a groupBy over a column stored as a number, or under `ces` over metrics -- is
 * LK_ERR_UNSUPPORTED ("numeric comparison leaves in sketch queries"), decided from the request before a segment is
 * read (the groupBy case: from the loaded files' schemas; in lk_eval_pushdown_dist on every rank alike).
 * Tag-name queries -- isTagQuery without a tagDataType, no chart, processor.tagNameCompressionEnabled = true (what
 * POST /api/v1/tags/{dataset} without a tagName sends, QueryEngineV2.scala:419-491) -- return every tag name once: the
 * worker's SELECT * rows (Commons.scala:428-459) after TagNameCompressionStage.  A glob's union schema (files in list
 * order, columns in file order, first appearance fixes the place) must start with "_cardinalhq.timestamp"; a row is
 * (timestamp, getDouble of the union's second column with NULL as 0.0, tags = the later columns whose text is non-NULL,
 * non-empty and not "null"), and a tag is kept only on the first row of the call that carries its name.  Two
 * deterministic stand-ins replace what the reference leaves to timing: rows of a glob count in file-list order and, within
 * a file, in row order (DuckDB's default preserve_insertion_order; assumed), and the seen-set the reference shares among
 * concurrently running globs sees the globs in request order.  Rows come back in ascending timestamp order (descending
 * under reverseSort), ties by glob, file position and row; LK_PER_GLOB_ROWS and LK_MERGED return the same rows, the
 * glob column being the row's glob or 0.  Tags are per row: lk_result_tag_value answers NULL for a column that is not
 * among the row's new names, lk_result_group_ids returns NULL and lk_result_num_group_columns 0.  lk_result_stats
 * carries "tag_names": {"columns", "found", "rows", "tiles_walked", "tiles_pruned"}.  LK_ERR_UNSUPPORTED, the message
 * beginning "tag queries without a tagDataType: ": processor.tagNameCompressionEnabled absent or false (the reference
 * then streams every passing row), processor.resetValueToField, extract / compute, a chart, a glob whose first column
 * is not the timestamp (the reference emits such rows whole under the wall clock), a second column that is VARCHAR /
 * BOOLEAN or of different numeric types in one glob, and lk_eval_pushdown_dist; a column of the files that is not loaded
 * fails the call as any referenced unloaded column does. */
int lk_eval_pushdown(lk_engine* e, const char* push_down_json, const char* const* paths, size_t n_paths,
                     int glob_size, unsigned flags, lk_result** out);

/* QueryEngineV2.evaluateFormula for one SegmentGroup (query-api/.../engine/QueryEngineV2.scala:310-389): arithmetic
 * over several base expressions, e.g. an error rate a / b * 100, joined per (timestamp, group key) on the device.
 * formula_json: {"formula": "a / b * 100",
 *                "expressions": {"a": {"pushDown": <PushDownRequest, as lk_eval_pushdown takes>, "paths": [..]},
 *                                "b": {...}}}
 * Only the expressions the formula references are evaluated; a formula without a variable (5 + 3) gives LK_OK and no
 * rows.  Rows: merged, ascending timestamp (order within one timestamp unspecified); value = the formula's value; tags =
 * those of the row the value takes its tags from (Formula.scala:32-69: e1's, e2's where an addition filled e1; a constant
 * has none without groupBys).  The tag columns are the union of the referenced expressions' tag columns in order of
 * first appearance; a row with empty tags answers NULL in every column.  lk_result_globs is all zeros.  The bulk tag
 * export does not apply to formula results: lk_result_group_ids returns NULL and lk_result_num_group_columns 0 -- read
 * tags with lk_result_tag_value.  lk_result_stats carries "formula": {"mode": "dense"|"hash", "cells", "operands_on_device",
 * "operands_uploaded", "regrows", "world", "rank", "operands"} (the last three: see lk_eval_formula_dist).
 * LK_ERR_ARG: malformed formula (unknown variable, unbalanced parentheses, a single term), expressions with different
 * steps.  LK_ERR_UNSUPPORTED (the message names the rule): `^`, relational operators, unary signs; expressions whose
 * groupBy sets differ; an expression without a chart, a tag query, extract / compute, metrics percentiles.
 * Engine options: cell spaces (buckets x union groups) up to "formula_dense_max_cells" use a dense cell table, larger
 * ones a hash table of "formula_hash_slots" slots to begin with (0: sized from the operands' rows) that regrows when full. */
int lk_eval_formula(lk_engine* e, const char* formula_json, int glob_size, lk_result** out);

size_t lk_result_num_rows(const lk_result* r);
const int64_t* lk_result_timestamps(const lk_result* r);   /* ascending (ties: glob, then group order) */
const double* lk_result_values(const lk_result* r);
const uint32_t* lk_result_globs(const lk_result* r);       /* glob index per row (0 when merged) */
size_t lk_result_num_tag_columns(const lk_result* r);
const char* lk_result_tag_name(const lk_result* r, size_t col);             /* "name", groupBys, queryTags keys */
const char* lk_result_tag_value(const lk_result* r, size_t row, size_t col); /* NULL => tag absent (S15) */
/* Percentile aggregations (`p<NN>`, logs/traces): the row's serialized DDSketch (sketches-java DDSketch.serialize
 * wire format, the `Left(bytes)` of SketchTags, PushDownAggregatorStage.scala:163-167; relative accuracy 0.01); the
 * row's value is getValueAtQuantile(NN / 100) of that sketch (BaseExpr.scala:59-61).  *len = 0 / NULL for other
 * aggregations.  Valid until lk_result_free. */
const uint8_t* lk_result_sketch(const lk_result* r, size_t row, size_t* len);
/* Bulk tag export (replaces one lk_result_tag_value call per row and column; the reference materializes tags per
 * row in Commons.toDataPoint, Commons.scala:399-462).  The name / groupBy tag columns are the first
 * lk_result_num_group_columns columns.  Row r's value in such a column `col` is
 *     dict[(lk_result_group_ids(r)[row] / stride) % ndim]       (NULL: the tag is absent, S15)
 * with dict = lk_result_tag_dictionary(r, col, &stride, &ndim).  NULL dictionary (ndim 0): the column yields no
 * tag (a hidden tag).  A row whose group tags are all absent takes its glob's queryTags (Commons.scala:450-452):
 * lk_result_tag_value on the columns after the group columns.  Arrays are valid until lk_result_free; an
 * engine-dictionary column's table is shared with the engine and costs O(1) once built. */
const uint32_t* lk_result_group_ids(const lk_result* r);
size_t lk_result_num_group_columns(const lk_result* r);
const char* const* lk_result_tag_dictionary(const lk_result* r, size_t col, uint64_t* stride, uint64_t* ndim);
/* JSON: {"scan_ms":..,"total_ms":..,"rows_scanned":..,"algorithmic_bytes":..,"tiles":..,"cells":..,
 *        "failed_globs":..,"general_segments":..} */
const char* lk_result_stats(const lk_result* r);
void lk_result_free(lk_result* r);

const char* lk_last_error(void);

/* ---- multi-GPU (one process per GPU; segments sharded across ranks, partial tables merged over RCCL) ----
 * Replaces the pod fan-out + query-api merge: SegmentSequencer.allSources (query-api/.../engine/
 * SegmentSequencer.scala:53-160), QueryEngineV2.mergeSortedSource (QueryEngineV2.scala:76-97) and
 * TimeGroupedSketchAggregator (core/.../eval/TimeGroupedSketchAggregator.scala:57-177). */
#define LK_UNIQUE_ID_BYTES 128
/* Fill `id` (LK_UNIQUE_ID_BYTES) on rank 0; broadcast it out of band (e.g. torch.distributed). */
int lk_comm_unique_id(uint8_t* id);
int lk_comm_init(lk_engine* e, const uint8_t* id, int world, int rank);
/* Host transport instead of RCCL (e.g. torch.distributed/gloo or MPI supplied by the caller; also lets several
 * ranks share one GPU, which RCCL refuses).  fn(user, send, bytes, recv) must all-gather `bytes` from every rank
 * into recv (world * bytes, rank order) and return 0; it is called from inside lk_eval_pushdown_dist, on the
 * calling thread, the same number of times with the same sizes on every rank. */
typedef int (*lk_allgather_fn)(void* user, const void* send, size_t bytes, void* recv);
int lk_comm_init_host(lk_engine* e, int world, int rank, lk_allgather_fn fn, void* user);
/* Like lk_eval_pushdown with LK_MERGED, but this rank evaluates only the segments whose index i has
 * shard[i] == rank; partial tables are reduced to rank 0 over RCCL, which alone receives rows
 * (other ranks get an empty result). shard == NULL: i % world. */
int lk_eval_pushdown_dist(lk_engine* e, const char* push_down_json, const char* const* paths, size_t n_paths,
                          const int32_t* shard, int glob_size, lk_result** out);
/* lk_eval_formula with a rank per pod: replaces query-api's fan-out of every base expression of a formula to the pods,
 * the merge of their streams (mergeSortedSource / TimeGroupedSketchAggregator) and Formula.eval over the merged sides
 * (QueryEngineV2.evaluateFormula, query-api/.../engine/QueryEngineV2.scala:310-389; Formula.scala:32-69).
 * formula_json: what lk_eval_formula takes; an expression may carry "shard": [..], one rank per path with the meaning
 * of lk_eval_pushdown_dist's shard (absent: i % world).  A shard of the wrong length or a rank outside [0, world) is
 * LK_ERR_ARG, decided -- like every refusal lk_eval_formula makes from the request -- before any collective, so every
 * rank must pass the same formula, the same variable names and the same pushDowns.  Each referenced expression is one
 * sharded merged evaluation (every rank takes part in each, in ascending byte order of the variable names) whose rows
 * land on rank 0 and stay on its device; rank 0 joins them and returns what lk_eval_formula returns over all the paths
 * (rows, tag columns, lk_result_globs all zero, no bulk export).  Every other rank gets LK_OK and an empty result that
 * still carries stats.  A failure of one expression fails the call on every rank at that expression.
 * lk_result_stats' "formula" also carries "world", "rank" and "operands": [{"var", "reduce", "rows", "kept"}] in
 * evaluation order (as lk_eval_formula's does, with world 1).  Without lk_comm_init*: LK_ERR_ARG. */
int lk_eval_formula_dist(lk_engine* e, const char* formula_json, int glob_size, lk_result** out);

#ifdef __cplusplus
}
#endif
#endif /* LAKESIDE_GPU_H */
