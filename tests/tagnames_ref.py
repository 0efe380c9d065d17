"""CPU restatement of the worker's tag-name query (isTagQuery without a tagDataType) -- test infrastructure only.

Per glob (Commons.scala:343-462) the worker runs `SELECT * FROM (SELECT * FROM read_parquet([...], union_by_name=True)
WHERE <window>) WHERE <filter>` (BaseExpr.scala:231-235; no ORDER BY, no LIMIT).  With the union's first column the
timestamp (branch T) a row becomes DataPoint(getLong(1), getDouble(2) (NULL: 0.0), tags = the later columns whose
getString is non-NULL, non-empty and not "null") (Commons.toDataPoint), TagNameCompressionStage.eval drops the tags whose
name it has seen in this call and the row when none is left, and PushDownAggregatorStage passes the row through.

Two stand-ins where the reference is not reproducible: rows of a glob in file-list order and row order within a file
(DuckDB's preserve_insertion_order, assumed); one seen-set over the globs taken in request order.

The filter and the window are evaluated by oracle/dataexpr.py's filter evaluation, the text of a value by
oracle/exemplar.py's JDBC getString restatement (both imported, neither edited).
"""
from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle import dataexpr as dx
from oracle import exemplar as ex


class Refused(Exception):
    """A shape the engine answers with LK_ERR_UNSUPPORTED."""


def union_order(schemas: Sequence[Sequence[str]]) -> List[str]:
    """read_parquet(union_by_name=True): files in list order, each file's columns in their own order, a name's first
    appearance fixes its place."""
    u: List[str] = []
    for names in schemas:
        for n in names:
            if n not in u:
                u.append(n)
    return u


def _read_tables(paths, sources):
    import pyarrow as pa
    import pyarrow.parquet as pq
    return [pq.read_table(p if sources is None else pa.BufferReader(sources[i])) for i, p in enumerate(paths)]


def glob_pass_mask(pr: dx.PushDownRequest, seg_idx, paths, sources, union, types) -> np.ndarray:
    """Window and filter over the glob's rows in file-list order, through oracle/dataexpr.py (as oracle/exemplar.py)."""
    be = pr.baseExpr
    segs = [pr.segmentRequests[i] for i in seg_idx]
    nonexistent = dx.field_set(be) - set(union)
    leafcols = dx._leaf_columns(be.filter)
    if any(c not in types for c in set(leafcols) - nonexistent):
        return None                                                  # Binder Error -> empty glob
    start, end = min(s.startTs for s in segs), max(s.endTs for s in segs)
    numcols = sorted({l.k for l in dx._leaves(be.filter) if l.op in dx.NUMERIC_OPS} - nonexistent)
    if any(types.get(c) == "string" for c in numcols) or not dx._check_numeric_literals(be.filter, nonexistent):
        return None
    strings = sorted(set(leafcols) - nonexistent - set(numcols))
    _, nums, strs = dx._read_glob(paths, [dx.TIMESTAMP], strings, sources)
    strs.update(dx._read_numeric(paths, [c for c in numcols if c in types], sources))
    ts, tsv = nums[dx.TIMESTAMP]
    ts = ts.astype(np.int64)
    try:
        t, _ = dx._eval_filter(be.filter, strs, nonexistent, len(ts))
    except dx.GlobSqlError:
        return None
    return tsv & (ts >= start) & (ts < end) & t


def to_data_point(tb, cols, union, types, r: int) -> Tuple[int, float, Dict[str, str]]:
    """Commons.toDataPoint, branch T, for row r of one file's table (cols: its columns as Python lists)."""
    def cell(c):
        return cols[c][r] if c in cols else None
    ts = int(cell(union[0]))
    v = cell(union[1])
    value = 0.0 if v is None else (float(np.float32(v)) if ex._kind(tb.schema.field(union[1]).type) == "float" else float(v))
    tags: Dict[str, str] = {}
    for c in union[2:]:
        x = cell(c)
        if x is None:
            continue
        s = ex._text(x, ex._kind(tb.schema.field(c).type), types[c])
        if s != "null" and s != "":
            tags[c] = s
    return ts, value, tags


def evaluate(pr: dx.PushDownRequest, paths: Sequence[str], glob_size: int, sources=None, per_glob: bool = True):
    """The rows the engine returns: [(ts, value, tags, glob column, (glob, file position, row))], in return order."""
    seen: set = set()
    rows = []
    for gi, g in enumerate(dx.globs_of(pr, glob_size)):
        gpaths = [paths[i] for i in g]
        gsrc = None if sources is None else [sources[i] for i in g]
        try:
            tables = _read_tables(gpaths, gsrc)
        except Exception:
            continue                                                 # an unreadable file: the glob is empty
        union = union_order([t.column_names for t in tables])
        types: Dict[str, str] = {}
        for t in tables:
            for f in t.schema:
                types[f.name] = ex.union_type(types.get(f.name), ex._kind(f.type))
        if union[0] != dx.TIMESTAMP:
            raise Refused(f"first column {union[0]}")
        kinds = {ex._kind(t.schema.field(union[1]).type) for t in tables if union[1] in t.column_names}
        if len(kinds) != 1 or not kinds <= {"int32", "int64", "float", "double"}:
            raise Refused(f"second column {union[1]}: {sorted(kinds)}")
        mask = glob_pass_mask(pr, g, gpaths, gsrc, union, types)
        if mask is None:
            continue
        offs = np.cumsum([0] + [t.num_rows for t in tables])
        lists = [{c: t.column(c).to_pylist() for c in t.column_names} for t in tables]
        for gr in np.nonzero(mask)[0].tolist():                      # stand-in 1: file-list order, then row order
            f = int(np.searchsorted(offs, gr, side="right") - 1)
            r = gr - int(offs[f])
            ts, value, tags = to_data_point(tables[f], lists[f], union, types, r)
            # TagNameCompressionStage.eval (stand-in 2: one seen-set, globs in request order)
            fresh = {k: v for k, v in tags.items() if k not in seen}
            seen.update(tags)
            if fresh:
                rows.append((ts, value, fresh, gi if per_glob else 0, (gi, f, r)))
    rows.sort(key=lambda x: x[4])
    rows.sort(key=lambda x: x[0], reverse=pr.reverseSort)             # stable: ties keep (glob, file, row)
    return rows


def name_count(rows) -> int:
    return sum(len(r[2]) for r in rows)
