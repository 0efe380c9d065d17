"""Expected rows of a field chart (chart.fieldName / fieldType), built from the oracle without changing it.

oracle/dataexpr.py refuses field charts, so the expectation restates the SQL (BaseExpr.getChartSql,
BaseExpr.scala:319-405)

    SELECT <step_ts>, <agg>(try_cast(<fieldName>$<fieldType> as double)) [/ 1000000 | / 1000], name <, groupBys>
    FROM (..window..) WHERE <fieldName>$<fieldType> IS NOT NULL AND <filter> GROUP BY ..

as the value chart the oracle does evaluate, over a *twin* of every input file: the rows whose field is NULL removed
(the IS NOT NULL conjunct) and `_cardinalhq.value` replaced by the double the SQL aggregates -- the numeric cast, the
parsed text, or NULL for text that casts to NULL.  A file without the column becomes a file with no rows
(union_by_name: NULL for all of them); a glob none of whose files has the column is a Binder Error, i.e. empty
(Commons.scala:249-253).  The divisor (duration: 1e6, datasize: 1e3) is applied to the finalized values.
"""
import json
import os
import re

import numpy as np

from oracle import dataexpr as dx

NUMBER = re.compile(r"-?[0-9]+(\.[0-9]+)?([eE][-+]?[0-9]+)?")
SCALE = {"duration": 1e6, "datasize": 1e3}


def text_value(s):
    """The two classes of text a field chart answers: a plain number -> its double; a first byte that is an ASCII
    letter other than i I n N -> None (try_cast gives NULL).  Anything else has no expectation here."""
    if NUMBER.fullmatch(s):
        v = float(s)
        if np.isfinite(v):
            return v
    elif s and s[0].isascii() and s[0].isalpha() and s[0] not in "iInN":
        return None
    raise ValueError(f"text {s!r} is outside the two classes a field chart evaluates")


def _kind(typ):
    import pyarrow as pa
    if pa.types.is_dictionary(typ):
        typ = typ.value_type
    if pa.types.is_integer(typ):
        return "int"
    if pa.types.is_float32(typ):
        return "float32"
    if pa.types.is_float64(typ):
        return "float64"
    if pa.types.is_string(typ) or pa.types.is_large_string(typ):
        return "text"
    raise NotImplementedError(f"chart field of type {typ}")


def _field_doubles(arr, kind, via_f32):
    """(keep, values, valid) of one file's field column: rows with a field, their doubles, which doubles are not NULL."""
    import pyarrow as pa
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    if pa.types.is_dictionary(arr.type):
        arr = arr.cast(arr.type.value_type)
    keep = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
    if kind == "text":
        vals = [text_value(s) for s in arr.filter(pa.array(keep)).to_pylist()]
        valid = np.array([v is not None for v in vals], dtype=bool)
        return keep, np.array([0.0 if v is None else v for v in vals], dtype=np.float64), valid
    a = arr.filter(pa.array(keep)).to_numpy(zero_copy_only=False)
    if via_f32:   # an integer file of a glob whose union type is FLOAT is cast to FLOAT first
        a = a.astype(np.float32)
    return keep, a.astype(np.float64), np.ones(len(a), dtype=bool)


def write_twins(paths, column, glob_size, out_dir):
    """Twin of every file for chart field `column`; returns (twin paths, per glob: some file has the column)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    os.makedirs(out_dir, exist_ok=True)
    tables = [pq.read_table(p) for p in paths]
    twins, has = [], []
    for g0 in range(0, len(paths), glob_size):
        glob = range(g0, min(len(paths), g0 + glob_size))
        kinds = {_kind(tables[i].schema.field(column).type) for i in glob if column in tables[i].column_names}
        has.append(bool(kinds))
        if "text" in kinds and len(kinds) > 1:
            raise NotImplementedError("numeric and VARCHAR files of the chart field in one glob")
        via_f32 = "float32" in kinds and "float64" not in kinds
        for i in glob:
            t = tables[i]
            vi = t.column_names.index(dx.VALUE)
            if column in t.column_names:
                kind = _kind(t.schema.field(column).type)
                keep, vals, valid = _field_doubles(t.column(column), kind, via_f32 and kind == "int")
                t = t.filter(pa.array(keep))
                t = t.set_column(vi, dx.VALUE, pa.array(vals, pa.float64(), mask=~valid))
            else:
                t = t.slice(0, 0)
                t = t.set_column(vi, dx.VALUE, pa.array([], pa.float64()))
            path = os.path.join(out_dir, f"twin_{i}_" + os.path.basename(paths[i]))
            pq.write_table(t, path)
            twins.append(path)
    return twins, has


def value_request(req):
    """The request without its chart field: (JSON text, column, divisor or None)."""
    r = json.loads(req) if isinstance(req, str) else json.loads(json.dumps(req))
    chart = r["baseExpr"]["chart"]
    name, typ = chart.pop("fieldName"), chart.pop("fieldType")
    return json.dumps(r), f"{name}${typ}", SCALE.get(typ)


def expected_cells(req, paths, glob_size, out_dir):
    """(parsed value request, per-glob oracle cells over the twins, divisor).  The cells carry their raw values, so one
    call serves every aggregate of the same filter, groupBys and field."""
    vreq, column, scale = value_request(req)
    twins, has = write_twins(paths, column, glob_size, out_dir)
    pr = dx.parse_pushdown(vreq)
    cells = dx.evaluate_glob_cells(pr, glob_size, twins)
    return pr, [cs if h else [] for cs, h in zip(cells, has)], scale


def _with_agg(pr, agg):
    import copy
    pr = copy.deepcopy(pr)
    pr.baseExpr.chart.aggregation = agg
    return pr


def per_glob_rows(pr, cells, scale, agg):
    div = (lambda v: v / scale) if scale else (lambda v: v)
    return [[(c.ts, div(c.agg_value(agg)), c.tags) for c in cs] for cs in cells]


def merged_rows(pr, cells, scale, agg):
    div = (lambda v: v / scale) if scale else (lambda v: v)
    return [(ts, div(v), tags) for ts, v, tags in dx.merge_glob_cells(_with_agg(pr, agg), cells)]
