"""Expected rows of a chart grouped by a numeric column, built from the oracle without changing it.

BaseExpr.getChartSql groups by the column as it is (`GROUP BY step_ts, "<col>", name`, BaseExpr.scala:338-346, 401-403)
and Commons.toDataPoint prints each group value with JDBC getString (Commons.scala:430-437).  oracle/dataexpr.py reads a
groupBy column's raw Python values and ignores the glob's union_by_name type, so the expectation is the oracle's over a
*twin* of every input file: each numeric groupBy column replaced by a VARCHAR column holding
`dx.numeric_tag_text(kinds of the glob, value)` -- the text DuckDB's group of that value prints under the glob's union
type (INTEGER < BIGINT < FLOAT < DOUBLE, integers cast to the float type first; BOOLEAN alone; every NaN one group;
-0.0 as 0.0) -- with NULL left NULL.  Grouping by that text is grouping by value, and the request stays unchanged.
tests/test_numgroup_ref_cpu.py pins the helper against the reference's own SQL on SQLite.
"""
import os

from oracle import dataexpr as dx


def glob_kinds(tables, column):
    """The numeric kinds (dx._tag_kind) of `column` over one glob's tables; empty: no file has it."""
    return {dx._tag_kind(t.schema.field(column).type) for t in tables if column in t.column_names}


def write_twins(paths, columns, glob_size, out_dir):
    """Twin of every file with each column of `columns` that is numeric in its glob rewritten as VARCHAR text; returns
    the twin paths (same order)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    os.makedirs(out_dir, exist_ok=True)
    tables = [pq.read_table(p) for p in paths]
    twins = []
    for g0 in range(0, len(paths), glob_size):
        glob = range(g0, min(len(paths), g0 + glob_size))
        for column in columns:
            kinds = glob_kinds([tables[i] for i in glob], column)
            if not kinds or kinds == {"text"}:
                continue
            if "text" in kinds or ("bool" in kinds and len(kinds) > 1):
                raise NotImplementedError(f"column {column}: union of {sorted(kinds)} in one glob")
            for i in glob:
                t = tables[i]
                if column not in t.column_names:
                    continue
                text = [dx.numeric_tag_text(kinds, v) for v in t.column(column).to_pylist()]
                tables[i] = t.set_column(t.column_names.index(column), column, pa.array(text, pa.string()))
    for i, t in enumerate(tables):
        path = os.path.join(out_dir, f"twin_{i}_" + os.path.basename(paths[i]))
        pq.write_table(t, path)
        twins.append(path)
    return twins


def distinct_texts(twins, column):
    """The distinct non-NULL texts of `column` over the twins (every row, no filter)."""
    import pyarrow.parquet as pq
    out = set()
    for p in twins:
        t = pq.read_table(p, columns=None)
        if column in t.column_names:
            out |= {v for v in t.column(column).to_pylist() if v is not None}
    return out
