"""Parquet files for the numeric groupBy tests: a `status` column of every numeric class, written as
tests/golden/make_fixtures.py writes its files (small row groups and pages, dictionaries on strings only), so a file
spans several pages and tiles and the definition-level prefix carries across the row scan's 256-row steps."""
import numpy as np

STATUS = "status"
RATIO = "ratio"
SVC = "resource.service.name"
OTHER = "attr.n"
LAT = "lat$number"
NAN = float("nan")

# file kind -> (arrow type name, values)
KINDS = {
    "A": ("int64", [200, 404, 500, -1, 2 ** 53 + 1, 2 ** 62, -2 ** 63]),
    "B": ("float64", [200.0, 0.0, -0.0, NAN, 1e23, 2.0 ** 53, 0.1]),
    "Bfinite": ("float64", [200.0, 0.0, -0.0, 1e23, 2.0 ** 53, 0.1]),
    "C": ("float32", [200.0, float(np.float32(0.1)), 2.0 ** 24, NAN, -0.0]),
    "D": ("int32", [200, 404, -1, 2 ** 24 + 1]),
    "E": ("bool", [True, False]),
    "F": (None, None),                 # no status column
    "G": ("int64", None),              # all NULL
    "V": ("string", ["200", "404", "ok"]),
}


def status_array(kind, n, rng, null_frac=0.1, values=None):
    import pyarrow as pa
    typ, vals = KINDS[kind] if values is None else ("int64", values)
    if typ is None:
        return None
    atype = {"int64": pa.int64(), "int32": pa.int32(), "float64": pa.float64(), "float32": pa.float32(),
             "bool": pa.bool_(), "string": pa.string()}[typ]
    if vals is None:
        return pa.array([None] * n, atype)
    pick = rng.integers(0, len(vals), n)
    mask = rng.random(n) < null_frac
    return pa.array([vals[k] for k in pick.tolist()], atype, mask=mask)


def write_file(path, kind, seed, rows=2500, null_frac=0.1, values=None, row_group_size=2048, metrics=False):
    """One file of `rows` rows over hour 0: timestamp, value, name (4 values), service, status (by kind), a DOUBLE
    `ratio`, another INT64 column, a DOUBLE chart field; `metrics`: timestamps on the 60 s grid and rollup_max."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    rng = np.random.default_rng(seed)
    n = rows
    ts = synth.T0 + (60_000 * rng.integers(0, 60, n) if metrics else rng.integers(0, synth.HOUR, n))
    v = np.round(rng.normal(0, 100, n), 3)
    cols = {
        dx.TIMESTAMP: pa.array(np.sort(ts), pa.int64()),
        ("rollup_max" if metrics else dx.VALUE): pa.array(v, pa.float64(), mask=rng.random(n) < 0.03),
        dx.NAME: pa.array([f"metric_{k:02d}" for k in rng.integers(0, 4, n)], pa.string()),
        SVC: pa.array([f"svc-{k}" for k in rng.integers(0, 4, n)], pa.string(), mask=rng.random(n) < 0.1),
        RATIO: pa.array([[0.25, 0.5, NAN, -0.0, 1e-3][k] for k in rng.integers(0, 5, n)], pa.float64(),
                        mask=rng.random(n) < 0.1),
        OTHER: pa.array(rng.integers(0, 1000, n), pa.int64()),
        LAT: pa.array(rng.lognormal(0, 2, n), pa.float64(), mask=rng.random(n) < 0.05),
    }
    st = status_array(kind, n, rng, null_frac, values)
    if st is not None:
        cols[STATUS] = st
    t = pa.table(cols)
    strings = [c for c in t.column_names if t.schema.field(c).type == pa.string()]
    pq.write_table(t, str(path), compression="NONE", use_dictionary=strings, row_group_size=row_group_size,
                   data_page_size=4096, column_encoding={c: "PLAIN" for c in t.column_names if c not in strings})
    return str(path)
