"""Files and requests of the value-leaf sketch tests (tests/test_gpu_sketch_vleaf.py, tests/test_gpu_sketch_vleaf_dist.py):
`p<NN>` and `ces` charts whose filter holds gt / ge / lt / le leaves on the chart's value column.

Every file holds one row group and one page per column of about 6,000 rows -- one tile of three 2,048-row sub-tiles, so in
scan_tiles two sub-tiles hand their first listed rows through `pend` and the third is drained after the loop -- with 16
names (1 row in 16 passes the sparse filter; the dense one lists every row, 512 per wave and sub-tile, which stream at
once) and a service column without NULLs (a late groupBy: the one-row-per-lane `issue_one` path).  Kinds:

  lean       no NULL, DOUBLE values of both signs and zeros: scan_lean's tiles (in a `ces` call)
  nulls      5 % NULL values, the others >= 0: scan_tiles; the NULLs are what `v >= 0` drops
  names70    70 names: the name dictionary is too large for scan_lean
  int64      an INT64 value column: the general row scan (ex_scan), whatever the leaf
  nonfinite  one NaN row and one +inf row, each under a name of its own"""
import json

import numpy as np

STEP = 300_000
GLOB = 2
SVC = "resource.service.name"
NUMCOL = "attr.n"
ROWS = 6000
SPARSE_NAME = "metric_03"
NAN_NAME, INF_NAME = "bad_nan", "bad_inf"
KINDS = ["lean", "nulls", "names70", "int64", "nonfinite"]


def write_file(path, kind, seed):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    rng = np.random.default_rng([41, seed])
    n = ROWS + 37 * seed
    ts = np.sort(synth.T0 + rng.integers(0, synth.HOUR, n))
    names = [f"metric_{k:02d}" for k in rng.integers(0, 70 if kind == "names70" else 16, n)]
    v = rng.lognormal(0.0, 2.0, n)
    if kind != "nulls":
        v *= np.where(rng.random(n) < 0.2, -1.0, 1.0)
    v[rng.random(n) < 0.03] = 0.0
    if kind == "int64":
        value = pa.array(np.rint(v * 4).astype(np.int64), pa.int64())
    elif kind == "nulls":
        value = pa.array(v, pa.float64(), mask=rng.random(n) < 0.05)
    else:
        if kind == "nonfinite":
            names[1700], v[1700] = NAN_NAME, np.nan
            names[4400], v[4400] = INF_NAME, np.inf
        value = pa.array(v, pa.float64())
    t = pa.table({
        dx.TIMESTAMP: pa.array(ts, pa.int64()),
        dx.VALUE: value,
        dx.NAME: pa.array(names, pa.string()),
        SVC: pa.array([f"svc-{k}" for k in rng.integers(0, 5, n)], pa.string()),
        NUMCOL: pa.array(rng.integers(0, 9, n), pa.int64()),
    })
    strings = [dx.NAME, SVC]
    pq.write_table(t, str(path), compression="NONE", use_dictionary=strings, row_group_size=1 << 16, data_page_size=1 << 22,
                   column_encoding={c: "PLAIN" for c in t.column_names if c not in strings})
    return str(path)


def write_files(root):
    """{kind: path}"""
    return {k: write_file(root / f"vleaf_{k}.parquet", k, i) for i, k in enumerate(KINDS)}


def num(op, x, k=None, dt="number"):
    from oracle import dataexpr as dx
    return {"k": k or dx.VALUE, "v": [x], "op": op, "extracted": False, "computed": False, "dataType": dt}


# the value conjuncts of the requests: v > x; x < v <= y (two conjuncts); not (v >= x); v < a or v > b (one conjunct)
VALUE_FILTERS = {
    "gt": [num("gt", "1.5")],
    "between": [num("gt", "0.5"), num("le", "20")],
    "not_ge": [{"not": num("ge", "2")}],
    "lt_or_gt": [{"op": "or", "q1": num("lt", "0.25"), "q2": num("gt", "3e1")}],
}


def name_filter(which):
    from lakeside_amd import synth
    return synth.leaf(synth.NAME, "eq", SPARSE_NAME) if which == "sparse" else synth.leaf(synth.NAME, "regex", "^metric_")


def and_all(parts):
    q = parts[-1]
    for p in reversed(parts[:-1]):
        q = {"op": "and", "q1": p, "q2": q}
    return q


def request(filt, agg, gbs, nsegs, dataset="logs"):
    from lakeside_amd import synth
    segs = [synth.segment_request(i, step=STEP, hour=0, dataset=dataset) for i in range(nsegs)]
    d = synth.pushdown(filt, segs, agg, list(gbs), dataset=dataset)
    if agg[0] == "p":
        d["baseExpr"]["chart"]["rollup"] = agg
    return json.dumps(d)


def pct_rows(res, glob=None):
    return [(int(res.ts[r]), res.tags[r], float(res.values[r]), res.sketch(r)) for r in range(len(res))
            if glob is None or int(res.globs[r]) == glob]
