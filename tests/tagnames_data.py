"""Parquet files for the tag-name queries (isTagQuery without a tagDataType): timestamp first, a value column second,
then probe columns named for the case each one makes.  Written with pyarrow; shared by the CPU and the GPU tests.

Every file has 900 rows in three row groups of 300 (`row_group_size=300`): with one page per column chunk a tile is one
row group -- one 256-row kernel step plus 44 rows, ending inside a ballot word.  Two globs of two files (glob_size 2).
`attr.keep` makes rows i % 3 == 0 fail the keep filter ("no") and rows i % 7 == 0 NULL (UNKNOWN: dropped).
"""
import os

import numpy as np

from lakeside_amd import synth

ROWS = 900
RG = 300
NFILES = 4
GLOB_SIZE = 2
TS = "_cardinalhq.timestamp"
VALUE = "_cardinalhq.value"
KEEP = "attr.keep"
FROM_ROWS = (0, 63, 64, 255, 256, 299, 300)   # p.row<R>: NULL before row R of every file, a value from R on
NUM_FROM = {"n.i32": 70, "n.i64": 130, "n.f32": 258, "n.f64": 10, "n.bool": 301}

KEEP_FILTER = synth.leaf(KEEP, "eq", "yes")
FILTERS = {
    "keep": KEEP_FILTER,
    "pass_all": synth.leaf("plain.full", "exists"),              # IS NOT NULL over a column without NULLs
    "pass_none": synth.leaf(KEEP, "eq", "nobody"),
    "nonexistent": synth.leaf("no.such.field", "eq", "x"),       # a field absent from the glob: false
    "numeric_gt": {"k": "n.rowno", "v": ["449.5"], "op": "gt", "extracted": False, "computed": False, "dataType": "number"},
    "regex": synth.leaf(KEEP, "regex", "^y.s$"),
}


def timestamps(f: int) -> np.ndarray:
    """Unsorted within the file; rows i % 50 == 7 lie outside the window; rows 120 / 121 tie across files."""
    i = np.arange(ROWS, dtype=np.int64)
    ts = synth.T0 + ((i * 37 + f * 11) % ROWS) * 1000 + f
    ts[(i == 120) | (i == 121)] = synth.T0 + 123_456
    out = i % 50 == 7
    ts[out] = np.where(i[out] % 100 == 7, synth.T0 - 5 - i[out], synth.T0 + synth.HOUR + i[out])
    return ts


def _strings(vals):
    import pyarrow as pa
    return pa.array(vals, pa.string())


def table(f: int, int_value: bool):
    """File f (0, 1: glob 0; 2, 3: glob 1) of a flavour."""
    import pyarrow as pa
    i = np.arange(ROWS)
    glob, pos = f // GLOB_SIZE, f % GLOB_SIZE
    cols = {TS: pa.array(timestamps(f), pa.int64())}
    vnull = (i == 1) | (i == 64) | (i % 11 == 5)              # NULL on emitted rows (1, 64): getDouble gives 0.0
    if int_value:
        cols[VALUE] = pa.array(i * 3 - 100 + f, pa.int64(), mask=vnull)
    else:
        cols[VALUE] = pa.array(i * 0.25 + f + 0.125, pa.float64(), mask=vnull)
    cols[KEEP] = _strings([None if k % 7 == 0 else ("no" if k % 3 == 0 else "yes") for k in i])
    cols["n.rowno"] = pa.array(i.astype(np.int64), pa.int64())
    for r in FROM_ROWS:
        cols[f"p.row{r}"] = _strings([None if k < r else f"v{r}" for k in i])
    cols["only.second"] = _strings([f"s{k % 4}" if pos == 1 else None for k in i])
    cols["only.glob2"] = _strings([f"g{k % 3}" if glob == 1 and k >= 5 else None for k in i])
    cols["fail.only"] = _strings([f"f{k % 5}" if k % 3 == 0 else None for k in i])
    cols["all.null"] = _strings([None] * ROWS)
    cols["all.empty"] = _strings([""] * ROWS)
    cols["all.nulltext"] = _strings(["null"] * ROWS)
    cols["mix.nothing"] = _strings([(None, "", "null")[k % 3] for k in i])
    cols["late.real"] = _strings([("", "null")[k % 2] if k < 100 else "real" for k in i])
    cols["plain.nulls"] = _strings([None if k < 40 or k % 5 == 0 else f"pl{k}" for k in i])
    cols["plain.full"] = _strings([f"pf{k % 90}" for k in i])
    cols["dict.nulls"] = _strings([None if k % 4 != 3 else f"d{k % 6}" for k in i])
    cols["n.i32"] = pa.array((i - 400).astype(np.int32), pa.int32(), mask=i < NUM_FROM["n.i32"])
    cols["n.i64"] = pa.array(i.astype(np.int64) * 10**10, pa.int64(), mask=i < NUM_FROM["n.i64"])
    cols["n.f32"] = pa.array((i * 0.1).astype(np.float32), pa.float32(), mask=i < NUM_FROM["n.f32"])
    f64 = i * 1.5
    f64[NUM_FROM["n.f64"]] = np.nan      # the first value is NaN ("NaN": keepable), 0.0 follows it
    f64[NUM_FROM["n.f64"] + 1] = 0.0
    cols["n.f64"] = pa.array(f64, pa.float64(), mask=i < NUM_FROM["n.f64"])
    cols["n.bool"] = pa.array(i % 2 == 0, pa.bool_(), mask=i < NUM_FROM["n.bool"])
    cols["twin.a"] = _strings([None if k < 200 else "ta" for k in i])
    cols["twin.b"] = _strings([None if k < 200 else f"tb{k}" for k in i])
    cols["tie.a"] = _strings([("a" if k >= 120 and pos == 0 else None) for k in i])
    cols["tie.b"] = _strings([("b" if k >= 120 and pos == 1 else None) for k in i])
    if pos == 1:
        cols["appended.col"] = _strings([None if k < 3 else f"ap{k % 2}" for k in i])   # not in the glob's first file
    return pa.table(cols)


PLAIN_COLS = ("plain.nulls", "plain.full")


def write_files(tmp_dir, flavour: str):
    """flavour "double": DOUBLE value column, one page per chunk.  "int": INT64 value column and small pages (a tile is
    then a few dozen rows).  Returns (paths, blobs)."""
    import pyarrow.parquet as pq
    paths, blobs = [], []
    for f in range(NFILES):
        t = table(f, flavour == "int")
        path = os.path.join(str(tmp_dir), f"tn_{flavour}_{f}.parquet")
        kw = dict(row_group_size=RG, use_dictionary=[c for c in t.column_names if c not in PLAIN_COLS],
                  compression="NONE" if f % 2 else "SNAPPY")
        if flavour == "int":
            kw.update(data_page_size=256, write_batch_size=50)
        pq.write_table(t, path, **kw)
        paths.append(path)
        blobs.append(open(path, "rb").read())
    return paths, blobs


def request(filt, nfiles=NFILES, reverse=False, processor=True, extra=None, base_extra=None) -> dict:
    """The PushDownRequest QueryEngineV2.evaluateTagQuery sends without a tagDataType."""
    be = {"id": "A", "dataset": "logs", "filter": filt}
    be.update(base_extra or {})
    req = {"baseExpr": be, "segmentRequests": [synth.segment_request(i, hour=0) for i in range(nfiles)],
           "reverseSort": reverse, "isTagQuery": True}
    if processor:
        req["processor"] = {"tagNameCompressionEnabled": True}
    req.update(extra or {})
    return req
