"""scan_clu -- the name-filter scan over the name-clustered value copy built at load -- against the oracle (MI355X).

Every case evaluates per glob and merged with LK_PLAN_BYTES, compares the rows with the oracle (tests/parity.py),
asserts from `clustered_tiles` that the kernel took tiles (or, where the case says so, none), and evaluates again with
LK_NO_CLUSTER=1 (scan_lean / scan_tiles): the same rows, bit for bit for MIN / MAX and sums of integral values, within
the suite's SUM bar (1 ulp of the correctly rounded value, both paths against the oracle) for real values.

scan_clu takes segments whole (every tile a copy and sorted timestamps, the widest tile below two steps), so the
synthetic segments here have 4,096-row pages: 2^20 rows over an hour give 256 tiles of about 14 s."""
import json
import os

import numpy as np
import pytest

from tests import nonfinite_data as nf
from tests.parity import assert_rows_equal, from_jsonable

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NAME = "_cardinalhq.name"
ALL16 = [f"metric_{i:02d}" for i in range(16)]
ROWS = 1 << 20


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_segs = {}      # (engine id, spec key) -> (key, blob)
_cells = {}     # request identity -> oracle cells


def _segment(engine, index, rows=ROWS, value_mode=0, null_frac=0.0, page_rows=1 << 12):
    from lakeside_amd import synth
    k = (id(engine), index, rows, value_mode, null_frac, page_rows)
    if k not in _segs:
        s = synth.make_segment(synth.segment_spec(index, rows=rows, value_mode=value_mode, null_frac=null_frac,
                                                  rg_rows=1 << 18, page_rows=page_rows))
        key = f"clu/{index}/{rows}/{value_mode}/{null_frac}/{page_rows}"
        engine.put_segment_ptr(key, s.ptr, s.size)
        _segs[k] = (key, s.bytes())
        s.free()
    return _segs[k]


def _bits(values):
    return np.asarray(values, np.float64).view(np.uint64).tolist()


def _check(engine, keys, blobs, segs, filt, agg, gbs=(), glob_size=10, taken=True, integral=True, label=""):
    """Oracle parity per glob and merged with the clustered path, then the same rows with LK_NO_CLUSTER=1."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS, LK_PLAN_BYTES, synth
    from oracle import dataexpr as dx
    req = json.dumps(synth.pushdown(filt, segs, agg, list(gbs)))
    ck = (tuple(keys), json.dumps(filt, sort_keys=True), tuple(gbs), json.dumps(segs, sort_keys=True), glob_size)
    pr = dx.parse_pushdown(req)
    if ck not in _cells:
        _cells[ck] = dx.evaluate_glob_cells(dx.parse_pushdown(req), glob_size, keys, sources=blobs)
    cells = _cells[ck]
    want_pg = [[(c.ts, c.agg_value(agg), c.tags) for c in cs] for cs in cells]
    want_mg = dx.merge_glob_cells(pr, cells)
    out = {}
    for off in (False, True):
        with _Env(**({"LK_NO_CLUSTER": 1} if off else {})):
            pg = engine.eval_pushdown(req, keys, glob_size, LK_PER_GLOB_ROWS | LK_PLAN_BYTES)
            mg = engine.eval_pushdown(req, keys, glob_size, LK_MERGED | LK_PLAN_BYTES)
        for gi, (g, w) in enumerate(zip(pg.per_glob(len(want_pg)), want_pg)):
            assert_rows_equal(g, w, agg, f"{label} off={off} glob {gi}")
        assert_rows_equal(mg.rows(), want_mg, agg, f"{label} off={off} merged")
        for r in (pg, mg):
            st = r.stats
            if off:
                assert st["clustered"] == 0 and st["clustered_tiles"] == 0, st
            elif taken:
                assert st["clustered"] == 1 and st["clustered_tiles"] > 0, st
            else:
                assert st["clustered_tiles"] == 0, st
        out[off] = (pg, mg)
    for a, b in zip(out[False], out[True]):
        assert a.ts.tolist() == b.ts.tolist() and a.tags == b.tags, label
        if agg != "sum" or integral:
            assert _bits(a.values) == _bits(b.values), f"{label}: LK_NO_CLUSTER rows differ"
    return out[False]


def _one(engine, index=0, **kw):
    from lakeside_amd import synth
    key, blob = _segment(engine, index, **kw)
    return [key], [blob], [synth.segment_request(index)]


def _with(segs, step=None, window=None):
    segs = [dict(s) for s in segs]
    for s in segs:
        if step:
            s["stepInMillis"] = step
        if window:
            s["startTs"] += window[0]
            s["endTs"] -= window[1]
    return segs


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_every_code_range(engine, agg):
    """`:in` all 16 names grouped by name: every code's range of every tile."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    pg, mg = _check(engine, keys, blobs, segs, synth.leaf(NAME, "in", *ALL16), agg, [NAME], label=f"all16 {agg}")
    assert len({t["name"] for t in mg.tags}) == 16
    assert mg.stats["clustered_tiles"] == mg.stats["tiles"]


def test_one_name_minute_step(engine):
    """C2's shape: most tiles pinned to one bucket, those holding a minute boundary split."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    pg, mg = _check(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "metric_07"), "sum", label="eq 1m")
    assert len(mg) == 60 and mg.stats["lean_split"] >= 1


@pytest.mark.parametrize("step,window", [(20000, None), (30000, None), (30000, (7000, 11000)), (60000, (61000, 1795000))])
def test_split_tiles(engine, step, window):
    """14 s tiles at 20 s / 30 s steps: one to three boundaries in many tiles; windows that cut tiles at both ends."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    for agg in ("sum", "max"):
        _check(engine, keys, blobs, _with(segs, step, window), synth.leaf(NAME, "in", "metric_03", "metric_11"), agg, [NAME],
               label=f"split {step} {window} {agg}")


def test_too_many_buckets_not_taken(engine):
    """A 7 s step: 14 s tiles are not below two steps, so no tile is taken and the rows still match."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    _check(engine, keys, blobs, _with(segs, 7000), synth.leaf(NAME, "eq", "metric_07"), "sum", taken=False, label="7s")


def test_mixed_call(engine):
    """One call over a clean segment (scan_clu) and a segment with NULL names and values, which gets no copy (scan_lean
    / scan_tiles): the three kernels share one call and one table.  The kernels are mixed per segment, not per tile."""
    from lakeside_amd import synth
    k0, b0 = _segment(engine, 0)
    k1, b1 = _segment(engine, 1, rows=1 << 19, value_mode=0, null_frac=0.05)
    segs = [synth.segment_request(0), synth.segment_request(1)]
    for agg in ("sum", "min"):
        pg, mg = _check(engine, [k0, k1], [b0, b1], segs, synth.leaf(NAME, "eq", "metric_07"), agg, glob_size=1,
                        label=f"mixed {agg}")
        assert 0 < mg.stats["clustered_tiles"] < mg.stats["tiles"], mg.stats


def test_full_size_tiles(engine):
    """The bench's tile shape: 2^21 rows in 65,536-row pages give 32 or 33 tiles of up to 112 s, still below two 60 s
    steps, so nearly every tile is split with one or two minute boundaries, a code's range (about 4,096 values;
    65,536 for the `:in` of all names) takes many passes of the streaming loop, the split search's sample gaps are 256
    rows wide and `crows` holds row indices up to 65,535."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 3, rows=1 << 21, page_rows=1 << 16)
    for agg in ("sum", "min"):
        pg, mg = _check(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "metric_07"), agg, label=f"64K tiles eq {agg}")
        assert mg.stats["tiles"] >= 32 and mg.stats["clustered_tiles"] == mg.stats["tiles"], mg.stats
    _check(engine, keys, blobs, _with(segs, window=(333000, 444000)), synth.leaf(NAME, "in", *ALL16), "max", [NAME],
           label="64K tiles all16 max window")


def test_no_copy_for_segments_scan_clu_cannot_take():
    """The host takes segments whole, so a segment with a tile that has no copy (NULLs) or unsorted timestamps gets no
    copy at all: nothing allocated, nothing in the cache weight, and its queries run the other kernels.  (A segment
    mixing eligible and ineligible tiles in one scan_clu call -- the tile-granular rule -- does not exist in this
    engine: see DESIGN section 9.)"""
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES, synth
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    eng = Engine(0)
    try:
        specs = {"nulls": synth.segment_spec(0, rows=1 << 18, null_frac=0.001, rg_rows=1 << 17, page_rows=1 << 12),
                 "shuffled": synth.segment_spec(0, rows=1 << 18, rg_rows=1 << 17, page_rows=1 << 12, ts_shuffle=1)}
        for label, spec in specs.items():
            s = synth.make_segment(spec)
            blob = s.bytes()
            eng.put_segment_ptr(label, s.ptr, s.size)
            s.free()
            assert eng.stats["clu_bytes"] == 0 and eng.stats["clu_alloc_failed"] == 0, (label, eng.stats)
            req = json.dumps(synth.pushdown(synth.leaf(NAME, "eq", "metric_07"), [synth.segment_request(0)], "sum", []))
            res = eng.eval_pushdown(req, [label], 10, LK_MERGED | LK_PLAN_BYTES)
            assert res.stats["clustered"] == 0 and res.stats["clustered_tiles"] == 0, (label, res.stats)
            pr = dx.parse_pushdown(req)
            assert_rows_equal(res.rows(), dx.merge_glob_cells(pr, dx.evaluate_glob_cells(pr, 10, [label], sources=[blob])),
                              "sum", label)
            eng.evict(label)
    finally:
        eng.close()


def test_name_absent_from_dictionary(engine):
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    pg, mg = _check(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "no_such_metric"), "sum", label="absent name")
    assert len(mg) == 0


@pytest.fixture(scope="module")
def odd_file(engine, tmp_path_factory):
    """A file written with pyarrow (the synthetic generator spreads all 16 names over every tile): pages of about
    1,024 rows, so tiles of about 1,024 rows and 31 s; `rare` appears in the first 700 rows only (an empty range in
    every later tile), rows 2,048 .. 4,095 are all `solo` (tiles holding a single code of a four-entry dictionary), and
    the row count, 20,011, leaves a last tile whose rows are no multiple of 64."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    n = 20011
    rng = np.random.default_rng(77)
    ts = synth.T0 + np.sort(rng.integers(0, 600_000, n))
    names = rng.choice(["a", "b", "solo"], n).astype(object)
    names[rng.choice(700, 60, replace=False)] = "rare"
    names[2048:4096] = "solo"
    val = rng.integers(-500, 500, n).astype(np.float64)
    t = pa.table({dx.TIMESTAMP: pa.array(ts, pa.int64()), dx.VALUE: pa.array(val, pa.float64()),
                  dx.NAME: pa.array(names.tolist(), pa.string())})
    path = str(tmp_path_factory.mktemp("clu") / "odd.parquet")
    pq.write_table(t, path, compression="NONE", use_dictionary=[dx.NAME], row_group_size=n, data_page_size=4096,
                   column_encoding={dx.TIMESTAMP: "PLAIN", dx.VALUE: "PLAIN"})
    engine.load_segment(path)
    with open(path, "rb") as f:
        return path, f.read()


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_absent_short_and_one_code_tiles(engine, odd_file, agg):
    from lakeside_amd import synth
    path, blob = odd_file
    segs = [synth.segment_request(0, hour=0)]
    for names in (["rare"], ["solo"], ["rare", "solo", "a", "b"]):
        pg, mg = _check(engine, [path], [blob], segs, synth.leaf(NAME, "in", *names), agg, [NAME],
                        label=f"odd {names} {agg}")
        assert mg.stats["tiles"] >= 8, mg.stats   # the page size did cut the row group into small tiles


def test_globs(engine):
    """Four segments, two globs: per-glob cells and merged cells (both in every _check)."""
    from lakeside_amd import synth
    ks, bs = zip(*[_segment(engine, i, rows=1 << 19, page_rows=1 << 11) for i in range(4)])
    segs = [synth.segment_request(i) for i in range(4)]
    for agg in ("sum", "max"):
        pg, mg = _check(engine, list(ks), list(bs), segs, synth.leaf(NAME, "in", "metric_07", "metric_08"), agg, [NAME],
                        glob_size=2, label=f"globs {agg}")
        assert mg.stats["clustered_tiles"] == mg.stats["tiles"]


def test_real_values_compensated(engine):
    """value_mode=1 (lognormal reals: the compensated path), and integral data with the exact-sum shortcut off."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 2, value_mode=1)
    pg, mg = _check(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "metric_07"), "sum", integral=False, label="real")
    assert mg.stats["exact_sum"] == 0
    keys, blobs, segs = _one(engine)
    with _Env(LK_NO_EXACT_SUM=1):
        pg, mg = _check(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "metric_07"), "sum", label="no exact sum")
        assert mg.stats["exact_sum"] == 0


@pytest.mark.parametrize("step", [3_600_000, 2_400_000])
@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_nonfinite(engine, tmp_path_factory, agg, step):
    """tests/nonfinite_data.py (+-inf, NaN, -0.0, overflowing sums), one 4,096-row tile per file spanning the hour:
    pinned at a 1 h step, split in two at 40 min.  As test_gpu_nonfinite.py: the oracle's rows, and the same class
    (finite, +inf, -inf, NaN, signed zero) row by row."""
    from lakeside_amd import synth
    if "nf" not in _segs:
        paths, blobs = nf.write_files(tmp_path_factory.mktemp("clu_nf"), "clean")
        for p in paths:
            engine.load_segment(p)
        _segs["nf"] = (paths, blobs)
    paths, blobs = _segs["nf"]
    pg, mg = _check(engine, paths, blobs, nf.segments(step), nf.all_names(), agg, [NAME], glob_size=nf.GLOB, integral=False,
                    label=f"nonfinite {agg} {step}")
    from oracle import dataexpr as dx
    req = json.dumps(synth.pushdown(nf.all_names(), nf.segments(step), agg, [NAME]))
    cells = dx.evaluate_glob_cells(dx.parse_pushdown(req), nf.GLOB, paths, sources=blobs)
    want = dx.merge_glob_cells(dx.parse_pushdown(req), cells)

    def classes(rows):
        zero = ("-0", "+0")
        return sorted((t, tags.get("name"), "0" if agg == "sum" and nf.value_class(v) in zero else nf.value_class(v))
                      for t, v, tags in rows)
    assert classes(mg.rows()) == classes(want)


def test_option_off(engine):
    """{"cluster_values": false}: no copy is built or counted, scan_clu never runs, the rows are the same."""
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES, synth
    from lakeside_amd.evaluator import Engine
    keys, blobs, segs = _one(engine)
    req = json.dumps(synth.pushdown(synth.leaf(NAME, "in", "metric_02", "metric_07"), segs, "sum", [NAME]))
    on = engine.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES)
    assert on.stats["clustered"] == 1 and engine.stats["clu_bytes"] >= 10 * ROWS
    assert engine.segment_bytes >= engine.stats["clu_bytes"] + len(blobs[0])
    eng = Engine(0, cluster_values=False)
    try:
        eng.put_segment(keys[0], blobs[0])
        assert eng.stats["clu_bytes"] == 0
        off = eng.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES)
        assert off.stats["clustered"] == 0 and off.stats["clustered_tiles"] == 0
        assert off.ts.tolist() == on.ts.tolist() and off.tags == on.tags and _bits(off.values) == _bits(on.values)
    finally:
        eng.close()


@pytest.mark.timeout(120)
def test_distributed_world1_loopback(engine):
    """lk_eval_pushdown_dist at world 1 with the loopback data path takes scan_clu too."""
    from lakeside_amd import synth
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    keys, blobs, segs = _one(engine)
    req = json.dumps(synth.pushdown(synth.leaf(NAME, "eq", "metric_07"), segs, "sum", []))
    pr = dx.parse_pushdown(req)
    want = dx.merge_glob_cells(pr, dx.evaluate_glob_cells(pr, 10, keys, sources=blobs))
    with _Env(LK_COMM_LOOPBACK=1):
        eng = Engine(0)
        try:
            eng.comm_init(Engine.unique_id(), 1, 0)
            eng.put_segment(keys[0], blobs[0])
            res = eng.eval_pushdown_dist(req, keys, None, 10)
            assert res.stats["clustered"] == 1, res.stats
            assert_rows_equal(res.rows(), want, "sum", "dist loopback")
        finally:
            eng.close()


def _golden():
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        return [c for c in json.load(f) if c["request"]["baseExpr"]["chart"]["aggregation"] in ("sum", "min", "max") and
                c["expected_merged"] is not None]


@pytest.mark.parametrize("case", _golden(), ids=lambda c: c["name"])
def test_golden_same_rows_either_way(engine, case):
    """The golden segments: the golden rows with the clustered path on (whichever segments it takes at the case's
    step) and with LK_NO_CLUSTER=1 (MIN / MAX bit for bit, sums each within the golden bar).  Measured on the MI355X:
    none of the twelve golden cases takes the path (`clustered` is 0 in each: their tiles are wider than two of their
    steps, their segments hold NULLs, or the query is a metrics or multi-column one), although some golden segments do
    carry a copy.  So these cases pin that the copy's presence changes no row, and assert that fact (`clustered` 0)
    so that a change in it is noticed; they cannot assert a tile count above 0."""
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES
    paths = [os.path.join(GOLDEN, p) for p in case["segments"]]
    for p in paths:
        engine.load_segment(p)
    agg = case["request"]["baseExpr"]["chart"]["aggregation"]
    on = engine.eval_pushdown(json.dumps(case["request"]), paths, case["glob_size"], LK_MERGED | LK_PLAN_BYTES)
    with _Env(LK_NO_CLUSTER=1):
        off = engine.eval_pushdown(json.dumps(case["request"]), paths, case["glob_size"], LK_MERGED | LK_PLAN_BYTES)
    assert_rows_equal(on.rows(), from_jsonable(case["expected_merged"]), agg, case["name"])
    assert_rows_equal(off.rows(), from_jsonable(case["expected_merged"]), agg, case["name"] + " LK_NO_CLUSTER")
    assert off.stats["clustered"] == 0
    assert on.stats["clustered"] == 0 and on.stats["clustered_tiles"] == 0, on.stats
    assert on.ts.tolist() == off.ts.tolist() and on.tags == off.tags
    if agg != "sum":
        assert _bits(on.values) == _bits(off.values)
