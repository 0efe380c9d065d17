"""Charts grouped by a numeric column (`:by status` over INT64 / INT32 / FLOAT / DOUBLE / BOOLEAN files) on the MI355X
through the C ABI, against the oracle over VARCHAR twins (tests/numgroup_ref.py, pinned by
tests/test_numgroup_ref_cpu.py): the union type per glob, NULLs, a file and a whole glob without the column, the
all-ones key, the discovery tables' LDS overflow and device regrows, sketches, metrics, field charts, formulas, and the
refused unions.  Bar: tests/parity.py::assert_rows_equal as it stands, rows and bulk export alike."""
import copy
import json
import os

import numpy as np
import pytest

from tests import numgroup_data as nd
from tests import numgroup_ref as nr
from tests.parity import assert_rows_equal, result_columns

pytestmark = pytest.mark.gpu

GLOB = 2
# globs: {A, D} BIGINT | {A, B} DOUBLE | {D, C} FLOAT | {E, E} BOOLEAN | {F, F} no column | {A, F} NULLs of F | {G, A}
ORDER = ["A", "D", "A", "B", "D", "C", "E", "E", "F", "F", "A", "F", "G", "A"]
AGGS = ("sum", "min", "max", "count", "avg")


def _segs(n=len(ORDER), step=60_000, start=None, end=None, dataset="logs"):
    from lakeside_amd import synth
    segs = [synth.segment_request(i, step=step, hour=0, dataset=dataset) for i in range(n)]
    for s in segs:
        if start is not None:
            s["startTs"], s["endTs"] = start, end
    return segs


def _name_in():
    from lakeside_amd import synth
    return synth.leaf(synth.NAME, "in", "metric_00", "metric_02")


def _num(k, op, v):
    return {"k": k, "v": [v], "op": op, "extracted": False, "computed": False, "dataType": "number"}


def _request(agg, gbs, filt=None, segs=None, dataset="logs", field=None):
    from lakeside_amd import synth
    return json.dumps(synth.pushdown(filt or _name_in(), segs or _segs(), agg, list(gbs), dataset=dataset, field=field))


@pytest.fixture(scope="module")
def files(engine, tmp_path_factory):
    root = tmp_path_factory.mktemp("numgroup")
    paths = [nd.write_file(root / f"f{i:02d}_{k}.parquet", k, seed=300 + i, rows=2000 + 71 * i) for i, k in enumerate(ORDER)]
    for p in paths:
        engine.load_segment(p)
    twins = nr.write_twins(paths, [nd.STATUS, nd.RATIO], GLOB, str(root / "twins"))
    return root, paths, twins


_cells = {}


def _expected(twins, gbs, filt, segs, label, dataset="logs"):
    """Oracle cells over the twins, once per (groupBys, filter, window) and shared by its aggregates."""
    from oracle import dataexpr as dx
    key = (tuple(twins[:1]), tuple(gbs), label)
    if key not in _cells:
        pr = dx.parse_pushdown(_request("sum", gbs, filt, segs, dataset))
        _cells[key] = (pr, dx.evaluate_glob_cells(pr, GLOB, twins))
    return _cells[key]


def _with_agg(pr, agg):
    pr = copy.deepcopy(pr)
    pr.baseExpr.chart.aggregation = agg
    return pr


def _bulk_rows(res):
    from oracle.cpu import tags_of_key
    ts, val, key = result_columns(res)
    return [(int(t), float(v), tags_of_key(k)) for t, v, k in zip(ts.tolist(), val.tolist(), key.tolist())]


def _check(engine, paths, twins, agg, gbs, filt=None, segs=None, label="base", dataset="logs", want=None):
    """Per-glob and merged rows, and the bulk export of both, against the oracle over the twins."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx
    if want is None:
        pr, cells = _expected(twins, gbs, filt, segs, label, dataset)
        want = ([[(c.ts, c.agg_value(agg), c.tags) for c in cs] for cs in cells], dx.merge_glob_cells(_with_agg(pr, agg), cells))
    req = _request(agg, gbs, filt, segs, dataset)
    what = f"{agg} by {list(gbs)} {label}"
    res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
    assert sum(len(w) for w in want[0]) > 0, what
    for gi, (g, w) in enumerate(zip(res.per_glob(len(want[0])), want[0])):
        assert_rows_equal(g, w, agg, f"{what} glob {gi}")
    globs = np.asarray(res.globs)
    bulk = _bulk_rows(res)
    for gi, w in enumerate(want[0]):
        assert_rows_equal([r for r, g in zip(bulk, globs.tolist()) if g == gi], w, agg, f"{what} bulk glob {gi}")
    merged = engine.eval_pushdown(req, paths, GLOB, LK_MERGED)
    assert_rows_equal(merged.rows(), want[1], agg, f"{what} merged")
    assert_rows_equal(_bulk_rows(merged), want[1], agg, f"{what} bulk merged")
    assert res.stats["general_segments"] == res.stats["segments"] > 0   # every segment on the general row scan
    return res, merged


# ---- 1. every aggregate x groupBys x filters over the seven globs ----

def _regex_and_eq():
    from lakeside_amd import synth
    return {"op": "and", "q1": synth.leaf(nd.SVC, "regex", "^svc-[1-3]$"), "q2": synth.leaf(synth.NAME, "eq", "metric_01")}


@pytest.mark.parametrize("filt", ["name_in", "regex_and_eq"])
@pytest.mark.parametrize("gbs", [(nd.STATUS,), (nd.STATUS, nd.SVC)], ids=["by_status", "by_status_service"])
def test_parity_every_aggregate(engine, files, gbs, filt):
    _, paths, twins = files
    f = None if filt == "name_in" else _regex_and_eq()
    for agg in AGGS:
        res, merged = _check(engine, paths, twins, agg, gbs, f, label=filt)
    tags = res.tags
    per = {g: {t.get(nd.STATUS) for t, gg in zip(tags, res.globs.tolist()) if gg == g} for g in range(7)}
    assert {"200", "-1", "9007199254740993", "-9223372036854775808"} <= per[0]          # BIGINT
    assert "9.007199254740992E15" in per[1] and "NaN" in per[1] and "-0.0" not in per[1] and "200" not in per[1]   # DOUBLE
    assert "1.6777216E7" in per[2] and "1.6777217E7" not in per[2]                      # FLOAT
    assert per[3] == {"true", "false", None}                                              # BOOLEAN
    assert per[4] == {None}                                                               # no file has the column
    assert None in per[5] and "-1" in per[5] and None in per[6]
    st = merged.stats
    assert st["numeric_dims"][0]["column"] == nd.STATUS and st["numdim_attempts"] == 1 and st["numdim_ms"] > 0
    # merged rows meet by text: "200.0" of the DOUBLE and FLOAT globs is one group, "200" of the BIGINT globs another
    assert {"200", "200.0"} <= {t.get(nd.STATUS) for t in merged.tags}


# ---- 2. numeric leaves ----

def test_numeric_leaf_on_the_group_column_and_on_another(engine, files, tmp_path):
    """`status ge 400 :by status`: the column is one numeric query column, filter and dimension alike.  The twins hold
    text, so the expectation filters the original rows first (a comparison under the union type: NaN orders greatest,
    NULL fails) and runs the oracle over the twins of what is left, without the leaf."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    _, paths, twins = files
    other = {"op": "and", "q1": _name_in(), "q2": _num(nd.OTHER, "lt", "500")}
    _check(engine, paths, twins, "sum", (nd.STATUS,), other, label="other_leaf")
    _check(engine, paths, twins, "max", (nd.STATUS, nd.SVC), other, label="other_leaf")
    kept = []
    for i, p in enumerate(paths):
        t = pq.read_table(p)
        if nd.STATUS in t.column_names:
            v = t.column(nd.STATUS).cast(pa.float64(), safe=False).to_numpy(zero_copy_only=False)   # NULL -> NaN here ...
            valid = t.column(nd.STATUS).is_valid().to_numpy(zero_copy_only=False)
            t = t.filter(pa.array(valid & ((v >= 400.0) | np.isnan(v))))                 # ... and out by `valid`
        else:
            t = t.slice(0, 0)
        path = str(tmp_path / f"kept_{i}.parquet")
        pq.write_table(t, path)
        kept.append(path)
    ktwins = nr.write_twins(kept, [nd.STATUS], GLOB, str(tmp_path / "twins"))
    # (BOOLEAN `ge 400` and a glob without the column: a comparison leaf DuckDB does not bind / a literal false)
    from oracle import dataexpr as dx
    pr = dx.parse_pushdown(_request("count", (nd.STATUS,)))
    cells = dx.evaluate_glob_cells(pr, GLOB, ktwins)
    cells[3] = []
    cells[4] = []
    leaf = {"op": "and", "q1": _name_in(), "q2": _num(nd.STATUS, "ge", "400")}
    for agg in ("count", "min"):
        want = ([[(c.ts, c.agg_value(agg), c.tags) for c in cs] for cs in cells], dx.merge_glob_cells(_with_agg(pr, agg), cells))
        res, _ = _check(engine, paths, twins, agg, (nd.STATUS,), leaf, label="own_leaf", want=want)
    seen = {t.get(nd.STATUS) for t in res.tags}
    assert "404" in seen and "NaN" in seen and "200" not in seen and None not in seen


# ---- 3. the window cuts tiles; one-second steps ----

def test_window_cuts_tiles_and_one_second_step(engine, files):
    from lakeside_amd import synth
    _, paths, twins = files
    cut = _segs(start=synth.T0 + 10 * 60_000 + 1234, end=synth.T0 + 40 * 60_000 + 777)
    _check(engine, paths, twins, "sum", (nd.STATUS,), segs=cut, label="cut")
    _check(engine, paths, twins, "min", (nd.STATUS, nd.SVC), segs=cut, label="cut")
    res, _ = _check(engine, paths, twins, "count", (nd.STATUS,), segs=_segs(step=1000), label="step1s")
    assert len(set(res.ts.tolist())) > 1000


# ---- 4 / 5. the discovery tables: LDS overflow, device regrows, deterministic ids ----

def _group_ids(res):
    import ctypes

    from lakeside_amd import _lib
    from lakeside_amd.evaluator import _View
    L = _lib.lib()
    h = res._owner.h
    gid = np.array(_View(res._owner, L.lk_result_group_ids(h), len(res.ts), "<u4"))
    dicts = []
    for c in range(L.lk_result_num_group_columns(h)):
        stride, ndim = ctypes.c_uint64(), ctypes.c_uint64()
        p = L.lk_result_tag_dictionary(h, c, ctypes.byref(stride), ctypes.byref(ndim))
        dicts.append((stride.value, [ctypes.string_at(p[d]) if p[d] else None for d in range(ndim.value)]))
    return gid, dicts


def _table_case(engine, root, name, rows, distinct, row_group_size, env, attempts):
    from lakeside_amd import LK_MERGED
    values = [int(v) for v in np.random.default_rng(7).choice(10 ** 9, distinct, replace=False) - 5 * 10 ** 8]
    path = nd.write_file(root / name, "A", seed=11, rows=rows, values=values, row_group_size=row_group_size)
    engine.load_segment(path)
    twins = nr.write_twins([path], [nd.STATUS], GLOB, str(root / ("twins_" + name)))
    want_distinct = len(nr.distinct_texts(twins, nd.STATUS))
    from lakeside_amd import synth
    every = synth.leaf(synth.NAME, "regex", "^metric_")
    segs = _segs(1, step=3_600_000)
    old = os.environ.get("LK_NUMDIM_INIT_SLOTS")
    if env is not None:
        os.environ["LK_NUMDIM_INIT_SLOTS"] = str(env)
    try:
        runs = []
        for agg in ("count", "sum"):
            res, merged = _check(engine, [path], twins, agg, (nd.STATUS,), every, segs, label=name)
            assert merged.stats["numdim_attempts"] >= attempts, merged.stats
            assert merged.stats["numeric_dims"] == [{"column": nd.STATUS, "values": want_distinct}]
            again = engine.eval_pushdown(_request(agg, (nd.STATUS,), every, segs), [path], GLOB, LK_MERGED)
            g1, d1 = _group_ids(merged)
            g2, d2 = _group_ids(again)
            assert np.array_equal(g1, g2) and d1 == d2, "dimension ids depend on the set of texts alone"
            runs.append(merged)
    finally:
        if env is not None:
            if old is None:
                del os.environ["LK_NUMDIM_INIT_SLOTS"]
            else:
                os.environ["LK_NUMDIM_INIT_SLOTS"] = old
    return want_distinct


def test_wide_column_overflows_lds_and_regrows_once(engine, tmp_path):
    """70,000 rows in one row group (a tile boundary at 64K inside it), 6,000 distinct values: more than the 1,024 keys
    of a workgroup's LDS table per tile, more than the 4,096 initial device slots."""
    assert _table_case(engine, tmp_path, "wide.parquet", 70_000, 6000, 70_000, None, 2) > 4096


def test_small_initial_table_regrows_twice(engine, tmp_path):
    """The initial-slots override at its floor of 64: 64 -> 512 -> 4,096 slots.  (A table grows x8, so two regrows need
    more than 512 distinct values: 600 here.)"""
    assert _table_case(engine, tmp_path, "w600.parquet", 3000, 600, 2048, 64, 3) > 512


# ---- 6. sketches ----

def test_percentiles_and_cardinality(engine, files):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx, hll
    from tests.test_gpu_features import _pct_rows_equal
    _, paths, twins = files
    segs = _segs(step=600_000)
    req_d = json.loads(_request("p95", (nd.STATUS,), segs=segs))
    req_d["baseExpr"]["chart"]["rollup"] = "p95"
    req = json.dumps(req_d)
    pr = dx.parse_pushdown(req)
    want = dx.evaluate_percentile_per_glob(pr, GLOB, twins)
    res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
    assert len(res) > 0
    for gi in range(len(want)):
        got = [(int(res.ts[r]), res.tags[r], float(res.values[r]), res.sketch(r)) for r in range(len(res)) if int(res.globs[r]) == gi]
        _pct_rows_equal(got, want[gi], 0.95, f"p95 glob {gi}")
    merged = engine.eval_pushdown(req, paths, GLOB, LK_MERGED)
    got = [(int(merged.ts[r]), merged.tags[r], float(merged.values[r]), merged.sketch(r)) for r in range(len(merged))]
    _pct_rows_equal(got, dx.merge_percentile(pr, want), 0.95, "p95 merged")
    req = _request("ces", (nd.STATUS, nd.SVC), segs=segs)
    pr = dx.parse_pushdown(req)
    want = dx.evaluate_ces_per_glob(pr, GLOB, twins)
    res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
    got = [[(int(res.ts[r]), float(res.values[r])) for r in range(len(res)) if int(res.globs[r]) == gi] for gi in range(len(want))]
    assert got == [[(ts, hll.estimate(ks)) for ts, ks in w] for w in want]
    assert max(v for g in got for _, v in g) > 4
    merged = engine.eval_pushdown(req, paths, GLOB, LK_MERGED)
    assert [(int(t), float(v)) for t, v in zip(merged.ts, merged.values)] == [(ts, hll.estimate(ks)) for ts, ks in dx.merge_ces(want)]


# ---- 7. metrics ----

def test_metrics_max_over_rollup(engine, tmp_path):
    kinds = ["A", "D", "B", "A"]
    paths = [nd.write_file(tmp_path / f"m{i}.parquet", k, seed=500 + i, rows=2500, metrics=True) for i, k in enumerate(kinds)]
    for p in paths:
        engine.load_segment(p)
    twins = nr.write_twins(paths, [nd.STATUS], GLOB, str(tmp_path / "twins"))
    req_d = json.loads(_request("max", (nd.STATUS,), segs=_segs(4, dataset="metrics"), dataset="metrics"))
    req_d["baseExpr"]["chart"]["rollup"] = "max"
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx
    req = json.dumps(req_d)
    pr = dx.parse_pushdown(req)
    cells = dx.evaluate_glob_cells(pr, GLOB, twins)
    res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
    assert len(res) > 100 and "redo" not in res.stats   # on the step grid
    for gi, (g, cs) in enumerate(zip(res.per_glob(2), cells)):
        assert_rows_equal(g, [(c.ts, c.agg_value("max"), c.tags) for c in cs], "max", f"metrics glob {gi}")
    merged = engine.eval_pushdown(req, paths, GLOB, LK_MERGED)
    assert_rows_equal(merged.rows(), dx.merge_glob_cells(pr, cells), "max", "metrics merged")


# ---- 8. field chart ----

def test_field_chart_avg_by_status(engine, files, tmp_path):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from tests import fieldchart_ref as fr
    _, paths, twins = files
    req = _request("avg", (nd.STATUS,), field=("lat", "number"))
    pr, cells, scale = fr.expected_cells(req, twins, GLOB, str(tmp_path / "ftwins"))   # twins composed
    res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
    assert len(res) > 100
    for gi, (g, w) in enumerate(zip(res.per_glob(len(cells)), fr.per_glob_rows(pr, cells, scale, "avg"))):
        assert_rows_equal(g, w, "avg", f"field avg glob {gi}")
    merged = engine.eval_pushdown(req, paths, GLOB, LK_MERGED)
    assert_rows_equal(merged.rows(), fr.merged_rows(pr, cells, scale, "avg"), "avg", "field avg merged")


# ---- 9. two numeric groupBys and a string one ----

def test_two_numeric_group_bys_and_service(engine, files):
    _, paths, twins = files
    for agg in ("sum", "count", "max"):
        res, merged = _check(engine, paths[:4], twins[:4], agg, (nd.STATUS, nd.RATIO, nd.SVC), segs=_segs(4), label="two")
    assert [d["column"] for d in merged.stats["numeric_dims"]] == [nd.STATUS, nd.RATIO]
    assert {t.get(nd.RATIO) for t in merged.tags} == {"0.25", "0.5", "NaN", "0.0", "0.001", None}


# ---- 10. refusals ----

def _refused(engine, req, paths, glob=GLOB, flags=None):
    from lakeside_amd import LK_PER_GLOB_ROWS, LakesideError
    from lakeside_amd._lib import LK_ERR_UNSUPPORTED
    with pytest.raises(LakesideError) as e:
        engine.eval_pushdown(req, paths, glob, flags or LK_PER_GLOB_ROWS)
    assert e.value.code == LK_ERR_UNSUPPORTED, str(e.value)
    return str(e.value)


def test_refusals_leave_the_engine_usable(engine, files, tmp_path):
    from lakeside_amd import LK_PER_GLOB_ROWS, synth
    _, paths, twins = files
    text = nd.write_file(tmp_path / "text.parquet", "V", seed=900, rows=600)
    engine.load_segment(text)
    a, d, e = paths[0], paths[1], paths[6]
    by = lambda n: _request("sum", (nd.STATUS,), segs=_segs(n))   # noqa: E731
    assert "VARCHAR in some files and numeric in others of glob 0" in _refused(engine, by(2), [text, a])
    assert "VARCHAR in glob 0 and numeric in glob 1" in _refused(engine, by(4), [text, text, a, d])
    assert "BOOLEAN in some files and numeric in others of glob 0" in _refused(engine, by(2), [e, a])
    mpath = nd.write_file(tmp_path / "m.parquet", "A", seed=901, rows=600, metrics=True)
    engine.load_segment(mpath)
    p95 = json.loads(_request("p95", (nd.STATUS,), segs=_segs(1, dataset="metrics"), dataset="metrics"))
    p95["baseExpr"]["chart"]["rollup"] = "max"
    assert "metrics p<NN> / ces take no numeric groupBy" in _refused(engine, json.dumps(p95), [mpath])
    ces = _request("ces", (nd.STATUS,), segs=_segs(1, dataset="metrics"), dataset="metrics")
    assert "metrics p<NN> / ces take no numeric groupBy" in _refused(engine, ces, [mpath])
    # unchanged: a string leaf on the numeric column empties that glob without an error ...
    eq = {"op": "and", "q1": _name_in(), "q2": synth.leaf(nd.STATUS, "eq", "200")}
    res = engine.eval_pushdown(_request("sum", (nd.STATUS,), eq, _segs(2)), [a, d], GLOB, LK_PER_GLOB_ROWS)
    assert len(res) == 0 and res.stats["failed_globs"] == 1
    # ... a VARCHAR status alone groups as a string column does, and the engine answers the numeric one afterwards
    res = engine.eval_pushdown(by(1), [text], GLOB, LK_PER_GLOB_ROWS)
    assert {t.get(nd.STATUS) for t in res.tags} == {"200", "404", "ok", None} and "numeric_dims" not in res.stats
    _check(engine, paths, twins, "count", (nd.STATUS,))


# ---- 11. formula ----

def test_formula_over_numeric_group_by(engine, files):
    """a / b * 100 with both operands `:by status`: the operands' dimensions reach the join through their TagCols."""
    from lakeside_amd import synth
    from tests import formula_ref as fr
    from tests.test_gpu_formula import be, expressions
    _, paths, twins = files
    for p in twins[:4]:
        engine.load_segment(p)
    err = {"op": "and", "q1": _name_in(), "q2": synth.leaf(nd.SVC, "in", "svc-1", "svc-2")}
    bes = {"a": be(err, "count", [nd.STATUS]), "b": be(_name_in(), "count", [nd.STATUS])}
    segs = {k: _segs(4) for k in bes}
    want, _, gbs = fr.expected(engine, bes, "a / b * 100", segs, {k: twins[:4] for k in bes}, 60_000, GLOB, synth.T0 + synth.HOUR)
    res = engine.eval_formula("a / b * 100", expressions(bes, segs, {k: paths[:4] for k in bes}), GLOB)
    assert fr.assert_rows(res.rows(), want, gbs, "a / b * 100") == len(res) > 100
    assert {"200", "200.0", "NaN", "-1"} <= {t.get(nd.STATUS) for t in res.tags}
