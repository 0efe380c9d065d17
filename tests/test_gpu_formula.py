"""Formulas over DataExprs (lk_eval_formula: a / b * 100 joined per (timestamp, group key) on the device) on the MI355X
through the C ABI, against tests/formula_ref.py: every variable through queryapi.evaluate_base_expr, then Formula.eval
restated in Python.  Values bit for bit (NaN = NaN), rows per timestamp as a set keyed by the group-value tuple.

Data: 3 synthetic segments of 2^14 rows (hours 0, 0, 1; 30 % NULL values, so sparse `sum` cells read exactly 0.0), a
fourth at hour 2 that only some expressions use (their bucket bases then differ), glob size 2 so operands merge across
globs, 60 s step; a hand-made logs file (NULL names and services, a numeric field, queryTags) and a metrics file.
Tests 1-8 run in both table modes: the dense cell table and, with formula_dense_max_cells = 0, the hash table."""
import json

import numpy as np
import pytest

from tests import formula_ref as fr

pytestmark = pytest.mark.gpu

STEP, GLOB = 60_000, 2
NOW = 10 ** 14
ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """Segment bytes and files, made once; every test loads them into its own engine."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    root = tmp_path_factory.mktemp("formula")
    hours = [0, 0, 1, 2]
    blobs = []
    for i, h in enumerate(hours):
        seg = synth.make_segment(synth.segment_spec(i, rows=1 << 14, hour=h, null_frac=0.3, rg_rows=1 << 12,
                                                    page_rows=1 << 10))
        blobs.append(seg.bytes())
        seg.free()
    rng = np.random.default_rng(5)
    # logs: names and services with NULLs (rows whose own tags are all absent), a numeric field
    n = 6000
    ts = np.sort(synth.T0 + rng.integers(0, 10 * STEP, n))
    name_id = rng.integers(0, 3, n)
    svc_id = rng.integers(0, 4, n)
    logs = pa.table({
        dx.TIMESTAMP: pa.array(ts, pa.int64()),
        dx.VALUE: pa.array(rng.integers(1, 50, n).astype(np.float64), pa.float64()),
        dx.NAME: pa.array([f"m{k}" for k in name_id], pa.string(), mask=name_id == 0),
        synth.SERVICE: pa.array([("svc-qt", "svc-1", "svc-2", "x")[k] for k in svc_id], pa.string(), mask=svc_id == 3),
        "kind": pa.array(["k"] * n, pa.string()),
        "lat$number": pa.array(rng.integers(1, 900, n).astype(np.float64), pa.float64()),
    })
    logs_path = str(root / "logs.parquet")
    strings = [dx.NAME, synth.SERVICE, "kind"]
    pq.write_table(logs, logs_path, compression="NONE", use_dictionary=strings, row_group_size=2500,
                   data_page_size=1 << 20, column_encoding={c: "PLAIN" for c in logs.column_names if c not in strings})
    # metrics: rollup_sum on the step grid
    m = 20_000
    mts = synth.T0 + STEP * rng.integers(0, 30, m)
    metrics = pa.table({
        dx.TIMESTAMP: pa.array(np.sort(mts), pa.int64()),
        "rollup_sum": pa.array(rng.integers(0, 1000, m).astype(np.float64), pa.float64()),
        synth.NAME: pa.array([f"metric_{k:02d}" for k in rng.integers(0, 3, m)], pa.string()),
        synth.SERVICE: pa.array([f"svc-{k:03d}" for k in rng.integers(0, 7, m)], pa.string()),
    })
    metrics_path = str(root / "metrics.parquet")
    strings = [synth.NAME, synth.SERVICE]
    pq.write_table(metrics, metrics_path, compression="NONE", use_dictionary=strings,
                   column_encoding={c: "PLAIN" for c in metrics.column_names if c not in strings},
                   row_group_size=m // 3, data_page_size=65536)
    return {"hours": hours, "blobs": blobs, "logs": logs_path, "metrics": metrics_path}


def make_engine(data, **opts):
    from lakeside_amd.evaluator import Engine
    eng = Engine(0, **opts)
    for i, b in enumerate(data["blobs"]):
        eng.put_segment(f"fx/{i}", b)
    eng.load_segment(data["logs"])
    eng.load_segment(data["metrics"])
    return eng


@pytest.fixture(params=["dense", "hash"])
def eng(request, data):
    e = make_engine(data, **({} if request.param == "dense" else {"formula_dense_max_cells": 0}))
    e.mode = request.param
    yield e
    e.close()


@pytest.fixture
def eng1(data):
    e = make_engine(data)
    yield e
    e.close()


def synth_segs(data, which, step=STEP):
    from lakeside_amd import synth
    return ([synth.segment_request(i, step=step, hour=data["hours"][i]) for i in which], [f"fx/{i}" for i in which])


def be(filt, agg, gbs=(), chart_type="count", dataset="logs", metric_type=None, field=None, ident="x"):
    e = {"id": ident, "dataset": dataset, "filter": filt,
         "chart": {"aggregation": agg, "groupBys": list(gbs), "type": chart_type}}
    if metric_type is not None:
        e["metricType"] = metric_type
    if field is not None:
        e["chart"]["fieldName"], e["chart"]["fieldType"] = field
    return e


def expressions(bes, segs, paths):
    return {k: {"pushDown": {"baseExpr": bes[k], "segmentRequests": segs[k], "reverseSort": False, "isTagQuery": False},
                "paths": paths[k]} for k in bes}


def check(engine, formula, bes, sp, mode=None):
    """Runs the formula and the reference; returns (result, expectation, rows compared)."""
    segs = {k: sp[k][0] for k in bes}
    paths = {k: sp[k][1] for k in bes}
    want, _, gbs = fr.expected(engine, bes, formula, segs, paths, STEP, GLOB, NOW)
    res = engine.eval_formula(formula, expressions(bes, segs, paths), GLOB)
    n = fr.assert_rows(res.rows(), want, gbs, formula)
    assert n == len(res)
    assert not res.globs.any()
    st = res.stats["formula"]
    if mode is not None and len(res):
        assert st["mode"] == mode
    return res, want, n


def all_names():
    from lakeside_amd import synth
    return synth.leaf(synth.NAME, "regex", "^metric_")


def test_error_rate(eng, data):
    """1. a = count under a service regex, b = count over everything, both :by service; a / b * 100.  b also reads the
    later-hour segment, so the operands' bucket bases differ; b alone has 18,000 live cells (hash mode: probing chains)."""
    from lakeside_amd import synth
    filt = {"op": "and", "q1": all_names(), "q2": synth.leaf(synth.SERVICE, "regex", "^svc-0[0-4]")}
    bes = {"a": be(filt, "count", [synth.SERVICE]), "b": be(all_names(), "count", [synth.SERVICE])}
    sp = {"a": synth_segs(data, [0, 1, 2]), "b": synth_segs(data, [0, 1, 2, 3])}
    res, want, n = check(eng, "a / b * 100", bes, sp, eng.mode)
    assert 1000 < n <= 2 * 60 * 50                           # a's keys: 50 services over two hours
    assert all(0.0 <= v <= 100.0 for v in res.values)
    assert res.tag_names[:2] == ["name", synth.SERVICE]
    st = res.stats["formula"]
    assert st["operands_on_device"] == 2 and st["operands_uploaded"] == 0
    res, _, n = check(eng, "b + 0", bes, sp, eng.mode)
    assert 4096 < n <= 3 * 60 * 100


def test_no_group_bys(eng, data):
    """2. keys are "default": the two names of the filter collapse to one row per timestamp; a constant has no tags."""
    from lakeside_amd import synth
    bes = {"a": be(synth.leaf(synth.NAME, "in", "metric_01", "metric_02"), "sum"),
           "b": be(synth.leaf(synth.NAME, "in", "metric_01", "metric_02", "metric_03"), "count")}
    sp = {"a": synth_segs(data, [0, 1, 2]), "b": synth_segs(data, [0, 1, 2, 3])}
    res, _, n = check(eng, "a / b", bes, sp, eng.mode)
    assert n == 120 and all(t in ({"name": "metric_01"}, {"name": "metric_02"}) for t in res.tags)
    res, _, n = check(eng, "a * 100", bes, sp, eng.mode)
    assert n == 120 and all(t in ({"name": "metric_01"}, {"name": "metric_02"}) for t in res.tags)
    res, _, n = check(eng, "100 * a", bes, sp, eng.mode)      # tags of e1, the constant: none
    assert n == 120 and all(t == {} for t in res.tags)


def test_fill(eng, data):
    """3. a covers a subset of b's services: + keeps b-only keys (0 + b, b's tags), the other operators drop them."""
    from lakeside_amd import synth
    filt = {"op": "and", "q1": synth.leaf(synth.NAME, "eq", "metric_03"), "q2": synth.leaf(synth.SERVICE, "regex", "^svc-00")}
    bes = {"a": be(filt, "max", [synth.SERVICE]), "b": be(synth.leaf(synth.NAME, "eq", "metric_03"), "sum", [synth.SERVICE])}
    sp = {"a": synth_segs(data, [0, 1, 2]), "b": synth_segs(data, [0, 1, 2])}
    counts = {}
    for f in ["a + b", "b + a", "a - b", "a * b", "a / b", "b + 0"]:
        res, want, counts[f] = check(eng, f, bes, sp, eng.mode)
        if f in ("a + b", "b + a"):
            only_b = [t for t in res.tags if not t.get(synth.SERVICE, "").startswith("svc-00")]
            assert only_b and all(t["name"] == "metric_03" for t in only_b)
    assert counts["a + b"] == counts["b + a"] == counts["b + 0"]
    assert counts["a - b"] == counts["a * b"] < counts["a + b"]
    assert counts["a / b"] < counts["a * b"]                  # b's exact zeros (all-NULL cells) drop under /


def test_division_by_zero(eng, data):
    """4. a / (b - b) and the -0.0 divisor a / ((0 - b) * 0) give LK_OK and no rows; a sum that is exactly 0 in some
    cells drops those cells only."""
    from lakeside_amd import synth
    bes = {"a": be(all_names(), "count", [synth.SERVICE]),
           "b": be(synth.leaf(synth.NAME, "eq", "metric_07"), "sum", [synth.SERVICE])}
    sp = {"a": synth_segs(data, [0, 1]), "b": synth_segs(data, [0, 1])}
    for f in ["a / (b - b)", "a / ((0 - b) * 0)"]:
        res, want, n = check(eng, f, bes, sp)
        assert n == 0 and len(res) == 0 and want == {}
    _, _, n_mul = check(eng, "a * b", bes, sp, eng.mode)
    _, _, n_div = check(eng, "a / b", bes, sp, eng.mode)
    assert 0 < n_div < n_mul


def test_transformer_twice(eng, data):
    """5. a rate chart at a 60 s step divides by 60 twice; a metrics count chart over a rate metric multiplies twice."""
    from lakeside_amd import synth
    bes = {"a": be(synth.leaf(synth.NAME, "eq", "metric_05"), "sum", [synth.SERVICE], chart_type="rate"),
           "c": be(synth.leaf(synth.NAME, "eq", "metric_05"), "sum", [synth.SERVICE])}
    sp = {"a": synth_segs(data, [0, 1, 2]), "c": synth_segs(data, [0, 1, 2])}
    res, _, n = check(eng, "a + 0", bes, sp, eng.mode)
    raw, _, _ = check(eng, "c + 0", bes, sp, eng.mode)
    assert n == len(raw) > 0
    key = lambda r: (r[0], r[2].get(synth.SERVICE, ""))   # noqa: E731
    plain = {key(r): r[1] for r in raw.rows()}
    assert all(fr.same_value(v, plain[key((t, v, g))] / 60.0 / 60.0) for t, v, g in res.rows())
    seg = [synth.segment_request(0, step=STEP, hour=0, dataset="metrics")]
    mb = {"m": be(synth.leaf(synth.NAME, "in", "metric_00", "metric_01"), "sum", [synth.SERVICE], dataset="metrics",
                  metric_type="rate"),
          "g": be(synth.leaf(synth.NAME, "eq", "metric_01"), "max", [synth.SERVICE], dataset="metrics")}
    msp = {"m": (seg, [data["metrics"]]), "g": (seg, [data["metrics"]])}
    res, _, n = check(eng, "m + 0", mb, msp, eng.mode)
    assert n == 30 * 7
    rawm, _, _ = check(eng, "g / m", mb, msp, eng.mode)
    assert len(rawm) > 0


def test_nesting(eng, data):
    """6. the same variable twice, and a nested ratio."""
    from lakeside_amd import synth
    filt = {"op": "and", "q1": all_names(), "q2": synth.leaf("_cardinalhq.level", "eq", "ERROR")}
    bes = {"a": be(filt, "count", [synth.NAMESPACE, synth.SERVICE]),
           "b": be(synth.leaf(synth.NAME, "in", "metric_00", "metric_09"), "count", [synth.SERVICE, synth.NAMESPACE])}
    sp = {"a": synth_segs(data, [0, 1, 2]), "b": synth_segs(data, [1, 2, 3])}
    _, _, n = check(eng, "a / (a + b)", bes, sp, eng.mode)
    assert n > 1000
    _, _, n = check(eng, "(a - b) / (a + b) * 100", bes, sp, eng.mode)
    assert n > 5


def test_aggregations(eng, data):
    """7. avg / max, min - min, a field-chart operand: all on the device; a p95 operand is assembled on the host and
    uploaded."""
    from lakeside_amd import synth
    one = synth.leaf(synth.NAME, "eq", "metric_02")
    bes = {"a": be(one, "avg", [synth.NAMESPACE]), "b": be(one, "max", [synth.NAMESPACE]),
           "c": be(synth.leaf(synth.NAME, "eq", "metric_04"), "min", [synth.NAMESPACE]),
           "d": be(one, "min", [synth.NAMESPACE]), "p": be(one, "p95", [synth.NAMESPACE]),
           "n": be(one, "count", [synth.NAMESPACE])}
    sp = {k: synth_segs(data, [0, 1, 2]) for k in bes}
    for f in ["a / b", "c - d"]:
        res, _, n = check(eng, f, bes, sp, eng.mode)
        assert n > 200 and res.stats["formula"]["operands_uploaded"] == 0
    lseg = [synth.segment_request(0, step=STEP, hour=0)]
    k = synth.leaf("kind", "eq", "k")
    fb = {"f": be(k, "sum", [synth.SERVICE], field=("lat", "number")), "v": be(k, "count", [synth.SERVICE])}
    fsp = {"f": (lseg, [data["logs"]]), "v": (lseg, [data["logs"]])}
    res, _, n = check(eng, "f / v", fb, fsp, eng.mode)
    assert n > 20 and res.stats["formula"]["operands_uploaded"] == 0
    res, _, n = check(eng, "p / n", bes, sp, eng.mode)
    assert n > 200
    assert res.stats["formula"]["operands_uploaded"] == 1 and res.stats["formula"]["operands_on_device"] == 1


def test_constant_on_the_left(eng, data):
    """8. 100 * a under groupBys: the value, the timestamp, the key, and tags among the candidate rows' (a's here)."""
    from lakeside_amd import synth
    bes = {"a": be(synth.leaf(synth.NAME, "in", "metric_10", "metric_11"), "count", [synth.SERVICE]),
           "b": be(synth.leaf(synth.NAME, "eq", "metric_12"), "count", [synth.SERVICE])}
    sp = {"a": synth_segs(data, [0, 1, 2]), "b": synth_segs(data, [0, 1, 2])}
    res, want, n = check(eng, "100 * a", bes, sp, eng.mode)
    assert n > 1000
    some = next(iter(want.values()))
    assert all(s.cands is not None for s in some.values())   # the expectation does carry candidates here
    res, want, n = check(eng, "100 * a + b", bes, sp, eng.mode)
    assert n > 1000


def test_query_tags_rows(eng1, data):
    """9. rows whose own tags are all absent (NULL name, NULL service) take the segment's queryTags and key as
    eval_merged_rows keys them -- here onto svc-qt, where named rows and a row without a name compete."""
    from lakeside_amd import synth
    seg = [synth.segment_request(0, step=STEP, hour=0, query_tags={synth.SERVICE: "svc-qt", "zone": "z"})]
    k = synth.leaf("kind", "eq", "k")
    bes = {"a": be(k, "sum", [synth.SERVICE]), "b": be(k, "count", [synth.SERVICE])}
    sp = {"a": (seg, [data["logs"]]), "b": (seg, [data["logs"]])}
    res, want, n = check(eng1, "a / b", bes, sp)
    assert n == 10 * 4                                        # svc-qt, svc-1, svc-2 and "" in ten buckets
    assert "zone" in res.tag_names and not any("zone" in t for t in res.tags)   # a named row wins under svc-qt
    # queryTags that key the all-absent rows onto a service no other row has: they come out as rows of their own
    seg2 = [synth.segment_request(0, step=STEP, hour=0, query_tags={synth.SERVICE: "svc-zz", "zone": "z"})]
    sp2 = {"a": (seg2, [data["logs"]]), "b": (seg2, [data["logs"]])}
    for f in ["a / b", "a + b", "100 * a"]:
        res, want, n = check(eng1, f, bes, sp2)
        assert n == 10 * 5
        if f != "100 * a":
            qt_rows = [t for t in res.tags if t.get("zone") == "z"]
            assert len(qt_rows) == 10 and all(t == {synth.SERVICE: "svc-zz", "zone": "z"} for t in qt_rows)


def test_refusals(eng1, data):
    """10. the gate, by status code and named rule; unreferenced expressions are not evaluated."""
    from lakeside_amd import synth
    from lakeside_amd._lib import LakesideError
    segs, paths = synth_segs(data, [0, 1])
    bes = {"a": be(all_names(), "count", [synth.SERVICE]), "b": be(all_names(), "sum", [synth.SERVICE]),
           "c": be(all_names(), "sum", [synth.NAMESPACE])}
    sp = {k: (segs, paths) for k in bes}
    ex = expressions(bes, {k: segs for k in bes}, {k: paths for k in bes})

    def refused(formula, exprs, code, word):
        with pytest.raises(LakesideError) as e:
            eng1.eval_formula(formula, exprs, GLOB)
        assert e.value.code == code, str(e.value)
        assert word in str(e.value), str(e.value)

    refused("a / c", ex, UNSUPPORTED, "groupBy")
    exemplar = json.loads(json.dumps(ex))
    del exemplar["b"]["pushDown"]["baseExpr"]["chart"]
    refused("a / b", exemplar, UNSUPPORTED, "chart")
    tagq = json.loads(json.dumps(ex))
    del tagq["b"]["pushDown"]["baseExpr"]["chart"]
    tagq["b"]["pushDown"]["isTagQuery"] = True
    tagq["b"]["pushDown"]["tagDataType"] = {"tagName": synth.SERVICE, "dataType": "string"}
    refused("a / b", tagq, UNSUPPORTED, "tag query")
    steps = json.loads(json.dumps(ex))
    for s in steps["b"]["pushDown"]["segmentRequests"]:
        s["stepInMillis"] = 10_000
    refused("a / b", steps, ARG, "step")
    refused("a ^ 2", ex, UNSUPPORTED, "'^'")
    refused("a / total", ex, ARG, "total")
    res = eng1.eval_formula("5 + 3", ex, GLOB)
    assert len(res) == 0 and res.stats["rows_scanned"] == 0 and res.stats["formula"]["operands_on_device"] == 0
    one = eng1.eval_formula("a + 0", ex, GLOB)
    two = eng1.eval_formula("a + b", ex, GLOB)
    assert one.stats["rows_scanned"] > 0 and one.stats["formula"]["operands_on_device"] == 1
    assert two.stats["rows_scanned"] == 2 * one.stats["rows_scanned"]
    # b's request (another step) is not even read when the formula does not name it
    assert eng1.eval_formula("a + 0", steps, GLOB).stats["rows_scanned"] == one.stats["rows_scanned"]


def test_end_to_end_payloads(eng1, data):
    """11. queryapi.evaluate_formula: id = the formula, label per Formula.label, tags, value, and the drop of
    timestamps later than now."""
    from lakeside_amd import queryapi as qa
    from lakeside_amd import synth
    filt = {"op": "and", "q1": all_names(), "q2": synth.leaf(synth.SERVICE, "regex", "^svc-01")}
    bes = {"a": be(filt, "count", [synth.SERVICE], ident="a"), "b": be(all_names(), "count", [synth.SERVICE], ident="b")}
    sp = {"a": synth_segs(data, [0, 1, 2]), "b": synth_segs(data, [0, 1, 2, 3])}
    segs = {k: sp[k][0] for k in bes}
    paths = {k: sp[k][1] for k in bes}
    now = synth.T0 + synth.HOUR + 7 * STEP
    formula = "a / b * 100"
    want, ast, gbs = fr.expected(eng1, bes, formula, segs, paths, STEP, GLOB, now)
    wantp = fr.expected_payloads(want, ast, formula, bes)
    got = qa.evaluate_formula(eng1, bes, formula, segs, paths, STEP, GLOB, now)
    assert 300 < len(got) == len(wantp) <= 68 * 10
    assert max(p["message"]["timestamp"] for p in got) == now
    for g, w in zip(got, wantp):
        gm, wm = g["message"], w["message"]
        assert (g["id"], g["type"], gm["timestamp"], gm["tags"], gm["label"]) == \
               (formula, "timeseries", wm["timestamp"], wm["tags"], wm["label"])
        assert fr.same_value(gm["value"], wm["value"])
    svc = got[0]["message"]["tags"][synth.SERVICE]
    assert got[0]["message"]["label"] == f"(resource.service.name = {svc}) / (resource.service.name = {svc}) * 100.0"


def test_regrow(data):
    """12. a hash table that starts from 64 slots regrows (no row dropped) and equals the dense result."""
    from lakeside_amd import synth
    bes = {"a": be(synth.leaf(synth.NAME, "in", "metric_01", "metric_02", "metric_03", "metric_04"), "sum",
                   [synth.SERVICE]),
           "b": be(all_names(), "count", [synth.SERVICE])}
    sp = {"a": synth_segs(data, [0, 1, 2]), "b": synth_segs(data, [0, 1, 2, 3])}
    rows = {}
    for mode, opts in (("dense", {}), ("hash", {"formula_dense_max_cells": 0, "formula_hash_slots": 64})):
        e = make_engine(data, **opts)
        try:
            res, _, n = check(e, "a / b * 100", bes, sp, mode)
            st = res.stats["formula"]
            assert (st["regrows"] >= 1) == (mode == "hash")
            rows[mode] = sorted((t, fr.bits(v), tuple(sorted(g.items()))) for t, v, g in res.rows())
        finally:
            e.close()
    assert rows["dense"] == rows["hash"] and len(rows["dense"]) > 1000
