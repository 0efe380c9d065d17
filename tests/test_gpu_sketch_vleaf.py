"""`p<NN>` and `ces` charts with numeric comparison leaves on the chart's value column ("p99 of the requests slower than
250 ms") on the MI355X through the C ABI vs the oracle (files and requests: tests/vleaf_data.py; the leaf rule itself:
tests/test_vleaf_cpu.py).  scan_tiles' COUNT instantiations test the leaves per passing row before the value is binned;
in a `ces` call scan_lean takes the lean tiles; a segment with an INT64 value column takes the row scan into the same
hash table.

Expectation: dx.evaluate_percentile_per_glob / merge_percentile (bins identical, quantile bit for bit) and
dx.evaluate_ces_per_glob / merge_ces (estimates equal), per glob and merged, as tests/test_gpu_features.py compares them.
Routes from the call's stats."""
import pytest

from tests import vleaf_data as vd

pytestmark = pytest.mark.gpu

# glob 0 mixes a DOUBLE-value and an INT64-value file (scan_tiles / scan_lean and ex_scan feed one table), glob 1 the
# NULL values and the 70 names
MAIN = ["lean", "int64", "nulls", "names70"]
N_INT64 = 1


@pytest.fixture(scope="module")
def files(engine, tmp_path_factory):
    paths = vd.write_files(tmp_path_factory.mktemp("sketch_vleaf"))
    for p in paths.values():
        engine.load_segment(p)
    return paths


def _filter(names, value_filter):
    return vd.and_all([vd.name_filter(names)] + vd.VALUE_FILTERS[value_filter])


def _check_routes(st, agg, nsegs, n_general, lean_split=None):
    assert st["filter"]["vleaf"] == 1 and st["table"] == "hash", st
    assert st["segments"] == nsegs and st["general_segments"] == n_general, st
    if lean_split is not None:
        assert st["lean_split"] == lean_split, st


def _check_pct(engine, req, paths, q, label, **routes):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx
    from tests.test_gpu_features import _pct_rows_equal
    pr = dx.parse_pushdown(req)
    want = dx.evaluate_percentile_per_glob(pr, vd.GLOB, paths)
    res = engine.eval_pushdown(req, paths, vd.GLOB, LK_PER_GLOB_ROWS)
    _check_routes(res.stats, "p", len(paths), **routes)
    for gi in range(len(want)):
        _pct_rows_equal(vd.pct_rows(res, gi), want[gi], q, f"{label} glob {gi}")
    merged = engine.eval_pushdown(req, paths, vd.GLOB, LK_MERGED)
    _check_routes(merged.stats, "p", len(paths), **routes)
    _pct_rows_equal(vd.pct_rows(merged), dx.merge_percentile(pr, want), q, f"{label} merged")
    return sum(len(w) for w in want)


def _check_ces(engine, req, paths, label, **routes):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx, hll
    pr = dx.parse_pushdown(req)
    want = dx.evaluate_ces_per_glob(pr, vd.GLOB, paths)
    res = engine.eval_pushdown(req, paths, vd.GLOB, LK_PER_GLOB_ROWS)
    _check_routes(res.stats, "ces", len(paths), **routes)
    got = [[(int(res.ts[r]), float(res.values[r])) for r in range(len(res)) if int(res.globs[r]) == gi]
           for gi in range(len(want))]
    assert got == [[(ts, hll.estimate(ks)) for ts, ks in w] for w in want], label
    merged = engine.eval_pushdown(req, paths, vd.GLOB, LK_MERGED)
    _check_routes(merged.stats, "ces", len(paths), **routes)
    assert [(int(t), float(v)) for t, v in zip(merged.ts, merged.values)] == \
        [(ts, hll.estimate(ks)) for ts, ks in dx.merge_ces(want)], label
    return sum(len(w) for w in want)


@pytest.mark.parametrize("value_filter", list(vd.VALUE_FILTERS))
@pytest.mark.parametrize("agg", ["p50", "p99", "ces"])
def test_value_leaves(engine, files, agg, value_filter):
    """Without a groupBy and with a late string groupBy (scan_tiles' issue_one path), under a sparse name filter and one
    that passes every row, per glob and merged."""
    paths = [files[k] for k in MAIN]
    for gbs in ([], [vd.SVC]):
        for names in ("sparse", "dense"):
            req = vd.request(_filter(names, value_filter), agg, gbs, len(paths))
            label = f"{agg} {value_filter} {gbs} {names}"
            if agg == "ces":
                # scan_lean takes the lean file's tile, scan_tiles the NULL values' and the 70 names'
                n = _check_ces(engine, req, paths, label, n_general=N_INT64, lean_split=1)
            else:
                n = _check_pct(engine, req, paths, float(agg[1:]) / 100.0, label, n_general=N_INT64, lean_split=0)
            assert n >= 20, label   # 12 steps in two globs


@pytest.mark.parametrize("value_filter", ["gt", "lt_or_gt"])
def test_ces_on_scan_tiles_alone(engine, files, value_filter, monkeypatch):
    """LK_NO_LEAN=1 LK_NO_LEAN_SPLIT=1: scan_tiles takes every tile of the fused segments, the lean file's included."""
    monkeypatch.setenv("LK_NO_LEAN", "1")
    monkeypatch.setenv("LK_NO_LEAN_SPLIT", "1")
    paths = [files[k] for k in MAIN]
    for gbs in ([], [vd.SVC]):
        for names in ("sparse", "dense"):
            req = vd.request(_filter(names, value_filter), "ces", gbs, len(paths))
            _check_ces(engine, req, paths, f"ces tiles {value_filter} {gbs} {names}", n_general=N_INT64, lean_split=0)


def _count(res):
    from oracle import ddsketch
    return sum(ddsketch.decode(res.sketch(r)).count() for r in range(len(res)))


def _zeros(res):
    from oracle import ddsketch
    return sum(ddsketch.decode(res.sketch(r)).bins()[2] for r in range(len(res)))


def test_null_values_leave_the_zero_bin(engine, files):
    """A leaf-free percentile bins a NULL value as 0.0; under `v >= 0` (every non-NULL value of the file passes) the
    NULL rows are gone, and only they."""
    import pyarrow.parquet as pq
    from lakeside_amd import LK_MERGED
    from oracle import dataexpr as dx
    t = pq.read_table(files["nulls"], columns=[dx.VALUE])
    nulls = t.column(dx.VALUE).null_count
    assert 100 < nulls < 600
    free = engine.eval_pushdown(vd.request(vd.name_filter("dense"), "p50", [], 1), [files["nulls"]], vd.GLOB, LK_MERGED)
    leaf = vd.and_all([vd.name_filter("dense"), vd.num("ge", "0")])
    req = vd.request(leaf, "p50", [], 1)
    kept = engine.eval_pushdown(req, [files["nulls"]], vd.GLOB, LK_MERGED)
    assert kept.stats["filter"]["vleaf"] == 1 and kept.stats["general_segments"] == 0, kept.stats
    assert _count(free) == t.num_rows and _count(kept) == t.num_rows - nulls
    assert _zeros(free) - _zeros(kept) == nulls
    _check_pct(engine, req, [files["nulls"]], 0.5, "nulls ge 0", n_general=0, lean_split=0)


def test_untrackable_values_behind_a_leaf(engine, files):
    """The leaf is tested before the value is binned: +inf and NaN fail the call only where the leaf keeps them."""
    from lakeside_amd import LK_MERGED, _lib, synth
    from oracle import dataexpr as dx
    path = [files["nonfinite"]]

    def run(names, *value_leaves):
        filt = vd.and_all([synth.leaf(synth.NAME, "in", "metric_00", *names)] + list(value_leaves))
        return vd.request(filt, "p50", [], 1)

    def fails(req):
        with pytest.raises(_lib.LakesideError) as ei:
            engine.eval_pushdown(req, path, vd.GLOB, LK_MERGED)
        assert ei.value.code == _lib.LK_ERR_ARG and "trackable" in str(ei.value), ei.value
        with pytest.raises(ValueError):
            dx.evaluate_percentile_per_glob(dx.parse_pushdown(req), vd.GLOB, path)

    # +inf: the leaf-free call fails; `lt 1e300` drops the row and equals the oracle; `gt 0` keeps it and fails
    fails(run([vd.INF_NAME]))
    assert _check_pct(engine, run([vd.INF_NAME], vd.num("lt", "1e300")), path, 0.5, "inf lt", n_general=0) > 0
    fails(run([vd.INF_NAME], vd.num("gt", "0")))
    # NaN is the greatest value: `lt` drops it, `ge` keeps it
    fails(run([vd.NAN_NAME]))
    assert _check_pct(engine, run([vd.NAN_NAME], vd.num("lt", "1e300")), path, 0.5, "nan lt", n_general=0) > 0
    fails(run([vd.NAN_NAME], vd.num("ge", "0")))
    # ces never bins a value: both rows count where the leaf keeps them
    for names, leaf in (([vd.INF_NAME, vd.NAN_NAME], vd.num("gt", "0")), ([vd.NAN_NAME], vd.num("lt", "1e300"))):
        filt = vd.and_all([synth.leaf(synth.NAME, "in", "metric_00", *names), leaf])
        _check_ces(engine, vd.request(filt, "ces", [synth.NAME], 1), path, f"ces nonfinite {names}", n_general=0)


def test_formula_operand_with_a_leaf(engine, files):
    """a / b with a = p95 of the values above 1.5 (assembled on the host and uploaded), b = count: against queryapi's
    host evaluation of each operand (tests/formula_ref.py)."""
    from lakeside_amd import synth
    from tests import formula_ref as fr
    from tests.test_gpu_formula import be, expressions
    paths = [files[k] for k in MAIN]
    segs = [synth.segment_request(i, step=vd.STEP, hour=0) for i in range(len(paths))]
    bes = {"a": be(_filter("dense", "gt"), "p95", [vd.SVC]), "b": be(vd.name_filter("dense"), "count", [vd.SVC])}
    segs_by, paths_by = {k: segs for k in bes}, {k: paths for k in bes}
    want, _, gbs = fr.expected(engine, bes, "a / b", segs_by, paths_by, vd.STEP, vd.GLOB, 10 ** 14)
    res = engine.eval_formula("a / b", expressions(bes, segs_by, paths_by), vd.GLOB)
    n = fr.assert_rows(res.rows(), want, gbs, "a / b")
    assert n == len(res) and n >= 12 * 5
    assert res.stats["formula"]["operands_uploaded"] == 1, res.stats


def _refused():
    from lakeside_amd import synth
    name = vd.name_filter("sparse")
    v = lambda op, x: vd.num(op, x)   # noqa: E731
    return {
        "another column": (vd.and_all([name, vd.num("ge", "3", vd.NUMCOL)]), [], "logs"),
        "value and another column": (vd.and_all([name, v("gt", "1"), vd.num("ge", "3", vd.NUMCOL)]), [], "logs"),
        "mixed conjunct": (vd.and_all([name, {"op": "or", "q1": v("gt", "1"), "q2": synth.leaf(vd.SVC, "eq", "svc-1")}]), [], "logs"),
        "six value leaves": (vd.and_all([v("gt", "-9"), v("gt", "-8"), v("gt", "-7"), v("lt", "7"), v("lt", "8"), v("lt", "9")]), [], "logs"),
        "numeric groupBy": (vd.and_all([name, v("gt", "1")]), [vd.NUMCOL], "logs"),
        "metrics ces": (vd.and_all([name, v("gt", "1")]), [], "metrics"),
    }


@pytest.mark.parametrize("shape", ["another column", "value and another column", "mixed conjunct", "six value leaves",
                                   "numeric groupBy", "metrics ces", "LK_NO_VLEAF"])
def test_still_refused(engine, files, shape, monkeypatch):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS, _lib
    if shape == "LK_NO_VLEAF":
        monkeypatch.setenv("LK_NO_VLEAF", "1")
        filt, gbs, dataset = _filter("sparse", "gt"), [], "logs"
    else:
        filt, gbs, dataset = _refused()[shape]
    for agg in (["ces"] if dataset == "metrics" else ["p50", "ces"]):
        for flags in (LK_PER_GLOB_ROWS, LK_MERGED):
            with pytest.raises(_lib.LakesideError) as ei:
                engine.eval_pushdown(vd.request(filt, agg, gbs, 1, dataset), [files["lean"]], vd.GLOB, flags)
            assert ei.value.code == _lib.LK_ERR_UNSUPPORTED, (shape, agg, ei.value)
            assert "numeric comparison leaves in sketch queries" in str(ei.value), (shape, agg, ei.value)
