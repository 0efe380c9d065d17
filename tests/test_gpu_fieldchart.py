"""Field charts (chart.fieldName / fieldType: the aggregate of the rows' `<fieldName>$<fieldType>` column) on the MI355X
through the C ABI, against the oracle over twin files (tests/fieldchart_ref.py): INT64 / INT32 / FLOAT / DOUBLE / VARCHAR
fields, NULLs, a field missing from a file and from a whole glob, the duration / datasize divisors, per glob and merged;
the NULL-free DOUBLE field on the value chart's own kernels, bit for bit; cell existence under `IS NOT NULL`; the empty
and the refused shapes."""
import json

import numpy as np
import pytest

from tests import fieldchart_ref as fr
from tests.parity import assert_rows_equal

pytestmark = pytest.mark.gpu

SVC = "resource.service.name"
NFILES, GLOB = 4, 2
WORDS = ["abc", "timeout", "Zed", "unknown"]


def write_files(root, rows=70_000):
    """4 files of ~70,000 rows in row groups of 30,000 (tiles of one page each, a partial one last)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    rng = np.random.default_rng(23)
    paths = []
    for i in range(NFILES):
        n = rows + 257 * i
        ts = np.sort(synth.T0 + rng.integers(0, synth.HOUR, n))
        lat = rng.lognormal(0, 2, n)
        lat[rng.random(n) < 0.01] = np.nan
        svc_id = rng.integers(0, 5, n)
        svc_null = rng.random(n) < 0.1
        dur_null = rng.random(n) < 0.1
        # existence: every svc-0 row of the first minute has no duration (its cells hold rows, but none with a field)
        dur_null |= (ts < synth.T0 + 60_000) & (svc_id == 0) & ~svc_null
        txt = [str(v) if k else WORDS[v % len(WORDS)]
               for k, v in zip((rng.random(n) < 0.8).tolist(), rng.integers(-500, 5000, n).tolist())]
        for j in range(0, n, 97):   # other spellings of class-1 numbers
            txt[j] = ("%.3f" % (j / 7.0), "%de2" % (j % 90), "-%d.5E-1" % (j % 1000), "007")[(j // 97) % 4]
        size = rng.integers(0, 1 << 20, n)
        cols = {
            dx.TIMESTAMP: pa.array(ts, pa.int64()),
            dx.VALUE: pa.array(lat, pa.float64()),
            dx.NAME: pa.array([f"metric_{k:02d}" for k in rng.integers(0, 4, n)], pa.string()),
            SVC: pa.array([f"svc-{k}" for k in svc_id], pa.string(), mask=svc_null),
            "size$datasize": pa.array(size.astype(np.int32) if i % 2 else size.astype(np.int64),
                                      mask=rng.random(n) < 0.1),
            "ratio$number": pa.array(rng.random(n).astype(np.float32), pa.float32()),
            "lat$number": pa.array(lat.copy(), pa.float64()),
            # DOUBLE with NULLs: stays on the fused kernels, where `rows` also count the rows without a field
            "gap$number": pa.array(rng.normal(0, 50, n), pa.float64(), mask=rng.random(n) < 0.1),
            "txt$number": pa.array(txt, pa.string(), mask=rng.random(n) < 0.1),
            "attr.dur": pa.array(rng.integers(0, 5_000_000, n), pa.int64()),
        }
        if i == 0:   # absent from file 1 (NULLs in glob 0) and from both files of the last glob (an empty glob)
            cols["dur$duration"] = pa.array(rng.integers(0, 5_000_000_000, n), pa.int64(), mask=dur_null)
        t = pa.table(cols)
        path = str(root / f"field{i}.parquet")
        strings = [c for c in t.column_names if t.schema.field(c).type == pa.string()]
        pq.write_table(t, path, compression="NONE", use_dictionary=strings, row_group_size=30_000,
                       data_page_size=1 << 20, column_encoding={c: "PLAIN" for c in t.column_names if c not in strings})
        paths.append(path)
    return paths


@pytest.fixture(scope="module")
def files(engine, tmp_path_factory):
    root = tmp_path_factory.mktemp("fieldchart")
    paths = write_files(root)
    for p in paths:
        engine.load_segment(p)
    return root, paths


def _segs(step=60_000, start=None, end=None):
    from lakeside_amd import synth
    segs = [synth.segment_request(i, step=step, hour=0) for i in range(NFILES)]
    for s in segs:
        if start is not None:
            s["startTs"], s["endTs"] = start, end
    return segs


def _name_eq():
    from lakeside_amd import synth
    return synth.leaf(synth.NAME, "eq", "metric_01")


def _request(field, agg, gbs=(), filt=None, segs=None):
    from lakeside_amd import synth
    return json.dumps(synth.pushdown(filt or _name_eq(), segs or _segs(), agg, list(gbs), field=field))


_expect_cache = {}


def _expected(files, field, gbs, filt=None, segs=None, label="base"):
    """Oracle cells over the twins, computed once per (field, groupBys, filter, window) and shared by its aggregates."""
    root, paths = files
    key = (field, tuple(gbs), label)
    if key not in _expect_cache:
        out = root / f"twins_{field[0]}_{len(gbs)}_{label}"
        _expect_cache[key] = fr.expected_cells(_request(field, "sum", gbs, filt, segs), paths, GLOB, str(out))
    return _expect_cache[key]


def _check(engine, files, field, agg, gbs, filt=None, segs=None, label="base", merged=True):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    _, paths = files
    pr, cells, scale = _expected(files, field, gbs, filt, segs, label)
    req = _request(field, agg, gbs, filt, segs)
    what = f"{field[0]}${field[1]} {agg} by {list(gbs)} {label}"
    res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
    for gi, (g, w) in enumerate(zip(res.per_glob(len(cells)), fr.per_glob_rows(pr, cells, scale, agg))):
        assert_rows_equal(g, w, agg, f"{what} glob {gi}")
    if merged:
        got = engine.eval_pushdown(req, paths, GLOB, LK_MERGED).rows()
        assert_rows_equal(got, fr.merged_rows(pr, cells, scale, agg), agg, f"{what} merged")
    return res


FIELDS = [("dur", "duration"), ("size", "datasize"), ("ratio", "number"), ("lat", "number"), ("gap", "number"),
          ("txt", "number")]


def _allowed(field):
    """(aggregate, merged too) pairs the gate evaluates for this fieldType."""
    if field[1] in ("duration", "datasize"):
        return [("sum", True), ("min", True), ("max", True), ("avg", False)]
    return [("sum", True), ("min", True), ("max", True), ("count", True), ("avg", True)]


@pytest.mark.parametrize("gbs", [(), (SVC,)], ids=["nogroup", "by_service"])
@pytest.mark.parametrize("field", FIELDS, ids=[f[0] for f in FIELDS])
def test_parity_every_aggregate(engine, files, field, gbs):
    for agg, merged in _allowed(field):
        res = _check(engine, files, field, agg, gbs, merged=merged)
        assert len(res) > 0
    if field[0] == "dur":   # the glob without a dur$duration file is empty; the other answers
        assert set(res.globs.tolist()) == {0}
    if field[0] in ("lat", "gap"):   # DOUBLE fields run on the fused kernels, with or without NULLs
        assert res.stats["general_segments"] == 0


def _num(k, op, v):
    return {"k": k, "v": [v], "op": op, "extracted": False, "computed": False, "dataType": "number"}


@pytest.mark.parametrize("field,agg", [(("dur", "duration"), "sum"), (("size", "datasize"), "max"),
                                       (("lat", "number"), "avg"), (("txt", "number"), "min")],
                         ids=["dur_sum", "size_max", "lat_avg", "txt_min"])
def test_parity_filters(engine, files, field, agg):
    from lakeside_amd import synth
    in_regex = {"op": "and", "q1": synth.leaf(synth.NAME, "in", "metric_00", "metric_02"),
                "q2": synth.leaf(SVC, "regex", "^svc-[1-3]$")}
    merged = not (agg == "avg" and field[1] != "number")
    _check(engine, files, field, agg, (SVC,), in_regex, label="in_regex", merged=merged)
    leaf = {"op": "and", "q1": _name_eq(), "q2": _num("attr.dur", "lt", "2500000")}
    res = _check(engine, files, field, agg, (), leaf, label="numeric_leaf", merged=merged)
    assert res.stats["general_segments"] > 0   # the row scan: the definition level is a conjunct there too


def test_parity_window_cuts_tiles_and_one_second_step(engine, files):
    from lakeside_amd import synth
    cut = _segs(start=synth.T0 + 10 * 60_000 + 1234, end=synth.T0 + 40 * 60_000 + 777)
    for field, agg in [(("size", "datasize"), "sum"), (("lat", "number"), "max"), (("txt", "number"), "count")]:
        _check(engine, files, field, agg, (SVC,), segs=cut, label="cut")
    sec = _segs(step=1000)   # a tile spans many buckets
    for field, agg in [(("dur", "duration"), "max"), (("lat", "number"), "sum"), (("gap", "number"), "min"),
                       (("txt", "number"), "sum")]:   # gap: buckets whose few rows all lack the field, fused kernels
        res = _check(engine, files, field, agg, (), segs=sec, label="step1s")
        assert len(set(res.ts.tolist())) > 1000


def test_same_kernel_same_bits(engine, files):
    """lat$number is the value column's bits: the field chart takes the value chart's launches and returns its rows."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    _, paths = files
    for agg in ("sum", "min", "max", "count", "avg"):
        for flags in (LK_PER_GLOB_ROWS, LK_MERGED):
            f = engine.eval_pushdown(_request(("lat", "number"), agg), paths, GLOB, flags)
            v = engine.eval_pushdown(_request(None, agg), paths, GLOB, flags)
            assert f.stats["general_segments"] == 0 and v.stats["general_segments"] == 0
            assert f.stats["segments"] == v.stats["segments"] == NFILES
            assert len(f) == len(v) > 0
            assert f.ts.tolist() == v.ts.tolist() and f.globs.tolist() == v.globs.tolist()
            assert np.asarray(f.values).tobytes() == np.asarray(v.values).tobytes(), agg
            assert f.tags == v.tags


def test_existence_null_field_rows_make_no_cell(engine, files):
    from lakeside_amd import LK_PER_GLOB_ROWS, synth
    _, paths = files
    every = synth.leaf(synth.NAME, "in", "metric_00", "metric_01", "metric_02", "metric_03")
    f = engine.eval_pushdown(_request(("dur", "duration"), "sum", (SVC,), every), paths, GLOB, LK_PER_GLOB_ROWS)
    v = engine.eval_pushdown(_request(None, "sum", (SVC,), every), paths, GLOB, LK_PER_GLOB_ROWS)
    cell = lambda r: {(t, g, tags[SVC]) for t, g, tags in zip(r.ts.tolist(), r.globs.tolist(), r.tags) if SVC in tags}   # noqa: E731
    first_svc0 = {c for c in cell(v) if c[0] == synth.T0 and c[1] == 0 and c[2] == "svc-0"}
    assert first_svc0, "the fixture holds rows of svc-0 in the first minute of glob 0"
    assert not (first_svc0 & cell(f)), "a cell whose rows all have a NULL field is not in the field chart"
    assert {c for c in cell(f) if c[0] == synth.T0 and c[1] == 0}, "the other services of that minute are"
    assert cell(f) < cell(v)


def test_empty_globs(engine, files):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    _, paths = files
    for flags in (LK_PER_GLOB_ROWS, LK_MERGED):   # fieldName without fieldType: every glob empty, the call succeeds
        res = engine.eval_pushdown(_request(("dur", None), "sum"), paths, GLOB, flags)
        assert len(res) == 0 and res.rows() == []
        assert res.stats["rows_scanned"] == 0
    req = json.loads(_request(("dur", "duration"), "sum"))
    req["baseExpr"]["chart"]["fieldType"] = None   # a JSON null is an absent fieldType
    assert len(engine.eval_pushdown(json.dumps(req), paths, GLOB, LK_MERGED)) == 0
    # no file of the last glob has dur$duration: that glob is empty while the first answers
    res = engine.eval_pushdown(_request(("dur", "duration"), "max", (SVC,)), paths, GLOB, LK_PER_GLOB_ROWS)
    assert len(res) > 0 and set(res.globs.tolist()) == {0}
    # asked of the last glob alone, the call still succeeds with no rows
    res = engine.eval_pushdown(_request(("dur", "duration"), "max", (SVC,), segs=_segs()[2:]), paths[2:], GLOB,
                               LK_PER_GLOB_ROWS)
    assert len(res) == 0


def _small_file(root, name, extra):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    n = 1000
    rng = np.random.default_rng(5)
    cols = {dx.TIMESTAMP: pa.array(np.sort(synth.T0 + rng.integers(0, synth.HOUR, n)), pa.int64()),
            dx.VALUE: pa.array(rng.random(n), pa.float64()),
            dx.NAME: pa.array(["metric_01"] * n, pa.string())}
    cols.update(extra(n))
    path = str(root / name)
    pq.write_table(pa.table(cols), path)
    return path


def _refused(engine, req, paths, flags=None):
    from lakeside_amd import LK_PER_GLOB_ROWS, LakesideError
    from lakeside_amd._lib import LK_ERR_UNSUPPORTED
    with pytest.raises(LakesideError) as e:
        engine.eval_pushdown(req, paths, GLOB, flags or LK_PER_GLOB_ROWS)
    assert e.value.code == LK_ERR_UNSUPPORTED, str(e.value)
    return str(e.value)


def test_refusals_by_request(engine, files):
    """Every rule of the shape gate that the request alone decides."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    _, paths = files

    def edited(field, agg="sum", gbs=(), **be):
        r = json.loads(_request(field, agg, gbs))
        r["baseExpr"].update(be)
        return json.dumps(r)

    rollup_ces = json.loads(_request(("lat", "number"), "sum"))
    rollup_ces["baseExpr"]["chart"]["rollup"] = "ces"
    table = [
        ("metrics dataset", edited(("lat", "number"), dataset="metrics"), LK_PER_GLOB_ROWS),
        ("p95", _request(("lat", "number"), "p95"), LK_PER_GLOB_ROWS),
        ("ces", _request(("lat", "number"), "ces"), LK_PER_GLOB_ROWS),
        ("ces rollup", json.dumps(rollup_ces), LK_PER_GLOB_ROWS),
        ("dotted name", _request(("attr.dur", "number"), "sum"), LK_PER_GLOB_ROWS),
        ("dotted type", _request(("lat", "num.ber"), "sum"), LK_PER_GLOB_ROWS),
        ("upper case", _request(("Lat", "number"), "sum"), LK_PER_GLOB_ROWS),
        ("leading digit", _request(("1lat", "number"), "sum"), LK_PER_GLOB_ROWS),
        ("groupBy is fieldName", _request(("lat", "number"), "sum", ("lat",)), LK_PER_GLOB_ROWS),
        ("count on duration", _request(("dur", "duration"), "count"), LK_PER_GLOB_ROWS),
        ("count on datasize", _request(("size", "datasize"), "count"), LK_MERGED),
        ("merged avg on duration", _request(("dur", "duration"), "avg"), LK_MERGED),
        ("merged avg on datasize", _request(("size", "datasize"), "avg"), LK_MERGED),
        ("extract", edited(("lat", "number"), extract={"regex": "(?P<x>.*)", "names": ["x"], "inputField": "m"}),
         LK_PER_GLOB_ROWS),
        ("compute", edited(("lat", "number"), compute={"fieldName": "c", "expr": "1"}), LK_PER_GLOB_ROWS),
    ]
    for label, req, flags in table:
        msg = _refused(engine, req, paths, flags)
        assert "field chart" in msg or "extract / compute" in msg, (label, msg)
    # ... while the per-glob avg on a duration is evaluated (test_parity_every_aggregate), as is the value chart
    assert len(engine.eval_pushdown(_request(None, "count"), paths, GLOB, LK_MERGED)) > 0


BAD_TEXT = ["1e999", " 12", "+5", "inf", ""]


def test_refusals_by_column(engine, tmp_path):
    """A BOOLEAN field; a numeric / VARCHAR mix in one glob; VARCHAR text outside the two classes -- refused only when
    a segment of the request references it."""
    import pyarrow as pa
    from lakeside_amd import LK_PER_GLOB_ROWS, synth
    segs1 = [synth.segment_request(0, hour=0)]
    flag = _small_file(tmp_path, "flag.parquet", lambda n: {"flag$number": pa.array([k % 2 == 0 for k in range(n)], pa.bool_())})
    engine.load_segment(flag)
    req1 = lambda f: json.dumps(synth.pushdown(_name_eq(), segs1, "sum", [], field=f))   # noqa: E731
    assert "neither numeric nor VARCHAR" in _refused(engine, req1(("flag", "number")), [flag])
    good = _small_file(tmp_path, "good.parquet", lambda n: {"bad$number": pa.array([str(k) for k in range(n)], pa.string())})
    engine.load_segment(good)
    for k, text in enumerate(BAD_TEXT):
        bad = _small_file(tmp_path, f"bad{k}.parquet",
                          lambda n: {"bad$number": pa.array([text if j == 500 else str(j) for j in range(n)], pa.string())})
        engine.load_segment(bad)
        assert "bad$number holds" in _refused(engine, req1(("bad", "number")), [bad]), repr(text)
        segs2 = [synth.segment_request(i, hour=0) for i in range(2)]   # refused next to a good file too
        _refused(engine, json.dumps(synth.pushdown(_name_eq(), segs2, "sum", [], field=("bad", "number"))), [good, bad])
    # the engine's dictionary of bad$number now holds every bad text; a request that references none of them answers
    res = engine.eval_pushdown(req1(("bad", "number")), [good], GLOB, LK_PER_GLOB_ROWS)
    assert len(res) > 0 and float(np.sum(res.values)) == float(sum(range(1000)))
    mixed = _small_file(tmp_path, "mixed.parquet", lambda n: {"bad$number": pa.array(list(range(n)), pa.int64())})
    engine.load_segment(mixed)
    segs2 = [synth.segment_request(i, hour=0) for i in range(2)]
    req2 = json.dumps(synth.pushdown(_name_eq(), segs2, "sum", [], field=("bad", "number")))
    assert "numeric in some files and VARCHAR in others" in _refused(engine, req2, [good, mixed])
    # the same two files in globs of their own are both evaluated
    res = engine.eval_pushdown(req2, [good, mixed], 1, LK_PER_GLOB_ROWS)
    assert set(res.globs.tolist()) == {0, 1}
