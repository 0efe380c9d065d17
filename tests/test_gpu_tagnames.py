"""Tag-name queries (isTagQuery without a tagDataType) on the MI355X through the C ABI against the restatement
(tests/tagnames_ref.py): every (file set, filter) case per glob and merged -- timestamps, values bit for bit, tags as sets
of (name, text), the glob column and the row order -- then reverseSort, the stats, queryapi.evaluate_tag_query and the
refusals.  The files are tests/tagnames_data.py's (900 rows each); every case here is refused by an engine without the
route ("tag queries without a tagDataType", LK_ERR_UNSUPPORTED)."""
import json
import os

import numpy as np
import pytest

from tests import tagnames_data as td

pytestmark = pytest.mark.gpu

PREFIX = "tag queries without a tagDataType: "
UNSUPPORTED = -2


@pytest.fixture(scope="module")
def files(engine, tmp_path_factory):
    d = tmp_path_factory.mktemp("tagnames_gpu")
    out = {fl: td.write_files(d, fl) for fl in ("double", "int")}
    for paths, _ in out.values():
        for p in paths:
            engine.load_segment(p)
    return out


@pytest.fixture(scope="module")
def ref_rows(files):
    """The restatement's per-glob rows per (flavour, filter), computed once and left unchanged."""
    from oracle import dataexpr as dx
    from tests import tagnames_ref as ref
    out = {}
    for fl, (paths, blobs) in files.items():
        for name, filt in td.FILTERS.items():
            pr = dx.parse_pushdown(json.dumps(td.request(filt)))
            out[fl, name] = ref.evaluate(pr, paths, td.GLOB_SIZE, sources=blobs)
    return out


def _rows(res):
    return list(zip(res.ts.tolist(), res.values.tolist(), res.tags, res.globs.tolist()))


def _same(got, want, merged, label):
    assert len(got) == len(want), f"{label}: {len(got)} rows vs {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], f"{label}: row {i} timestamp {g[0]} vs {w[0]}"
        assert np.float64(g[1]).tobytes() == np.float64(w[1]).tobytes(), f"{label}: row {i} value {g[1]} vs {w[1]}"
        assert set(g[2].items()) == set(w[2].items()), f"{label}: row {i} tags\n{g[2]}\nvs\n{w[2]}"
        assert g[3] == (0 if merged else w[3]), f"{label}: row {i} glob {g[3]} vs {w[3]}"


@pytest.mark.parametrize("flavour", ["double", "int"])
@pytest.mark.parametrize("filt", sorted(td.FILTERS))
def test_cases_equal_the_restatement(engine, files, ref_rows, flavour, filt):
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from tests import tagnames_ref as ref
    paths, _ = files[flavour]
    req = json.dumps(td.request(td.FILTERS[filt]))
    want = ref_rows[flavour, filt]
    for flags, merged in ((LK_PER_GLOB_ROWS, False), (LK_MERGED, True)):
        res = engine.eval_pushdown(req, paths, td.GLOB_SIZE, flags)
        _same(_rows(res), want, merged, f"{flavour} {filt} merged={merged}")
        tn = res.stats["tag_names"]
        assert tn["found"] == ref.name_count(want) and tn["rows"] == len(want)
        if want:
            assert tn["tiles_pruned"] > 0, tn       # later tiles and files find most columns already in first[]
            assert tn["tiles_walked"] > 0


def test_reverse_sort(engine, files):
    from lakeside_amd import LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx
    from tests import tagnames_ref as ref
    paths, blobs = files["double"]
    req = json.dumps(td.request(td.FILTERS["keep"], reverse=True))
    want = ref.evaluate(dx.parse_pushdown(req), paths, td.GLOB_SIZE, sources=blobs)
    got = _rows(engine.eval_pushdown(req, paths, td.GLOB_SIZE, LK_PER_GLOB_ROWS))
    _same(got, want, False, "reverseSort")
    assert [g[0] for g in got] == sorted((g[0] for g in got), reverse=True) and len(got) > 3


def test_queryapi_evaluate_tag_query(engine, files, ref_rows):
    from lakeside_amd import queryapi, synth
    paths, _ = files["double"]
    be = {"id": "A", "dataset": "logs", "filter": td.FILTERS["keep"],
          "chart": {"aggregation": "count", "groupBys": [], "type": "count"}}
    segs = [synth.segment_request(i, hour=0) for i in range(td.NFILES)]
    want = ref_rows["double", "keep"]
    got = queryapi.evaluate_tag_query(engine, be, segs, paths, glob_size=td.GLOB_SIZE)
    assert got == [{"message": w[2]} for w in want]
    assert "chart" in be                                            # the caller's expression is left as it was
    few = queryapi.evaluate_tag_query(engine, be, segs, paths, limit=2, glob_size=td.GLOB_SIZE)
    assert few == got[:2] and len(got) > 2
    # with a tagDataType the request is the tag-value query: `exists` ANDed on, (value, count) rows
    vals = queryapi.evaluate_tag_query(engine, be, segs, paths, tag_data_type={"tagName": "only.second", "dataType": "string"},
                                       glob_size=td.GLOB_SIZE)
    assert {m["message"]["only.second"] for m in vals} == {"s0", "s1", "s2", "s3"}
    assert all("count" in m["message"] for m in vals)


def _refused(engine, req, paths, why, glob_size=td.GLOB_SIZE):
    from lakeside_amd import LK_PER_GLOB_ROWS
    from lakeside_amd.evaluator import LakesideError
    with pytest.raises(LakesideError) as e:
        engine.eval_pushdown(json.dumps(req), paths, glob_size, LK_PER_GLOB_ROWS)
    assert e.value.code == UNSUPPORTED and why in str(e.value), str(e.value)
    return str(e.value)


def test_refusals(engine, files, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    paths, _ = files["double"]
    keep = td.FILTERS["keep"]
    assert PREFIX + "processor.tagNameCompressionEnabled" in _refused(engine, td.request(keep, processor=False), paths,
                                                                      "tagNameCompressionEnabled")
    n = 50
    ts = pa.array(synth.T0 + np.arange(n, dtype=np.int64), pa.int64())
    val = pa.array(np.arange(n, dtype=np.float64), pa.float64())
    tag = pa.array([f"t{k % 3}" for k in range(n)], pa.string())
    shapes = {
        "name_first": (pa.table({"a.tag": tag, td.TS: ts, td.VALUE: val}), PREFIX + "the first column of glob 0 is a.tag"),
        "string_second": (pa.table({td.TS: ts, "a.tag": tag, td.VALUE: val}), PREFIX + "the second column a.tag of glob 0"),
        "unloaded": (pa.table({td.TS: ts, td.VALUE: val, "a.tag": tag,
                               "a.list": pa.array([[k] for k in range(n)], pa.list_(pa.int64()))}), "a.list"),
    }
    for name, (t, why) in shapes.items():
        p = str(tmp_path / f"{name}.parquet")
        pq.write_table(t, p)
        engine.load_segment(p)
        _refused(engine, td.request(synth.leaf("a.tag", "exists"), nfiles=1), [p], why)
        engine.evict(p)


def test_dist_world1_is_refused(files):
    from lakeside_amd.evaluator import Engine, LakesideError
    paths, _ = files["double"]
    eng = Engine(0)
    try:
        eng.comm_init_host(1, 0, allgather=lambda b: [b])   # world 1 over the host transport
        with pytest.raises(LakesideError) as e:
            eng.eval_pushdown_dist(json.dumps(td.request(td.FILTERS["keep"])), paths, None, td.GLOB_SIZE)
        assert e.value.code == UNSUPPORTED and PREFIX + "lk_eval_pushdown_dist" in str(e.value)
    finally:
        eng.close()
