"""scan_clu's pinned tiles merged from the clustered copy's per-(tile, code) aggregates (`cagg`, built by clu_build
with the reduction scan_clu streams with: csrc/clu_reduce.hpp) on the MI355X.

Every case is evaluated three ways, per glob and merged, each against the oracle:
  * as it stands (pinned tiles merge `cagg`);
  * with LK_NO_CLU_AGG=1 (pinned tiles stream their value ranges): the same rows BIT FOR BIT in timestamps, tags and
    value bits, for SUM, MIN and MAX, real values included -- the aggregates are what the stream hands global_merge;
  * with LK_NO_CLUSTER=1 (scan_lean / scan_tiles), with tests/test_gpu_clustered.py's bars: bit for bit for MIN / MAX
    and integral sums; real sums both within the suite's SUM bar (1 ulp of the correctly rounded value) of the oracle.

Segments are 2^19 rows in 65,536-row pages: 8 or 9 tiles (the loader also cuts a tile where a stream has more runs
than the kernels stage, so the count is read from `stats`) of up to 7.5 minutes.  A 1 h step on the segment's hour
pins every tile; a step near a tile's span splits those that hold a bucket boundary.

Plan bytes (LK_PLAN_BYTES) are the evidence of the path: a pinned tile that merges aggregates counts the 128-B lines
of the `cagg` entries it merges and no value line.  A range of n values counts between 8 n and 8 n + 254 B of lines
when streamed, and a tile's merged `cagg` entries lie in at most as many lines as there are passing codes, so with
every one of T tiles pinned, V passing values and P passing names:
    8 V - 128 P T  <=  D = plan_bytes(LK_NO_CLU_AGG=1) - plan_bytes  <=  8 V + 254 P T
(the issue's "by at least the value ranges' bytes", less the `cagg` lines the new path does read).  Every pinned tile
with a few dozen passing values adds a positive term to D and a split tile adds none, so over one segment and filter
0 < D(call) < D(all-pinned call) says that the call had tiles of both kinds.  The files of tests/nonfinite_data.py are
one tile each: there a split call is all split, and D = 0."""
import json

import numpy as np
import pytest

from tests import nonfinite_data as nf
from tests.parity import assert_rows_equal
from tests.test_gpu_clustered import ALL16, NAME, _bits, _cells, _Env, _one, _segment, _with, odd_file  # noqa: F401

pytestmark = pytest.mark.gpu

HOUR = 3_600_000
TILE = 1 << 16
MODES = (("agg", {}), ("noagg", {"LK_NO_CLU_AGG": 1}), ("off", {"LK_NO_CLUSTER": 1}))


def _three(engine, keys, blobs, segs, filt, agg, gbs=(), glob_size=10, integral=True, label=""):
    """{mode: (per-glob result, merged result)} after the oracle and the cross-mode comparisons."""
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
    for mode, env in MODES:
        with _Env(**env):
            pg = engine.eval_pushdown(req, keys, glob_size, LK_PER_GLOB_ROWS | LK_PLAN_BYTES)
            mg = engine.eval_pushdown(req, keys, glob_size, LK_MERGED | LK_PLAN_BYTES)
        for gi, (g, w) in enumerate(zip(pg.per_glob(len(want_pg)), want_pg)):
            assert_rows_equal(g, w, agg, f"{label} {mode} glob {gi}")
        assert_rows_equal(mg.rows(), want_mg, agg, f"{label} {mode} merged")
        for r in (pg, mg):
            if mode == "off":
                assert r.stats["clustered"] == 0 and r.stats["clustered_tiles"] == 0, r.stats
            else:
                assert r.stats["clustered"] == 1 and r.stats["clustered_tiles"] > 0, (label, mode, r.stats)
        out[mode] = (pg, mg)
    for a, b, c in zip(out["agg"], out["noagg"], out["off"]):
        assert a.ts.tolist() == b.ts.tolist() and a.tags == b.tags, label
        assert _bits(a.values) == _bits(b.values), f"{label}: LK_NO_CLU_AGG rows differ"
        assert a.ts.tolist() == c.ts.tolist() and a.tags == c.tags, label
        if agg != "sum" or integral:
            assert _bits(a.values) == _bits(c.values), f"{label}: LK_NO_CLUSTER rows differ"
    return out


def _pb(out):
    """Plan bytes of the merged evaluation: (aggregates, LK_NO_CLU_AGG=1)."""
    return out["agg"][1].stats["plan_bytes"], out["noagg"][1].stats["plan_bytes"]


_counts = {}


def _name_counts(blob):
    """{name: rows} of a segment."""
    import io

    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    k = id(blob)
    if k not in _counts:
        names = np.asarray(pq.read_table(io.BytesIO(blob), columns=[dx.NAME]).column(dx.NAME).to_pylist(), dtype=str)
        u, n = np.unique(names, return_counts=True)
        _counts[k] = (blob, dict(zip(u.tolist(), n.tolist())))
    return _counts[k][1]


def _assert_all_pinned(out, blob, names, label):
    """Every tile merged its aggregates: D within the docstring's bounds.  Returns D."""
    st = out["agg"][1].stats
    T = st["tiles"]
    assert st["clustered_tiles"] == T, (label, st)
    V = sum(_name_counts(blob)[n] for n in names)
    a, b = _pb(out)
    assert 8 * V - 128 * len(names) * T <= b - a <= 8 * V + 254 * len(names) * T, (label, a, b, V, T)
    assert a < b
    return b - a


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_all_pinned_one_name(engine, agg):
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    segs = _with(segs, HOUR)
    out = _three(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "metric_07"), agg, label=f"pinned eq {agg}")
    _assert_all_pinned(out, blobs[0], ["metric_07"], f"pinned eq {agg}")
    assert out["agg"][1].stats["tiles"] >= 8 and len(out["agg"][1]) == 1


@pytest.mark.parametrize("names", [["metric_03", "metric_07", "metric_11"], ALL16], ids=["in3", "all16"])
def test_all_pinned_in(engine, names):
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    segs = _with(segs, HOUR)
    for agg in ("sum", "min", "max"):
        out = _three(engine, keys, blobs, segs, synth.leaf(NAME, "in", *names), agg, [NAME], label=f"in {len(names)} {agg}")
        _assert_all_pinned(out, blobs[0], names, f"in {len(names)} {agg}")
        assert len(out["agg"][1]) == len(names)
    # ungrouped: the passing codes of a tile share one cell
    out = _three(engine, keys, blobs, segs, synth.leaf(NAME, "in", *names), "sum", label=f"in {len(names)} one cell")
    assert len(out["agg"][1]) == 1


def test_real_values_and_compensated_integers(engine):
    """value_mode=1 (lognormal reals) for SUM / MIN / MAX, then the integral data with the exact-sum shortcut off (the
    compensated form of the same `hi`)."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 2, rows=1 << 19, value_mode=1, page_rows=TILE)
    segs = _with(segs, HOUR)
    for agg in ("sum", "min", "max"):
        for filt, gbs in ((synth.leaf(NAME, "eq", "metric_07"), ()), (synth.leaf(NAME, "in", *ALL16), (NAME,))):
            out = _three(engine, keys, blobs, segs, filt, agg, gbs, integral=False, label=f"real {agg} {len(gbs)}")
            assert out["agg"][1].stats["exact_sum"] == 0
            a, b = _pb(out)
            assert a < b
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    segs = _with(segs, HOUR)
    with _Env(LK_NO_EXACT_SUM=1):
        out = _three(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "metric_07"), "sum", label="no exact sum")
        assert out["agg"][1].stats["exact_sum"] == 0
        a, b = _pb(out)
        assert a < b


def test_pinned_and_split_in_one_call(engine):
    """Tiles of up to 7.5 min at a 10 min step: tiles that hold a multiple of 10 min are split, the others pinned.
    Both kinds occur: 0 < D < D of the all-pinned call (module docstring), over all of the segment's tiles."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    names = ["metric_03", "metric_11"]
    for agg in ("sum", "max"):
        allp = _three(engine, keys, blobs, _with(segs, HOUR), synth.leaf(NAME, "in", *names), agg, [NAME],
                      label=f"all pinned {agg}")
        d_all = _assert_all_pinned(allp, blobs[0], names, f"all pinned {agg}")
        out = _three(engine, keys, blobs, _with(segs, 600_000), synth.leaf(NAME, "in", *names), agg, [NAME],
                     label=f"mixed kinds {agg}")
        st = out["agg"][1].stats
        assert st["clustered_tiles"] == st["tiles"] == allp["agg"][1].stats["tiles"] >= 8, st
        a, b = _pb(out)
        assert 0 < b - a < d_all, (a, b, d_all)
        assert len(out["agg"][1]) == 6 * len(names)


def test_window_cuts_tiles(engine):
    """A 1 h step with the window cut 7 s / 11 s inside the hour: the first and the last tile are no longer inside the
    window, so they are split tiles (rows outside the window dropped) and must not merge their aggregates: the rows
    are the oracle's and the streamed path's, they differ from the whole hour's, and D falls below the whole hour's."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    names = ["metric_07", "metric_08"]
    for agg in ("sum", "min", "max"):
        full = _three(engine, keys, blobs, _with(segs, HOUR), synth.leaf(NAME, "in", *names), agg, [NAME],
                      label=f"whole window {agg}")
        d_all = _assert_all_pinned(full, blobs[0], names, f"whole window {agg}")
        out = _three(engine, keys, blobs, _with(segs, HOUR, (7000, 11000)), synth.leaf(NAME, "in", *names), agg, [NAME],
                     label=f"cut window {agg}")
        a, b = _pb(out)
        assert 0 < b - a < d_all, (a, b, d_all)
        if agg == "sum":   # the cut did drop rows of the end tiles
            assert _bits(full["agg"][1].values) != _bits(out["agg"][1].values)


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_absent_short_and_one_code_tiles(engine, odd_file, agg):
    """tests/test_gpu_clustered.py's odd file (a name absent from most tiles, single-code tiles, a last tile whose rows
    are no multiple of 64; tiles of about 31 s within ten minutes): every tile pinned at a 1 h step, and the 1 m
    step's pinned and split tiles."""
    from lakeside_amd import synth
    path, blob = odd_file
    for step in (HOUR, 60_000):
        segs = [synth.segment_request(0, step=step, hour=0)]
        for names in (["rare"], ["solo"], ["rare", "solo", "a", "b"]):
            out = _three(engine, [path], [blob], segs, synth.leaf(NAME, "in", *names), agg, [NAME],
                         label=f"odd {names} {agg} {step}")
            assert out["agg"][1].stats["tiles"] >= 8
            a, b = _pb(out)
            assert (a < b) if step == HOUR else (a <= b)   # (`rare` lies in one tile, which the 1 m step may split)


@pytest.mark.parametrize("step", [3_600_000, 2_400_000])
@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_nonfinite(engine, tmp_path_factory, agg, step):
    """tests/nonfinite_data.py (+-inf, NaN, -0.0, overflowing sums; one 4,096-row tile per file): pinned at a 1 h step
    (aggregates), split at 40 min.  A NaN under MIN raises FLAG_MIN_NAN from the stored per-code mask: the rows (which
    the flag's re-run decides) are the same either way, and the classes are the oracle's."""
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    from tests import test_gpu_clustered as tc
    if "nf" not in tc._segs:
        paths, blobs = nf.write_files(tmp_path_factory.mktemp("clu_agg_nf"), "clean")
        for p in paths:
            engine.load_segment(p)
        tc._segs["nf"] = (paths, blobs)
    paths, blobs = tc._segs["nf"]
    out = _three(engine, paths, blobs, nf.segments(step), nf.all_names(), agg, [NAME], glob_size=nf.GLOB, integral=False,
                 label=f"nonfinite {agg} {step}")
    a, b = _pb(out)
    assert out["agg"][1].stats["tiles"] == out["agg"][1].stats["clustered_tiles"] == nf.NFILES   # one tile per file
    assert (a < b) if step == 3_600_000 else (a == b)   # all pinned / all split: the same bytes both ways
    req = json.dumps(synth.pushdown(nf.all_names(), nf.segments(step), agg, [NAME]))
    cells = dx.evaluate_glob_cells(dx.parse_pushdown(req), nf.GLOB, paths, sources=blobs)
    want = dx.merge_glob_cells(dx.parse_pushdown(req), cells)

    def classes(rows):
        zero = ("-0", "+0")
        return sorted((t, tags.get("name"), "0" if agg == "sum" and nf.value_class(v) in zero else nf.value_class(v))
                      for t, v, tags in rows)
    for mode in ("agg", "noagg"):
        assert classes(out[mode][1].rows()) == classes(want), mode
    # MIN over the NaN rows of `naninf`: the same bits either way (checked in _three), and a NaN row exists
    if agg == "min":
        assert any(t.get("name") == "naninf" for t in out["agg"][1].tags)


@pytest.mark.timeout(120)
def test_distributed_world1_loopback(engine):
    from lakeside_amd import synth
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    segs = _with(segs, HOUR)
    req = json.dumps(synth.pushdown(synth.leaf(NAME, "in", "metric_07", "metric_09"), segs, "sum", [NAME]))
    pr = dx.parse_pushdown(req)
    want = dx.merge_glob_cells(pr, dx.evaluate_glob_cells(pr, 10, keys, sources=blobs))
    with _Env(LK_COMM_LOOPBACK=1):
        eng = Engine(0)
        try:
            eng.comm_init(Engine.unique_id(), 1, 0)
            eng.put_segment(keys[0], blobs[0])
            res = eng.eval_pushdown_dist(req, keys, None, 10)
            with _Env(LK_NO_CLU_AGG=1):
                ref = eng.eval_pushdown_dist(req, keys, None, 10)
            for r in (res, ref):
                assert r.stats["clustered"] == 1, r.stats
                assert_rows_equal(r.rows(), want, "sum", "dist loopback")
            assert res.ts.tolist() == ref.ts.tolist() and res.tags == ref.tags and _bits(res.values) == _bits(ref.values)
        finally:
            eng.close()


def test_no_copy_behaves_as_before(engine):
    """{"cluster_values": false} and a segment with NULLs (no copy): nothing is built or counted, no tile is taken, the
    toggle changes nothing, and the rows are the engine's with the copy."""
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES, synth
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    segs = _with(segs, HOUR)
    req = json.dumps(synth.pushdown(synth.leaf(NAME, "in", "metric_02", "metric_07"), segs, "sum", [NAME]))
    on = engine.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES)
    assert on.stats["clustered"] == 1
    eng = Engine(0, cluster_values=False)
    try:
        eng.put_segment(keys[0], blobs[0])
        assert eng.stats["clu_bytes"] == 0
        res = []
        for env in ({}, {"LK_NO_CLU_AGG": 1}):
            with _Env(**env):
                res.append(eng.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES))
        for off in res:
            assert off.stats["clustered"] == 0 and off.stats["clustered_tiles"] == 0
            assert off.ts.tolist() == on.ts.tolist() and off.tags == on.tags and _bits(off.values) == _bits(on.values)
        assert res[0].stats["plan_bytes"] == res[1].stats["plan_bytes"]
        s = synth.make_segment(synth.segment_spec(1, rows=1 << 18, null_frac=0.001, rg_rows=1 << 17, page_rows=TILE))
        blob = s.bytes()
        eng2 = Engine(0)
        try:
            eng2.put_segment_ptr("nulls", s.ptr, s.size)
            s.free()
            assert eng2.stats["clu_bytes"] == 0 and eng2.stats["clu_alloc_failed"] == 0
            rq = json.dumps(synth.pushdown(synth.leaf(NAME, "eq", "metric_07"), [synth.segment_request(1, step=HOUR)], "sum", []))
            pr = dx.parse_pushdown(rq)
            want = dx.merge_glob_cells(pr, dx.evaluate_glob_cells(pr, 10, ["nulls"], sources=[blob]))
            for env in ({}, {"LK_NO_CLU_AGG": 1}):
                with _Env(**env):
                    r = eng2.eval_pushdown(rq, ["nulls"], 10, LK_MERGED | LK_PLAN_BYTES)
                assert r.stats["clustered"] == 0 and r.stats["clustered_tiles"] == 0, r.stats
                assert_rows_equal(r.rows(), want, "sum", "nulls")
        finally:
            eng2.close()
    finally:
        eng.close()


def test_engine_clu_bytes_is_the_sum_over_tiles(tmp_path_factory):
    """A file of tests/nonfinite_data.py is one tile of 4,096 rows with a 12-name dictionary: one block of
    clu_block_bytes(4096, 12) after the 128-B-aligned descriptor array (the layout of csrc/layout.hpp in Python
    integers, as tests/test_clu_layout_cpu.py pins the function); three files, three times that."""
    from lakeside_amd.evaluator import Engine

    def align(x, a):
        return (x + a - 1) // a * a
    paths, blobs = nf.write_files(tmp_path_factory.mktemp("clu_agg_size"), "clean")
    per_file = align(1 * 16, 128) + align(288 + 32 * len(nf.KINDS) + 10 * nf.ROWS, 128)
    eng = Engine(0)
    try:
        for i, p in enumerate(paths):
            eng.load_segment(p)
            assert eng.stats["clu_bytes"] == (i + 1) * per_file, (i, eng.stats)
        assert eng.segment_bytes >= eng.stats["clu_bytes"] + sum(len(b) for b in blobs)
    finally:
        eng.close()
