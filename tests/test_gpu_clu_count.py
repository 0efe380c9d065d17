"""COUNT and AVG charts answered from the name-clustered value copy (scan_clu, clu_kernel.hpp) on the MI355X.

COUNT reads no value: a pinned tile's count of a code is a difference of two `cpref` entries, a whole sub-block's a
difference of two `csub` entries, and only a sub-block that holds a bucket boundary has its `crows` (2 B per element)
looked at.  AVG is scan_clu<AGG_SUM> with the table's `rows` plane kept.

Every case is evaluated per glob and merged, against the oracle (tests/parity.py), in four modes: as it stands, with
LK_NO_CLU_AGG=1, with LK_NO_CLU_SUB=1 and with LK_NO_CLUSTER=1 (scan_lean / scan_tiles).  `clustered` is 1 and
`clustered_tiles` above 0 in the first three and 0 in the last.  COUNT rows are the same BIT FOR BIT in the four
modes, AVG rows too where the values are integral; AVG of real values holds the suite's bar against the oracle in each
mode (the double-double partials combine in another order).

The segments are the ones tests/test_gpu_clustered.py and tests/test_gpu_clu_sub.py cache."""
import json

import numpy as np
import pytest

from tests import nonfinite_data as nf
from tests.parity import assert_rows_equal
from tests.test_gpu_clu_sub import CRAFT_STEP, FILTERS, TILE, _sub_counts, crafted  # noqa: F401
from tests.test_gpu_clustered import ALL16, NAME, _bits, _cells, _Env, _one, _segment, _segs, _with, odd_file  # noqa: F401

pytestmark = pytest.mark.gpu

HOUR = 3_600_000
MODES = (("on", {}), ("noagg", {"LK_NO_CLU_AGG": 1}), ("nosub", {"LK_NO_CLU_SUB": 1}), ("off", {"LK_NO_CLUSTER": 1}))
AGGS = ["count", "avg"]


def _four(engine, keys, blobs, segs, filt, agg, gbs=(), glob_size=10, integral=True, label=""):
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
                assert r.stats["clustered"] == 0 and r.stats["clustered_tiles"] == 0, (label, r.stats)
            else:
                assert r.stats["clustered"] == 1 and r.stats["clustered_tiles"] > 0, (label, mode, r.stats)
        out[mode] = (pg, mg)
    for mode in ("noagg", "nosub", "off"):
        for a, b in zip(out["on"], out[mode]):
            assert a.ts.tolist() == b.ts.tolist() and a.tags == b.tags, (label, mode)
            if agg == "count" or integral:
                assert _bits(a.values) == _bits(b.values), f"{label}: {mode} rows differ"
    return out


def _merged(engine, keys, segs, filt, agg, gbs=(), glob_size=10, **env):
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES, synth
    req = json.dumps(synth.pushdown(filt, segs, agg, list(gbs)))
    with _Env(**env):
        return engine.eval_pushdown(req, keys, glob_size, LK_MERGED | LK_PLAN_BYTES)


@pytest.mark.parametrize("agg", AGGS)
def test_minute_step(engine, agg):
    """2^20 rows in 4,096-row pages at the 1 m step: most tiles pinned (cpref alone), those holding a minute boundary
    split with one sub-block each.  Every code by name, one name, and a name no row has."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    out = _four(engine, keys, blobs, segs, synth.leaf(NAME, "in", *ALL16), agg, [NAME], label=f"all16 {agg}")
    mg = out["on"][1]
    assert len({t["name"] for t in mg.tags}) == 16 and mg.stats["clustered_tiles"] == mg.stats["tiles"]
    out = _four(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "metric_07"), agg, label=f"eq 1m {agg}")
    assert len(out["on"][1]) == 60
    out = _four(engine, keys, blobs, segs, synth.leaf(NAME, "eq", "no_such_metric"), agg, label=f"absent {agg}")
    assert len(out["on"][1]) == 0


@pytest.mark.parametrize("step", [600_000, 300_000])
@pytest.mark.parametrize("agg", AGGS)
def test_sub_blocks(engine, agg, step):
    """2^19 rows in 65,536-row pages: 16 sub-blocks a tile, one boundary in a split tile at 10 min, one or two at
    5 min.  COUNT reads fewer bytes with the area than with its ranges streamed whole."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    for name, filt, gbs in FILTERS:
        out = _four(engine, keys, blobs, _with(segs, step), filt(synth), agg, gbs, label=f"sub {name} {agg} {step}")
        st = out["on"][1].stats
        assert st["clustered_tiles"] == st["tiles"] >= 8, st
        assert out["on"][1].stats["plan_bytes"] < out["nosub"][1].stats["plan_bytes"]


@pytest.mark.parametrize("step,window", [(20000, None), (30000, None), (30000, (7000, 11000)), (60000, (61000, 1795000))])
def test_short_steps_and_cut_windows(engine, step, window):
    """14 s tiles at 20 s / 30 s steps (one to three boundaries in many tiles) and windows that cut tiles at both
    ends: the classes outside the window are dropped from counts as they are from sums."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    for agg in AGGS:
        _four(engine, keys, blobs, _with(segs, step, window), synth.leaf(NAME, "in", "metric_03", "metric_11"), agg, [NAME],
              label=f"split {step} {window} {agg}")


@pytest.mark.parametrize("step", [60_000, HOUR])
@pytest.mark.parametrize("agg", AGGS)
def test_odd_file(engine, odd_file, agg, step):
    """A name absent from most tiles, single-code tiles and a last tile whose rows are no multiple of 64."""
    from lakeside_amd import synth
    path, blob = odd_file
    segs = [synth.segment_request(0, step=step, hour=0)]
    for names in (["rare"], ["solo"], ["rare", "solo", "a", "b"]):
        out = _four(engine, [path], [blob], segs, synth.leaf(NAME, "in", *names), agg, [NAME], label=f"odd {names} {agg} {step}")
        assert out["on"][1].stats["tiles"] >= 8
        if agg == "count" and len(names) == 4:
            assert int(np.sum(out["on"][1].values)) == 20011


@pytest.mark.parametrize("agg", AGGS)
def test_mixed_call(engine, agg):
    """A clean segment (scan_clu) and one with 5 % NULLs (no copy: scan_lean / scan_tiles) in one call and one table.
    The table is not lean here: its `rows` and `cnt` planes differ, and scan_clu adds to both."""
    from lakeside_amd import synth
    k0, b0 = _segment(engine, 0)
    k1, b1 = _segment(engine, 1, rows=1 << 19, value_mode=0, null_frac=0.05)
    segs = [synth.segment_request(0), synth.segment_request(1)]
    out = _four(engine, [k0, k1], [b0, b1], segs, synth.leaf(NAME, "eq", "metric_07"), agg, glob_size=1, label=f"mixed {agg}")
    for mode in ("on", "noagg", "nosub"):
        st = out[mode][1].stats
        assert 0 < st["clustered_tiles"] < st["tiles"], (mode, st)


@pytest.mark.parametrize("step", [60_000, 600_000])
def test_avg_of_real_values(engine, step):
    """value_mode=1 (lognormal reals, compensated sums): AVG holds the suite's bar against the oracle in each mode."""
    from lakeside_amd import synth
    if step == 60_000:
        keys, blobs, segs = _one(engine, 2, value_mode=1)
    else:
        keys, blobs, segs = _one(engine, 2, rows=1 << 19, value_mode=1, page_rows=TILE)
    for name, filt, gbs in FILTERS[:2]:
        out = _four(engine, keys, blobs, _with(segs, step), filt(synth), "avg", gbs, integral=False, label=f"real {name} {step}")
        assert out["on"][1].stats["exact_sum"] == 0


@pytest.mark.parametrize("agg", AGGS)
def test_nonfinite(engine, tmp_path_factory, agg):
    """tests/nonfinite_data.py at a 1 h step (one pinned 4,096-row tile per file): NaN and +-inf values are counted
    like any other, and AVG reports what the oracle reports, class by class."""
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    if "nf" not in _segs:
        paths, blobs = nf.write_files(tmp_path_factory.mktemp("clu_count_nf"), "clean")
        for p in paths:
            engine.load_segment(p)
        _segs["nf"] = (paths, blobs)
    paths, blobs = _segs["nf"]
    out = _four(engine, paths, blobs, nf.segments(HOUR), nf.all_names(), agg, [NAME], glob_size=nf.GLOB, integral=False,
                label=f"nonfinite {agg}")
    req = json.dumps(synth.pushdown(nf.all_names(), nf.segments(HOUR), agg, [NAME]))
    pr = dx.parse_pushdown(req)
    want = dx.merge_glob_cells(pr, dx.evaluate_glob_cells(pr, nf.GLOB, paths, sources=blobs))
    if agg == "count":
        got = {(t, tags.get("name")): v for t, v, tags in out["on"][1].rows()}
        assert got == {(t, tags.get("name")): v for t, v, tags in want}
        assert sum(got.values()) == nf.ROWS * len(paths)   # no row is left out for its value
    else:
        def classes(rows):
            zero = ("-0", "+0")
            return sorted((t, tags.get("name"), "0" if nf.value_class(v) in zero else nf.value_class(v)) for t, v, tags in rows)
        for mode, _ in MODES:
            assert classes(out[mode][1].rows()) == classes(want), mode


def test_plan_bytes_pinned(engine):
    """An all-pinned call (1 h step on the hour): COUNT reads descriptors, lookups, the truth word and cpref whatever
    LK_NO_CLU_AGG says, and SUM reads at least one 128-B line of cagg more in every tile that holds a passing code
    (here every tile: the generator spreads all 16 names over each)."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    filt = synth.leaf(NAME, "in", "metric_02", "metric_07")
    cnt = _merged(engine, keys, _with(segs, HOUR), filt, "count", [NAME])
    cnt_noagg = _merged(engine, keys, _with(segs, HOUR), filt, "count", [NAME], LK_NO_CLU_AGG=1)
    sm = _merged(engine, keys, _with(segs, HOUR), filt, "sum", [NAME])
    tiles = cnt.stats["tiles"]
    print("pinned plan bytes: count", cnt.stats["plan_bytes"], "count LK_NO_CLU_AGG", cnt_noagg.stats["plan_bytes"], "sum",
          sm.stats["plan_bytes"], "tiles", tiles)
    assert cnt.stats["clustered"] == 1 and cnt.stats["clustered_tiles"] == tiles == sm.stats["clustered_tiles"] >= 8
    assert cnt.stats["plan_bytes"] == cnt_noagg.stats["plan_bytes"] > 0
    assert _bits(cnt.values) == _bits(cnt_noagg.values)
    assert sm.stats["plan_bytes"] - cnt.stats["plan_bytes"] >= 128 * tiles


def test_plan_bytes_split(engine, crafted):
    """tests/test_gpu_clu_sub.py's crafted tile (one split tile of four sub-blocks, the third one straddling).  Streamed
    whole, SUM counts the lines of 8 n value bytes and 2 n row-index bytes for n passing elements and COUNT only the
    latter, the rest alike: the difference is at least 8 n.  With the area COUNT reads two csub lines per code and the
    straddler's row indices: less than its own LK_NO_CLU_SUB figure."""
    from lakeside_amd import synth
    path, blob, names = crafted["int"]
    segs = [synth.segment_request(0, step=CRAFT_STEP, hour=0)]
    counts = _sub_counts(blob)
    for passing in (["gap"], ["a", "gap", "fill"], ["a", "b", "gap", "fill"]):
        filt = synth.leaf(NAME, "in", *passing)
        n = sum(sum(counts[p]) for p in passing)
        cnt_whole = _merged(engine, [path], segs, filt, "count", [NAME], LK_NO_CLU_SUB=1)
        sum_whole = _merged(engine, [path], segs, filt, "sum", [NAME], LK_NO_CLU_SUB=1)
        cnt_area = _merged(engine, [path], segs, filt, "count", [NAME])
        print("split plan bytes", passing, "n", n, "count whole", cnt_whole.stats["plan_bytes"], "sum whole",
              sum_whole.stats["plan_bytes"], "count area", cnt_area.stats["plan_bytes"])
        for r in (cnt_whole, sum_whole, cnt_area):
            assert r.stats["clustered"] == 1 and r.stats["tiles"] == r.stats["clustered_tiles"] == 1, r.stats
        assert int(np.sum(cnt_area.values)) == n and _bits(cnt_area.values) == _bits(cnt_whole.values)
        assert sum_whole.stats["plan_bytes"] - cnt_whole.stats["plan_bytes"] >= 8 * n
        assert cnt_area.stats["plan_bytes"] < cnt_whole.stats["plan_bytes"]


@pytest.mark.timeout(120)
def test_distributed_world1_loopback(engine):
    """lk_eval_pushdown_dist at world 1 with the loopback data path counts from the copy too."""
    from lakeside_amd import synth
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    keys, blobs, segs = _one(engine)
    req = json.dumps(synth.pushdown(synth.leaf(NAME, "eq", "metric_07"), segs, "count", []))
    pr = dx.parse_pushdown(req)
    want = dx.merge_glob_cells(pr, dx.evaluate_glob_cells(pr, 10, keys, sources=blobs))
    with _Env(LK_COMM_LOOPBACK=1):
        eng = Engine(0)
        try:
            eng.comm_init(Engine.unique_id(), 1, 0)
            eng.put_segment(keys[0], blobs[0])
            res = eng.eval_pushdown_dist(req, keys, None, 10)
            assert res.stats["clustered"] == 1, res.stats
            assert_rows_equal(res.rows(), want, "count", "dist loopback count")
        finally:
            eng.close()


def test_formula_over_counts(engine):
    """`a / b * 100` over two count operands (one name over all 16): the rows with both operands counted from the copy
    are bit for bit those of scan_lean's counts."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine)
    ex = {"a": {"pushDown": synth.pushdown(synth.leaf(NAME, "eq", "metric_07"), segs, "count", []), "paths": keys},
          "b": {"pushDown": synth.pushdown(synth.leaf(NAME, "in", *ALL16), segs, "count", []), "paths": keys}}
    on = engine.eval_formula("a / b * 100", ex, 10)
    with _Env(LK_NO_CLUSTER=1):
        off = engine.eval_formula("a / b * 100", ex, 10)
    assert len(on) == 60 and on.ts.tolist() == off.ts.tolist() and on.tags == off.tags
    assert _bits(on.values) == _bits(off.values)
    assert all(0.0 < v < 100.0 for v in np.asarray(on.values).tolist())
    for e in ex.values():   # the operands themselves take the path
        r = engine.eval_pushdown(json.dumps(e["pushDown"]), keys, 10)
        assert r.stats["clustered"] == 1, r.stats


def test_option_off(engine):
    """{"cluster_values": false}: no copy, scan_clu never runs, the same counts and averages."""
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES, synth
    from lakeside_amd.evaluator import Engine
    keys, blobs, segs = _one(engine)
    eng = Engine(0, cluster_values=False)
    try:
        eng.put_segment(keys[0], blobs[0])
        assert eng.stats["clu_bytes"] == 0
        for agg in AGGS:
            req = json.dumps(synth.pushdown(synth.leaf(NAME, "in", "metric_02", "metric_07"), segs, agg, [NAME]))
            on = engine.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES)
            assert on.stats["clustered"] == 1 and on.stats["clustered_tiles"] > 0, on.stats
            off = eng.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES)
            assert off.stats["clustered"] == 0 and off.stats["clustered_tiles"] == 0, off.stats
            assert off.ts.tolist() == on.ts.tolist() and off.tags == on.tags and _bits(off.values) == _bits(on.values)
    finally:
        eng.close()
