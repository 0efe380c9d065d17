"""scan_clu over every chunk-dictionary size and index width the name-clustered value copy admits, and under name-only
filter trees, on the MI355X (files and trees: tests/clu_shapes.py, pinned on the CPU by tests/test_clu_shapes_cpu.py).

Every case is evaluated per glob and merged, each against the oracle with assert_rows_equal (tests/parity.py: the
suite's bar, no tolerance of its own), in five modes:
  on      as it stands                          noagg   LK_NO_CLU_AGG=1 (pinned tiles stream their ranges)
  nosub   LK_NO_CLU_SUB=1 (split tiles stream whole)
  off     LK_NO_CLUSTER=1 (scan_lean)           tiles   LK_NO_CLUSTER=1 LK_NO_LEAN=1 LK_NO_LEAN_SPLIT=1 (scan_tiles)
LK_NO_LEAN=1 alone only turns the lean table planes off (eval.cpp, setup_scan): scan_lean still takes the tiles.  What
keeps it from them is LK_NO_LEAN_SPLIT=1, so the fifth leg sets both, and `lean_split == 0` in its stats says that
scan_lean was not launched: every tile went to scan_tiles.
`clustered` is 1 and `clustered_tiles` equals `tiles` in the first three modes (under a cut window: the tiles that meet
it), both are 0 in the other two.  COUNT, MIN, MAX and sums / averages of integral values are the same rows BIT FOR BIT
in the five modes; sums of real values hold the oracle bar in each mode (their double-double partials combine in
another order).

Groups: (a) every code of every shape by name; (b) every code into one cell; (c) sub-blocks at the edges of the
dictionary; (d) NaN in the last code; (e) name-only filter trees.  A filter leaf over another field -- even one no
file has, which the glob compiles to `false` (QSeg::leaf_false) -- brings a second string column into the plan
(plan_filter), and plan_segments' clu_query wants exactly one: the planner declines such a tree, so the two of
clu_shapes.ABSENT_TREES assert `clustered == 0` and the oracle's rows (scan_clu's leaf_false term is unreachable)."""
import json

import numpy as np
import pytest

from tests import clu_shapes as cs
from tests import filter_trees as ft
from tests import nonfinite_data as nf
from tests.parity import assert_rows_equal
from tests.test_gpu_clustered import _bits, _Env

pytestmark = pytest.mark.gpu

NAME = cs.NAME
MODES = (("on", {}), ("noagg", {"LK_NO_CLU_AGG": 1}), ("nosub", {"LK_NO_CLU_SUB": 1}), ("off", {"LK_NO_CLUSTER": 1}),
         ("tiles", {"LK_NO_CLUSTER": 1, "LK_NO_LEAN": 1, "LK_NO_LEAN_SPLIT": 1}))
CLU_MODES = ("on", "noagg", "nosub")
AGGS = ["sum", "min", "max", "count", "avg"]
TEN_MIN = 10 * cs.MIN
A_SHAPES = [s for s in cs.SHAPES if not s.startswith("big_tile") and s != "uniform_65"]


class Shapes:
    def __init__(self, engine, dirpath):
        self.files = {}
        self.clu_growth = {}
        for k in cs.labels():
            f = cs.File(dirpath, *k)
            before = engine.stats["clu_bytes"]
            engine.load_segment(f.path)
            self.clu_growth[k] = engine.stats["clu_bytes"] - before
            self.files[k] = f
        self.cells = {}

    def get(self, shapes, flavour):
        return [self.files[(s, flavour)] for s in shapes]


@pytest.fixture(scope="module")
def shapes(engine, tmp_path_factory):
    return Shapes(engine, tmp_path_factory.mktemp("clu_shapes_gpu"))


def _segs(n, step, window=None):
    from lakeside_amd import synth
    segs = [synth.segment_request(j, step=step, hour=0) for j in range(n)]
    for s in segs:
        if window:
            s["startTs"] += window[0]
            s["endTs"] -= window[1]
    return segs


def _five(engine, sh, fs, step, filt, agg, gbs=(), glob_size=10, window=None, taken=True, label=""):
    """{mode: (per-glob result, merged result)} of one request over the files `fs`, after the oracle, the stats and the
    cross-mode comparisons of the module docstring."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS, LK_PLAN_BYTES, synth
    from oracle import dataexpr as dx
    keys, blobs = [f.path for f in fs], [f.blob for f in fs]
    segs = _segs(len(fs), step, window)
    req = json.dumps(synth.pushdown(filt, segs, agg, list(gbs)))
    ck = (tuple(keys), json.dumps(filt, sort_keys=True), tuple(gbs), step, window, glob_size)
    pr = dx.parse_pushdown(req)
    if ck not in sh.cells:
        sh.cells[ck] = dx.evaluate_glob_cells(pr, glob_size, keys, sources=blobs)
    cells = sh.cells[ck]
    want_pg = [[(c.ts, c.agg_value(agg), c.tags) for c in g] for g in cells]
    want_mg = dx.merge_glob_cells(pr, cells)
    integral = all(f.flavour == "int" for f in fs)
    # (a filter no row passes may leave the call without a cell space: then nothing is launched at all)
    empty = not any(len(g) for g in cells)
    out = {"want": (want_pg, want_mg)}
    for mode, env in MODES:
        with _Env(**env):
            pg = engine.eval_pushdown(req, keys, glob_size, LK_PER_GLOB_ROWS | LK_PLAN_BYTES)
            mg = engine.eval_pushdown(req, keys, glob_size, LK_MERGED | LK_PLAN_BYTES)
        for gi, (g, w) in enumerate(zip(pg.per_glob(len(want_pg)), want_pg)):
            assert_rows_equal(g, w, agg, f"{label} {mode} glob {gi}")
        assert_rows_equal(mg.rows(), want_mg, agg, f"{label} {mode} merged")
        for r in (pg, mg):
            st = r.stats
            if mode in CLU_MODES and taken and empty and st["clustered"] == 0:
                assert st["clustered_tiles"] == 0, (label, mode, st)
            elif mode in CLU_MODES and taken:
                assert st["clustered"] == 1, (label, mode, st)
                if window is None:
                    assert st["clustered_tiles"] == st["tiles"] > 0, (label, mode, st)
                else:   # the tiles that meet the window: the files' last few rows may lie in a tile of their own
                    assert st["tiles"] - 2 * len(fs) <= st["clustered_tiles"] <= st["tiles"], (label, mode, st)
                    assert st["clustered_tiles"] > 0
            else:
                assert st["clustered"] == 0 and st["clustered_tiles"] == 0, (label, mode, st)
            if mode == "tiles":
                assert st["lean_split"] == 0, (label, st)   # scan_lean was not launched: scan_tiles took every tile
            elif mode == "off" and taken:
                assert st["lean_split"] >= 1, (label, st)   # scan_lean was
        out[mode] = (pg, mg)
    for mode, _ in MODES[1:]:
        for a, b in zip(out["on"], out[mode]):
            assert a.ts.tolist() == b.ts.tolist() and a.tags == b.tags, (label, mode)
            if agg in ("count", "min", "max") or integral:
                assert _bits(a.values) == _bits(b.values), f"{label}: {mode} rows differ from the clustered path's"
    return out


def _all(fs):
    return cs.leaf("in", *sorted({n for f in fs for n in f.present()}))


# ---- (a) every code of every shape ----
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("flavour", ["int", "real"])
@pytest.mark.parametrize("shape", A_SHAPES)
def test_every_code_by_name(engine, shapes, shape, flavour, agg):
    """`in` all names grouped by name.  At 60 s pinned and split tiles mix, at 20 s (`short_runs`: 50 s) up to two
    boundaries fall in a tile; once more under a window that cuts the first and the last tile.  `two_dicts_1m`, whose
    tiles are 300 s wide, runs at 200 s and 10 min instead.  The counts add up to the file's rows."""
    fs = shapes.get([shape], flavour)
    steps = cs.STEPS[shape]
    big, small = (steps[1], steps[0]) if len(steps) == 3 else (steps[-1], steps[0])
    for step, window in ((big, None), (small, None), (small, cs.cut_window([shape]))):
        out = _five(engine, shapes, fs, step, _all(fs), agg, [NAME], window=window, label=f"a {shape} {flavour} {agg} {step} {window}")
        mg = out["on"][1]
        assert {t["name"] for t in mg.tags} == set(fs[0].present())
        if agg == "count":
            lo, hi = (cs.T0 + window[0], cs.T0 + ft.HOUR - window[1]) if window else (cs.T0, cs.T0 + ft.HOUR)
            inside = int(((fs[0].ts >= lo) & (fs[0].ts < hi)).sum())
            assert int(np.sum(mg.values)) == inside and (window is not None or inside == fs[0].rows)
            if window:
                assert inside < fs[0].rows   # the cut did drop rows of the end tiles


def test_sixty_five_names_get_no_copy(engine, shapes):
    """One name past build_cluster's rule (dict_n 65, bw 7): nothing is built or charged, scan_clu is never launched and
    the rows are the oracle's; the 64-name file beside it did get its copy."""
    for flavour in ("int", "real"):
        assert shapes.clu_growth[("uniform_65", flavour)] == 0
        assert shapes.clu_growth[("uniform_64", flavour)] >= 10 * cs.ROWS
        fs = shapes.get(["uniform_65"], flavour)
        for agg in AGGS:
            out = _five(engine, shapes, fs, 60_000, _all(fs), agg, [NAME], taken=False, label=f"65 names {flavour} {agg}")
            assert len({t["name"] for t in out["on"][1].tags}) == 65


# ---- (b) many codes, one cell ----
@pytest.mark.parametrize("agg", ["sum", "min", "max", "count"])
@pytest.mark.parametrize("flavour", ["int", "real"])
def test_many_codes_one_cell(engine, shapes, flavour, agg):
    """`regex ^metric_` with no groupBy at a 10 min step: every tile of the 10-minute files is pinned, and all of its
    codes -- up to 64 lanes at once -- merge into the one cell (`growing` ends in a second bucket)."""
    for shape in A_SHAPES:
        fs = shapes.get([shape], flavour)
        out = _five(engine, shapes, fs, TEN_MIN, cs.leaf("regex", "^metric_"), agg, label=f"b {shape} {flavour} {agg}")
        mg = out["on"][1]
        assert len(mg) == (2 if shape == "growing" else 1)
        if agg == "count":
            assert int(np.sum(mg.values)) == fs[0].rows


# ---- (c) sub-blocks at the edges ----
def _edge_filters(shape, fs):
    if shape == "two_dicts_1m":   # the 33-entry chunk's last code (introduced last) and the 5-entry chunk's first
        return [("all", _all(fs)), ("last", cs.leaf("eq", "metric_20")), ("first", cs.leaf("eq", "metric_00"))]
    k = int(shape[-2:])
    return [("all", _all(fs)), ("last", cs.leaf("eq", cs.NAMES[k - 1])), ("first", cs.leaf("eq", cs.NAMES[0]))]


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("flavour", ["int", "real"])
@pytest.mark.parametrize("shape", ["big_tile_07", "big_tile_64", "two_dicts_1m"])
def test_sub_blocks_at_the_edges(engine, shapes, shape, flavour, agg):
    """One split tile of five sub-blocks whose 10 min boundary falls inside the third (big_tile), and the tiles of
    10,000 rows of two chunk dictionaries inside a stride sized for the larger one (two_dicts_1m: at 10 min under a
    window that cuts both tiles, and at 200 s, where a boundary falls inside a sub-block of each).  The split tiles read
    fewer bytes with the area than with LK_NO_CLU_SUB=1."""
    fs = shapes.get([shape], flavour)
    calls = [(TEN_MIN, None)] if shape != "two_dicts_1m" else [(TEN_MIN, cs.cut_window([shape])), (200_000, None)]
    for step, window in calls:
        for name, filt in _edge_filters(shape, fs):
            out = _five(engine, shapes, fs, step, filt, agg, [NAME], window=window, label=f"c {shape} {flavour} {agg} {name} {step}")
            assert len(out["on"][1]) > 0
            a, b = out["on"][1].stats["plan_bytes"], out["nosub"][1].stats["plan_bytes"]
            assert 0 < a < b, (shape, flavour, agg, name, step, a, b)


# ---- (d) NaN in the last code ----
def _classes(rows, agg):
    zero = ("-0", "+0")
    return sorted((t, tags.get("name"), "0" if agg == "sum" and nf.value_class(v) in zero else nf.value_class(v))
                  for t, v, tags in rows)


@pytest.mark.parametrize("agg", ["min", "max", "sum"])
@pytest.mark.parametrize("which", ["uniform", "big_tile"])
def test_nan_in_the_last_code(engine, shapes, which, agg):
    """NaNs in the rows of the last code (lane dict_n - 1, bit dict_n - 1 of a pinned tile's mask, the last half-word of
    the sub-block area's NaN bits -- alone in its word where dict_n is odd), two files in two globs.  uniform: 60 s and
    20 s steps, the first five minutes' cells of the last code hold NaN alone.  big_tile: the NaNs lie in whole
    sub-blocks of a split tile.  A merged MIN that met a NaN is evaluated again with its cells kept per glob
    (`redo` == 2), whichever kernel met it."""
    fs = shapes.get([f"{which}_07", f"{which}_64"], "nan")
    for step in ((60_000, 20_000) if which == "uniform" else (TEN_MIN,)):
        out = _five(engine, shapes, fs, step, nf.all_names(), agg, [NAME], glob_size=1, label=f"d {which} {agg} {step}")
        want_pg, want_mg = out["want"]
        assert len(want_pg) == 2
        for mode, _ in MODES:
            pg, mg = out[mode]
            assert _classes(mg.rows(), agg) == _classes(want_mg, agg), mode
            for gi, g in enumerate(pg.per_glob(len(want_pg))):
                assert _classes(g, agg) == _classes(want_pg[gi], agg), (mode, gi)
            assert mg.stats.get("redo", 0) == (2 if agg == "min" else 0), (mode, mg.stats)
        rows = {(tags["name"], t): v for t, v, tags in out["on"][1].rows()}
        if which == "uniform":   # cells of NaN alone: MIN has nothing else to return there
            only_nan = [v for (n, t), v in rows.items() if n == "metric_06" and t < cs.T0 + 4 * cs.MIN]
            assert len(only_nan) == 4 * cs.MIN // step and all(v != v for v in only_nan)
        else:   # NaN beside other values in both of the tile's buckets: MAX and SUM return it, MIN skips it
            v = [v for (n, t), v in rows.items() if n == "metric_63"]
            assert len(v) == 2 and all((x != x) == (agg != "min") for x in v)


# ---- (e) name-only filter trees ----
def _tree_call(engine, shapes, i, tree, label, taken=True):
    si, flavour, agg, gbs, glob_size, step, cut = cs.tree_case(i)
    fs = shapes.get(cs.TREE_SETS[si], flavour)
    try:
        out = _five(engine, shapes, fs, step, tree, agg, gbs, glob_size=glob_size,
                    window=cs.cut_window(cs.TREE_SETS[si]) if cut else None, taken=taken, label=label)
        for mode, _ in MODES:
            for r in out[mode]:
                assert r.stats["filter"]["table"] == 1, (mode, r.stats)
    except AssertionError as e:
        raise AssertionError(f"{ft.describe('clu_shapes', i, tree, cs.TREE_SEED)}: {e}") from e
    return out


@pytest.mark.parametrize("i", range(cs.N_TREES))
def test_random_name_trees(engine, shapes, i):
    """filter_trees.random_tree over the name alone (1 + i % 6 leaves: not, or, !=, not_in, regex, contains, exists);
    file sets, flavours, aggregates, groupBys, glob sizes, steps and cut windows rotate (clu_shapes.tree_case)."""
    _tree_call(engine, shapes, i, cs.tree(i), f"e tree {i}")


@pytest.mark.parametrize("j", range(len(cs.HAND_TREES)))
def test_hand_written_trees(engine, shapes, j):
    label, tree = cs.HAND_TREES[j]
    for i in (4 * j + 3, 4 * j + 6):   # two rotations each: a cut 20 s call over all four files, a 60 s call over three
        _tree_call(engine, shapes, i, tree, f"e hand {label} {i}")


@pytest.mark.parametrize("j", range(len(cs.ABSENT_TREES)))
def test_trees_over_an_absent_field_are_declined(engine, shapes, j):
    """See the module docstring: a second string column keeps the call from scan_clu; the rows are the oracle's."""
    label, tree = cs.ABSENT_TREES[j]
    out = _tree_call(engine, shapes, 5 + j, tree, f"e absent {label}", taken=False)
    assert len(out["on"][1]) > 0
