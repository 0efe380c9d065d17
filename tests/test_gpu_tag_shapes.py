"""The dictionary-index decoders of every string column that is NOT the name -- filter keys and group dims -- at every
index width 1..17 and on both sides of the LDS lookup cap, on the MI355X (files and requests: tests/tag_shapes.py,
pinned on the CPU by tests/test_tag_shapes_cpu.py).

Every chart case is evaluated per glob and merged, each against the oracle with assert_rows_equal (tests/parity.py: the
suite's bar, no tolerance of its own), through five routes, each proven by the call's stats:
  lean         as it stands: scan_lean takes the NULL-free tiles and decodes the tag per listed row (late_issue / rowsN),
               scan_tiles the tiles with NULL tags.  lean_split >= 1, filter.late_mask != 0, late_chunk == 0,
               general_segments == 0
  chunk        LK_LATE_CHUNK=1, requests with a leaf on the tag column whose group space is <= 65,536 (setup_scan's
               rule): scan_lean<.., EARLY> decodes 16 rows of the tag per chunk (late_code; bw > 7 or a dictionary
               past the cap: its per-row stage).  late_chunk == 1, lean_split >= 1
  tiles        LK_NO_LEAN=1 LK_NO_LEAN_SPLIT=1: scan_tiles alone, the tag late-materialized per listed row (lp.meta).
               lean_split == 0, general_segments == 0
  tiles_early  the same with LK_NO_LATE=1: every column through g8_issue / g8_window / g8_unpack in phase 1.
               lean_split == 0
  rows         the filter gains `and attr.dur >= 0`, a numeric leaf every row passes: the general row scan (ex_scan AGG,
               hybrid_get_buf).  general_segments == segments
Timestamps and tags are the same rows in the five routes; COUNT, MIN, MAX and the sums / averages of the `int` flavour
are lean's BIT FOR BIT in the other four; sums of real values hold the oracle bar in each route.

Strata: (a) every code a group; (b) leaves on the tag column at the codes on either side of the top index bit; (c)
exists / not exists over NULL tags (the NULL group and the merged MIN / MAX fold are (a) on the `nulls` files); (d) a
file without the column beside one with it; (e) tag queries; (f) exemplar rows (ex_gather's packed_get prints the tag).
(b) and (c) run on the `int` flavour (a filter reads no value); the `real` flavour runs (a) and (b)'s grouped case."""
import json

import pytest

from tests import tag_shapes as tg
from tests.parity import assert_rows_equal
from tests.test_gpu_clustered import _bits, _Env

pytestmark = pytest.mark.gpu

NAME = tg.NAME
_TILES = {"LK_NO_LEAN": 1, "LK_NO_LEAN_SPLIT": 1}
ROUTES = (("lean", {}), ("chunk", {"LK_LATE_CHUNK": 1}), ("tiles", _TILES), ("tiles_early", dict(_TILES, LK_NO_LATE=1)),
          ("rows", {}))
AGGS = ["sum", "min", "max", "count", "avg"]
TEN_MIN, FOUR_MIN = 10 * tg.MIN, 4 * tg.MIN
SMALL = [s for s in tg.SHAPES if s not in (tg.BIG, "absent")]
VARIANTS = {s: (("plain", "nulls") if s in tg.WIDE else ("plain",)) for s in tg.SHAPES}
KEY = lambda t: sorted(t.items())   # noqa: E731


class Shapes:
    def __init__(self, engine, dirpath):
        self.files = tg.make_files(dirpath)
        for f in self.files.values():
            engine.load_segment(f.path)
        self.cells = {}


@pytest.fixture(scope="module")
def shapes(engine, tmp_path_factory):
    return Shapes(engine, tmp_path_factory.mktemp("tag_shapes_gpu"))


def routes_of(tag_leaf, gbs):
    """The routes a chart request runs through (`chunk`: see the module docstring)."""
    return [r for r, _ in ROUTES if r != "chunk" or (tag_leaf and tg.TAGW not in gbs)]


def _check_stats(route, st, label):
    if route == "lean":
        assert st["lean_split"] >= 1 and st["filter"]["late_mask"] != 0 and st["late_chunk"] == 0, (label, st)
        assert st["general_segments"] == 0, (label, st)
    elif route == "chunk":
        assert st["late_chunk"] == 1 and st["lean_split"] >= 1, (label, st)
    elif route == "tiles":
        assert st["lean_split"] == 0 and st["general_segments"] == 0, (label, st)
    elif route == "tiles_early":
        assert st["lean_split"] == 0, (label, st)
    else:
        assert st["general_segments"] == st["segments"] > 0, (label, st)


def _five(engine, sh, fs, step, filt, aggs, gbs, tag_leaf, glob_size=10, label="", empty=False):
    """{agg: {route: (per-glob result, merged result)}} of one request over the files `fs`, after the oracle, the stats
    and the cross-route comparisons of the module docstring.  The oracle's cells are evaluated once per (files, filter,
    groupBys, step, glob size) and every aggregate is derived from them; the `rows` route's extra leaf passes every
    row, so its expectation is the same.  `empty`: the oracle passes no row (the call may then be left without a cell
    space and launch nothing, so the stats prove no route); every other request must pass some."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS, synth
    from oracle import dataexpr as dx
    keys, blobs = [f.path for f in fs], [f.blob for f in fs]
    segs = tg.segs(len(fs), step)
    ck = (tuple(keys), json.dumps(filt, sort_keys=True), tuple(gbs), step, glob_size)
    if ck not in sh.cells:
        pr = dx.parse_pushdown(json.dumps(synth.pushdown(filt, segs, "sum", list(gbs))))
        sh.cells[ck] = dx.evaluate_glob_cells(pr, glob_size, keys, sources=blobs)
    cells = sh.cells[ck]
    assert any(len(g) for g in cells) != empty, label
    integral = all(f.flavour == "int" for f in fs)
    out = {}
    for agg in aggs:
        pr = dx.parse_pushdown(json.dumps(synth.pushdown(filt, segs, agg, list(gbs))))
        want_pg = [[(c.ts, c.agg_value(agg), c.tags) for c in g] for g in cells]
        want_mg = dx.merge_glob_cells(pr, cells)
        res = out[agg] = {}
        for route, env in ROUTES:
            if route not in routes_of(tag_leaf, gbs):
                continue
            req = json.dumps(synth.pushdown(tg.with_dur(filt) if route == "rows" else filt, segs, agg, list(gbs)))
            with _Env(**env):
                pg = engine.eval_pushdown(req, keys, glob_size, LK_PER_GLOB_ROWS)
                mg = engine.eval_pushdown(req, keys, glob_size, LK_MERGED)
            for gi, (g, w) in enumerate(zip(pg.per_glob(len(want_pg)), want_pg)):
                assert_rows_equal(g, w, agg, f"{label} {agg} {route} glob {gi}")
            assert_rows_equal(mg.rows(), want_mg, agg, f"{label} {agg} {route} merged")
            for r in (pg, mg):
                if empty:
                    assert len(r) == 0, (label, agg, route)
                else:
                    _check_stats(route, r.stats, f"{label} {agg} {route}")
            res[route] = (pg, mg)
        for route in res:
            for a, b in zip(res["lean"], res[route]):
                assert a.ts.tolist() == b.ts.tolist() and a.tags == b.tags, (label, agg, route)
                if agg in ("count", "min", "max") or integral:
                    assert _bits(a.values) == _bits(b.values), f"{label} {agg}: {route} rows differ from lean's"
    return out


def _by_tag_checks(out, fs, col):
    """Every value of the files is a group (and NULL one more), and the counts add up to the files' rows."""
    mg = out["count"]["lean"][1]
    groups = {t.get(col) for t in mg.tags}
    want = {v for f in fs for v in f.present()}
    assert {g for g in groups if g in want} == want and len(groups) == len(want) + any((f.codes < 0).any() for f in fs)
    assert int(sum(mg.values)) == sum(f.rows for f in fs)


# ---- (a) every code a group ----
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("flavour", ["int", "real"])
@pytest.mark.parametrize("shape", SMALL)
def test_every_code_is_a_group(engine, shapes, shape, flavour, agg):
    """`name in (all four)` :by tag at a 4 min step (three buckets; from 1,025 values on one bucket of 10 min, so the
    rows stay few): one wrong code anywhere changes a row.  On the `nulls` files the NULL group is a row, and the
    merged MIN / MAX take the rekey fold."""
    step = FOUR_MIN if tg.NVALUES[shape] < 1025 else TEN_MIN
    for variant in VARIANTS[shape]:
        fs = [shapes.files[(shape, flavour, variant)]]
        out = _five(engine, shapes, fs, step, tg.all_names(), [agg], [fs[0].col], False, label=f"a {shape} {flavour} {variant}")
        if agg == "count":
            _by_tag_checks(out, fs, fs[0].col)


@pytest.mark.parametrize("agg", ["sum", "count"])
@pytest.mark.parametrize("variant", ["plain", "nulls"])
@pytest.mark.parametrize("flavour", ["int", "real"])
def test_every_code_is_a_group_65537(engine, shapes, flavour, variant, agg):
    """65,537 groups in one bucket, pages of 13..17 bits (the NULLs of `nulls` lie in the 17-bit pages)."""
    fs = [shapes.files[(tg.BIG, flavour, variant)]]
    out = _five(engine, shapes, fs, TEN_MIN, tg.all_names(), [agg], [tg.TAGW], False, label=f"a {tg.BIG} {flavour} {variant}")
    if agg == "count":
        _by_tag_checks(out, fs, tg.TAGW)


# ---- (b) leaves on the tag column ----
@pytest.mark.parametrize("shape", SMALL)
def test_leaves_on_the_tag(engine, shapes, shape):
    """`in` of the values of code 0, 2^(bw-1) - 1, 2^(bw-1) and the last code and of a value no file holds, `!=` the
    last code's value, a regex that passes the even values, `not (in ..)`: grouped by name at 10 min; `in` once more by
    name and tag at 4 min, in both flavours.  A wrong mask or shift sends a row through the wrong leaf."""
    for variant in VARIANTS[shape]:
        f = shapes.files[(shape, "int", variant)]
        for i, (name, filt) in enumerate(tg.tag_filters(shape)):
            out = _five(engine, shapes, [f], TEN_MIN, filt, ["count", AGGS[i % 3]], [NAME], True, label=f"b {shape} {variant} {name}")
            got = int(sum(out["count"]["lean"][1].values))
            edges = set(tg.edge_values(shape))
            tags = [t for t in f.tags]
            want = {"in edges": sum(t in edges for t in tags), "not in edges": sum(t is not None and t not in edges for t in tags),
                    "ne last": sum(t is not None and t != tg.TAGS[tg.NVALUES[shape] - 1] for t in tags),
                    "regex half": sum(t is not None and t[-1] in "02468" for t in tags)}[name]
            assert got == want > 0, (shape, variant, name, got, want)
        for flavour in ("int", "real"):
            g = shapes.files[(shape, flavour, variant)]
            out = _five(engine, shapes, [g], FOUR_MIN, tg.tag_filters(shape)[0][1], ["sum", "max"], [NAME, g.col], True,
                        label=f"b {shape} {flavour} {variant} by name and tag")
            assert {t[g.col] for t in out["sum"]["lean"][1].tags} == set(tg.edge_values(shape)) & set(g.present())


def test_leaves_on_the_tag_65537(engine, shapes):
    for variant in ("plain", "nulls"):
        f = shapes.files[(tg.BIG, "int", variant)]
        out = _five(engine, shapes, [f], TEN_MIN, tg.tag_filters(tg.BIG)[0][1], ["count", "sum"], [NAME], True, label=f"b {tg.BIG} {variant}")
        edges = set(tg.edge_values(tg.BIG))
        assert int(sum(out["count"]["lean"][1].values)) == sum(t in edges for t in f.tags) >= 2


# ---- (c) NULL tags ----
@pytest.mark.parametrize("shape", [s for s in tg.WIDE if s != tg.BIG])
def test_exists_over_null_tags(engine, shapes, shape):
    """The value index is the definition levels' prefix, not the row: `exists` and `not exists`, by name."""
    f = shapes.files[(shape, "int", "nulls")]
    nulls = int((f.codes < 0).sum())
    for i, (name, filt) in enumerate(tg.null_filters(shape)):
        out = _five(engine, shapes, [f], FOUR_MIN, filt, ["count", AGGS[i]], [NAME], True, label=f"c {shape} {name}")
        assert int(sum(out["count"]["lean"][1].values)) == (nulls if name == "not exists" else f.rows - nulls) > 0


# ---- (d) a file without the column ----
@pytest.mark.parametrize("flavour", ["int", "real"])
@pytest.mark.parametrize("glob_size", [1, 2])
def test_absent_column_beside_wide_33(engine, shapes, flavour, glob_size):
    """`absent` and wide_33 in two globs and in one: the file without the column gives the NULL group (dim_null).  In a
    glob of its own its leaves on the column compile to `false` (and the oracle passes no row under `not exists`
    either: the other glob has no NULL); in one glob with wide_33 its rows are NULLs of the union and pass `not exists`
    alone."""
    fs = [shapes.files[("absent", flavour, "plain")], shapes.files[("wide_33", flavour, "plain")]]
    out = _five(engine, shapes, fs, FOUR_MIN, tg.all_names(), AGGS, [tg.TAG], False, glob_size, f"d {flavour} {glob_size} by tag")
    mg = out["count"]["lean"][1]
    assert int(sum(mg.values)) == fs[0].rows + fs[1].rows
    assert int(sum(v for v, t in zip(mg.values, mg.tags) if t.get(tg.TAG) not in fs[1].present())) == fs[0].rows
    for name, filt in [tg.tag_filters("wide_33")[0], tg.tag_filters("wide_33")[3]] + tg.null_filters("wide_33"):
        none = name == "not exists" and glob_size == 1
        out = _five(engine, shapes, fs, TEN_MIN, filt, ["count", "sum"], [NAME], True, glob_size, f"d {flavour} {glob_size} {name}", none)
        if name == "not exists" and not none:
            assert int(sum(out["count"]["lean"][1].values)) == fs[0].rows
    _five(engine, shapes, fs, FOUR_MIN, tg.with_names({"not": tg.leaf(tg.TAG, "in", tg.TAGS[0], tg.TAGS[32])}), ["min", "avg"],
          [NAME, tg.TAG], True, glob_size, f"d {flavour} {glob_size} by name and tag")


# ---- (e) tag queries ----
TAG_ROUTES = ("lean", "tiles", "tiles_early")


def _tag_query(engine, f, label):
    """The tag query over the file (`name in (all four) and <tag> exists`, as query-api sends it) through three routes:
    per glob and merged == the oracle's {tag, count} rows."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS, synth
    from oracle import dataexpr as dx
    req = json.dumps(synth.pushdown(tg.with_names(tg.leaf(f.col, "exists")), tg.segs(1, 60_000), tag=f.col))
    pr = dx.parse_pushdown(req)
    want_pg = dx.evaluate_tag_per_glob(pr, f.col, [f.path], 1, sources=[f.blob])
    want_mg = dx.evaluate_tag_merged(pr, f.col, [f.path], 1, sources=[f.blob])
    assert len(want_mg) == tg.NVALUES[f.shape]
    for route, env in ROUTES:
        if route not in TAG_ROUTES:
            continue
        with _Env(**env):
            pg = engine.eval_pushdown(req, [f.path], 1, LK_PER_GLOB_ROWS)
            mg = engine.eval_pushdown(req, [f.path], 1, LK_MERGED)
        got = pg.per_glob(len(want_pg))
        for gi, (g, w) in enumerate(zip(got, want_pg)):
            assert sorted((r[2] for r in g), key=KEY) == sorted(w, key=KEY), f"{label} {route} glob {gi}"
        assert sorted(mg.tags, key=KEY) == sorted(want_mg, key=KEY), f"{label} {route} merged"
        for st in (pg.stats, mg.stats):
            assert st["general_segments"] == 0 and (st["lean_split"] >= 1) == (route == "lean"), (label, route, st)


@pytest.mark.parametrize("shape", SMALL + [tg.BIG])
def test_tag_query(engine, shapes, shape):
    for variant in VARIANTS[shape]:
        _tag_query(engine, shapes.files[(shape, "int", variant)], f"e {shape} {variant}")


# ---- (f) exemplar rows ----
@pytest.mark.parametrize("shape", SMALL + [tg.BIG])
def test_exemplar_prints_the_tag(engine, shapes, shape):
    """No chart, limit 200, both sort directions, under (b)'s `in` leaf: ex_scan filters on the tag and ex_gather
    (packed_get) prints its text, equal to the oracle's row for row."""
    from tests.test_gpu_exemplar import _check, _request
    for variant in VARIANTS[shape]:
        f = shapes.files[(shape, "real", variant)]
        for order, reverse in (("desc", False), ("asc", True)):
            req = _request(tg.tag_filters(shape)[0][1], 1, limit=200, order=order, reverse=reverse, hour=0)
            got = _check(engine, req, [f.path], [f.blob], 1, f"f {shape} {variant} {order}")
            assert 0 < len(got) <= 200
            assert {t[f.col] for t in got.tags} <= set(tg.edge_values(shape))
        # and the file's first 200 rows, unfiltered: the codes 0, 1, 2 .. in order, each printed as its own value
        req = _request(tg.all_names(), 1, limit=200, order="asc", hour=0)
        got = _check(engine, req, [f.path], [f.blob], 1, f"f {shape} {variant} head")
        assert len(got) == 200


# ---- what the routes reach ----
def test_routes_reach_every_width():
    """From the parametrisation above alone: the (file, query) cases per route and the widths of their tag tiles."""
    tally = {r: [0, set()] for r, _ in ROUTES}

    def add(shape, nvariants, tag_leaf, gbs, n=1):
        for r in routes_of(tag_leaf, gbs):
            tally[r][0] += n * nvariants
            tally[r][1] |= tg.widths(shape)
    for s in SMALL + [tg.BIG]:
        nv, col = len(VARIANTS[s]), tg.tag_column(s)
        add(s, nv, False, [col], 2)                                            # (a), two flavours
        add(s, nv, True, [NAME], 4 if s != tg.BIG else 1)                      # (b) by name
        if s != tg.BIG:
            add(s, nv, True, [NAME, col], 2)                                   # (b) by name and tag, two flavours
            if s in tg.WIDE:
                add(s, 1, True, [NAME], 2)                                     # (c)
    add("wide_33", 1, False, [tg.TAG], 4)                                      # (d): 2 flavours x 2 glob sizes
    add("wide_33", 1, True, [NAME], 14)                                        # (4 filters; `not exists` in two globs is empty)
    add("wide_33", 1, True, [NAME, tg.TAG], 4)
    print({r: (n, min(w), max(w)) for r, (n, w) in tally.items()})
    for r in ("lean", "tiles", "tiles_early", "rows"):
        assert tally[r][1] == set(range(1, 18)), (r, tally[r])
    assert tally["chunk"][1] == set(range(1, 18)) and tally["chunk"][0] > 100
