"""Seeded random filter trees (tests/filter_trees.py) through every scan path of the MI355X evaluator, against the
oracle (oracle/dataexpr.py::_eval_filter evaluates any tree exactly).  Bar: tests/parity.py::assert_rows_equal as it
stands -- count / min / max bit-exact, sums within 1 ulp of the exact sum -- per glob and merged.

Per tree the aggregate (sum / min / max / count / avg), the groupBys ([] / [service] / [name, namespace]), glob_size
(1 / 2 / 3) rotate; every fourth tree runs at a 1 s step over a window that cuts tiles, the others at 10 minutes; every
seventh runs over the NULL-free small-dictionary files alone (a, b, f), so scan_lean can take a whole call.  Two
fixtures: `clean` (no NULL value: lean tables) and `nulls` (5 % NULL, 2 % NaN values).

Strata, 40 trees each on both fixtures (wide 24, numeric 32: the oracle's side of their trees is slow; tag / exemplar / numeric groupBy: 20-24 trees reused from them); the paths a
stratum must reach are asserted from the call's stats (`filter`, `lean_split`, `general_segments`).  A stratum's trees
are checked against the oracle's output alone before the GPU runs: at most a quarter degenerate (no row or every row
passes), one tree under 5 % and one over 60 % of the rows."""
import json

import pytest

from tests import filter_trees as ft
from tests.parity import assert_rows_equal

pytestmark = pytest.mark.gpu

N = 40
COUNTS = {"wide": 24, "numeric": 32}   # fewer trees where the oracle's side of a tree is slow (many cells, row loops)
AGGS = ["sum", "min", "max", "count", "avg"]
GBS = [[], [ft.SVC], [ft.NAME, ft.NS]]
LEAN_FILES = [0, 1, 5]   # profiles a, b, f
CUT = (ft.T0 + 7 * 60_000 + 13, ft.T0 + 12 * 60_000 + 7)   # the 1 s-step window: inside tiles, off the step grid

# Trees the fuzz found failing, kept as literals: (label, fixture, tree, agg, groupBys, glob_size, step)
FOUND = []


class Data:
    def __init__(self, engine, dirpath, value_nulls):
        self.name = "nulls" if value_nulls else "clean"
        self.paths, self.blobs, self.ts = ft.make_files(dirpath, value_nulls)
        self.keys = [f"ftree/{self.name}/{p}" for p in ft.PROFILES]
        for k, b in zip(self.keys, self.blobs):
            engine.put_segment(k, b)
        self.cache = {}


@pytest.fixture(scope="module")
def clean(engine, tmp_path_factory):
    return Data(engine, tmp_path_factory.mktemp("ftree_clean"), False)


@pytest.fixture(scope="module")
def nulls(engine, tmp_path_factory):
    return Data(engine, tmp_path_factory.mktemp("ftree_nulls"), True)


@pytest.fixture(params=["clean", "nulls"])
def data(request):
    return request.getfixturevalue(request.param)


class Case:
    """One tree's call: the rotation of aggregate, groupBys, glob_size, step / window and file set by index."""

    def __init__(self, d, stratum, i, tree, gbs=None, agg=None, glob_size=None, step=None):
        from lakeside_amd import synth
        self.label = f"{d.name}: {ft.describe(stratum, i, tree)}"
        self.tree = tree
        self.agg = agg or AGGS[i % 5]
        self.gbs = gbs if gbs is not None else (ft.wide_group_bys(i, tree) if stratum == "wide" else GBS[i % 3])
        self.glob_size = glob_size or 1 + i % 3
        self.step = step or (1000 if i % 4 == 3 else 600_000)
        self.files = LEAN_FILES if i % 7 == 0 else list(range(len(d.keys)))
        self.keys = [d.keys[j] for j in self.files]
        self.blobs = [d.blobs[j] for j in self.files]
        self.segs = [synth.segment_request(j, step=self.step, hour=0) for j in self.files]
        self.window = (ft.T0, ft.T0 + ft.HOUR)
        if self.step == 1000:
            self.window = CUT
            for s in self.segs:
                s["startTs"], s["endTs"] = CUT
        self.window_rows = sum(int(((d.ts[j] >= self.window[0]) & (d.ts[j] < self.window[1])).sum()) for j in self.files)

    def request(self, **kw):
        from lakeside_amd import synth
        return json.dumps(synth.pushdown(self.tree, self.segs, self.agg, self.gbs, **kw))


def expect(d, stratum, i, tree):
    """The case with the oracle's cells, per-glob rows, merged rows and passing-row count (cached per fixture)."""
    from oracle import dataexpr as dx
    key = (stratum, i)
    if key not in d.cache:
        c = Case(d, stratum, i, tree)
        c.req = c.request()
        c.pr = dx.parse_pushdown(c.req)
        cells = dx.evaluate_glob_cells(c.pr, c.glob_size, c.keys, sources=c.blobs)
        c.per_glob = [[(x.ts, x.agg_value(c.agg), x.tags) for x in g] for g in cells]
        c.merged = dx.merge_glob_cells(c.pr, cells)
        c.passing = sum(x.rows for g in cells for x in g)
        d.cache[key] = c
    return d.cache[key]


def honest(cases, stratum):
    """The fuzz is not vacuous, from the oracle's output alone."""
    frac = [c.passing / c.window_rows for c in cases]
    degenerate = sum(c.passing == 0 or c.passing == c.window_rows for c in cases)
    assert 4 * degenerate <= len(cases), f"{stratum}: {degenerate} of {len(cases)} trees pass no row or every row"
    assert min(f for f in frac if f > 0) < 0.05 and max(f for f in frac if f < 1) > 0.60, f"{stratum}: pass fractions {sorted(frac)}"


def run(engine, c, merged_only=False):
    """GPU == oracle per glob and merged; returns (merged rows, merged stats)."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    if not merged_only:
        got = engine.eval_pushdown(c.req, c.keys, c.glob_size, LK_PER_GLOB_ROWS).per_glob(len(c.per_glob))
        for gi, (g, w) in enumerate(zip(got, c.per_glob)):
            assert_rows_equal(g, w, c.agg, f"{c.label} glob {gi}")
    res = engine.eval_pushdown(c.req, c.keys, c.glob_size, LK_MERGED)
    rows = res.rows()
    assert_rows_equal(rows, c.merged, c.agg, f"{c.label} merged")
    return rows, res.stats


def run_stratum(engine, d, stratum):
    cases = [expect(d, stratum, i, t) for i, t in ft.trees(stratum, COUNTS.get(stratum, N))]
    honest(cases, stratum)
    return cases, [run(engine, c)[1] for c in cases]


def test_one_column(engine, data):
    cases, stats = run_stratum(engine, data, "one_column")
    assert all(s["filter"]["table"] == 1 for s in stats)
    if data.name == "clean":
        assert any(s["lean_split"] == 2 for s in stats), [s["lean_split"] for s in stats]
    else:
        assert all(s["lean_split"] <= 1 for s in stats), [s["lean_split"] for s in stats]


def test_early_late(engine, data):
    cases, stats = run_stratum(engine, data, "early_late")
    f = [s["filter"] for s in stats]
    assert 2 * sum(x["late_mask"] != 0 for x in f) >= len(f), f
    assert {x["early"] == 0 for x in f if x["late_mask"]} == {True, False}, f   # a non-zero early column: the swap runs


def test_mixed(engine, data):
    cases, stats = run_stratum(engine, data, "mixed")
    assert all(s["filter"]["late_mask"] == 0 and s["filter"]["table"] == 1 for s in stats), [s["filter"] for s in stats]


def test_wide(engine, data):
    cases, stats = run_stratum(engine, data, "wide")
    ncols = [len({ft.NAME} | set(ft._leaf_count(c.tree)) | set(c.gbs)) for c in cases]
    assert min(ncols) >= 4 and max(ncols) == 8, ncols          # more than 3 columns: no swap
    assert all(s["filter"]["table"] == 1 for s in stats), [s["filter"] for s in stats]


def test_program(engine, data):
    cases, stats = run_stratum(engine, data, "program")
    assert all(s["filter"]["table"] == 0 and s["filter"]["leaves"] >= 7 for s in stats), [s["filter"] for s in stats]
    assert max(s["filter"]["leaves"] for s in stats) == 32


def test_value_leaves(engine, data):
    cases, stats = run_stratum(engine, data, "value_leaves")
    assert all(s["filter"]["vleaf"] == 1 for s in stats), [s["filter"] for s in stats]
    if data.name == "clean":
        assert any(s["general_segments"] == 0 and s["segments"] > 0 for s in stats), [s["general_segments"] for s in stats]
    else:
        assert all(s["general_segments"] > 0 for s in stats if s["segments"]), [s["general_segments"] for s in stats]


def test_numeric(engine, data):
    cases, stats = run_stratum(engine, data, "numeric")
    assert all(s["general_segments"] == s["segments"] for s in stats)
    assert any(s["segments"] > 0 for s in stats)


def _reused(names, per):
    return [(s, i, t) for s in names for i, t in ft.trees(s, per)]


def test_tag_query(engine, data):
    """Trees of the first five strata as tag queries over the service and the name."""
    from lakeside_amd import LK_MERGED
    from oracle import dataexpr as dx
    key = lambda t: sorted(t.items())   # noqa: E731
    nonempty = 0
    for s, i, tree in _reused(["one_column", "early_late", "mixed", "wide", "program"], 4):
        c = Case(data, s, i, tree)
        for tag in (ft.SVC, ft.NAME):
            req = c.request(tag=tag)
            want = dx.evaluate_tag_merged(dx.parse_pushdown(req), tag, c.keys, c.glob_size, sources=c.blobs)
            got = engine.eval_pushdown(req, c.keys, c.glob_size, LK_MERGED)
            assert sorted(got.tags, key=key) == sorted(want, key=key), f"tag {tag} {c.label}"
            nonempty += bool(want)
    assert nonempty >= 10


def test_exemplar(engine, data):
    """<= 6-leaf and 7..12-leaf trees as exemplar queries, limit 50, both orders (the interpreter of the row scan)."""
    from lakeside_amd import LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx
    from oracle import exemplar as ex
    picks = _reused(["mixed", "early_late"], 6) + [(s, i, t) for s, i, t in _reused(["program", "numeric"], 24)
                                                   if 7 <= len(ft.leaves_of(t)) <= 12][:12]
    assert sum(len(ft.leaves_of(t)) > 6 for _, _, t in picks) >= 8
    nonempty = 0
    for n, (s, i, tree) in enumerate(picks):
        c = Case(data, s, i, tree)
        order = "DESC" if n % 2 else "ASC"
        req = json.dumps({"baseExpr": {"id": "A", "dataset": "logs", "limit": 50, "order": order, "filter": tree},
                          "segmentRequests": c.segs})
        want = ex.evaluate_exemplar(dx.parse_pushdown(req), c.keys, c.glob_size, sources=c.blobs)
        res = engine.eval_pushdown(req, c.keys, c.glob_size, LK_PER_GLOB_ROWS)
        rows = list(zip(res.ts.tolist(), res.values.tolist(), res.tags, res.globs.tolist()))
        assert len(rows) == len(want), f"exemplar {order} {c.label}: {len(rows)} rows vs {len(want)}"
        for g, w in zip(rows, want):
            assert (g[0], g[3], g[2]) == (w[0], w[3], w[2]), f"exemplar {order} {c.label}"
        nonempty += bool(want)
    assert nonempty >= len(picks) // 2


def test_numeric_group_by(engine, data, tmp_path):
    """Trees of the mixed and numeric strata grouped by attr.code (INT32), expectation over VARCHAR twins."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx
    from tests import numgroup_ref as nr
    twins = nr.write_twins(data.paths, [ft.CODE], len(data.paths), str(tmp_path / "twins"))
    for s, i, tree in _reused(["mixed", "numeric"], 10):
        c = Case(data, s, i, tree, gbs=[ft.CODE] + GBS[i % 3][:1])
        req = c.request()
        pr = dx.parse_pushdown(req)
        cells = dx.evaluate_glob_cells(pr, c.glob_size, [twins[j] for j in c.files])
        got = engine.eval_pushdown(req, c.keys, c.glob_size, LK_PER_GLOB_ROWS)
        for gi, (g, w) in enumerate(zip(got.per_glob(len(cells)), cells)):
            assert_rows_equal(g, [(x.ts, x.agg_value(c.agg), x.tags) for x in w], c.agg, f"numgb {c.label} glob {gi}")
        res = engine.eval_pushdown(req, c.keys, c.glob_size, LK_MERGED)
        assert_rows_equal(res.rows(), dx.merge_glob_cells(pr, cells), c.agg, f"numgb {c.label} merged")
        assert [x["column"] for x in res.stats["numeric_dims"]] == [ft.CODE], res.stats


def _same_answer(engine, d, stratum, toggles, monkeypatch, n=16):
    """Merged rows with each toggle set == the default's: the same timestamps and tags, count / min / max bit-identical,
    sum / avg each inside the oracle's bar.  Returns the stats per toggle."""
    out = {t: [] for t in toggles}
    for i, tree in ft.trees(stratum, n):
        c = expect(d, stratum, i, tree)
        base, _ = run(engine, c, merged_only=True)
        for t in toggles:
            with monkeypatch.context() as m:
                m.setenv(t, "1")
                rows, stats = run(engine, c, merged_only=True)
            out[t].append(stats)
            assert [(r[0], r[2]) for r in sorted(rows, key=_rk)] == [(r[0], r[2]) for r in sorted(base, key=_rk)], f"{t} {c.label}"
            if c.agg in ("count", "min", "max"):
                assert_rows_equal(rows, base, c.agg, f"{t} vs default {c.label}")
    return out


def _rk(r):
    return (r[0], sorted(r[2].items()))


def test_same_answer_late(engine, data, monkeypatch):
    st = _same_answer(engine, data, "early_late", ["LK_NO_LATE", "LK_LATE_CHUNK", "LK_NO_EARLY_FIRST"], monkeypatch)
    assert all(s["lean_split"] == 0 for s in st["LK_NO_LATE"]), "LK_NO_LATE left scan_lean on"
    if data.name == "clean":
        assert any(s["late_chunk"] == 1 for s in st["LK_LATE_CHUNK"]), [s["late_chunk"] for s in st["LK_LATE_CHUNK"]]


def test_same_answer_lean_split(engine, data, monkeypatch):
    st = _same_answer(engine, data, "one_column", ["LK_NO_LEAN_SPLIT"], monkeypatch)
    assert all(s["lean_split"] == 0 for s in st["LK_NO_LEAN_SPLIT"])


def test_same_answer_vleaf(engine, data, monkeypatch):
    st = _same_answer(engine, data, "value_leaves", ["LK_NO_VLEAF"], monkeypatch)
    assert all(s["filter"]["vleaf"] == 0 and s["general_segments"] == s["segments"] for s in st["LK_NO_VLEAF"])


def test_found_trees(engine, clean, nulls):
    from oracle import dataexpr as dx
    for label, fixture, tree, agg, gbs, glob_size, step in FOUND:
        d = clean if fixture == "clean" else nulls
        c = Case(d, label, 1, tree, gbs=gbs, agg=agg, glob_size=glob_size, step=step)
        c.req = c.request()
        c.pr = dx.parse_pushdown(c.req)
        cells = dx.evaluate_glob_cells(c.pr, c.glob_size, c.keys, sources=c.blobs)
        c.per_glob = [[(x.ts, x.agg_value(c.agg), x.tags) for x in g] for g in cells]
        c.merged = dx.merge_glob_cells(c.pr, cells)
        run(engine, c)
