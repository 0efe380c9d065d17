"""Pins the fixtures of tests/tag_shapes.py without a GPU, so that a pyarrow that cuts other pages is noticed here and
not as a silently weaker tests/test_gpu_tag_shapes.py.

The files' tiles are read with `build/load_check --tiles=<tag column>` (tools/load_check.cpp: the loader's own TileDesc
/ TileCol of that column, what the scan kernels' decoders see).  The census is the fact the GPU test rests on: every
index width 1..17 occurs in a tag-column tile, and pages of the 96-bit window's widths (bw <= 8) occur under chunk
dictionaries on both sides of LUT_CAP.  The sensitivity test proves, with the oracle alone, that the `int` data cannot
hide one mis-decoded row."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import tag_shapes as tg
from tests.parity import assert_rows_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE_DICT = 2


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tg.make_files(tmp_path_factory.mktemp("tag_shapes"))


def _tiles_of(paths, col):
    """{basename: [tile: {field: int}]} of column `col` from one run of the harness over `paths`."""
    out = subprocess.run([os.path.join(ROOT, "build", "load_check"), f"--tiles={col}", "1"] + paths, check=True,
                         capture_output=True, text=True, timeout=300).stdout
    bases = {os.path.basename(p) for p in paths}
    res, cur = {}, None
    for line in out.splitlines():
        head = line.split(" ", 1)[0]
        if head in bases:
            assert " error" not in line, line
            cur = res.setdefault(head, [])
        elif line.startswith("  tile "):
            f = line.split()
            assert int(f[1]) == len(cur)
            cur.append({kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]})
        assert not line.startswith("  unloaded"), line
    assert out.splitlines()[-1] == "failures=0"
    return res


@pytest.fixture(scope="module")
def tiles(files):
    """{(shape, flavour, variant): [tile]} of the tag column of every file that has one."""
    subprocess.run(["make", "-C", ROOT, "build/load_check"], check=True, capture_output=True)
    res = {}
    for col in (tg.TAG, tg.TAGW):
        keys = [k for k, f in files.items() if f.col == col and k[0] != "absent"]
        got = _tiles_of([files[k].path for k in keys], col)
        for k in keys:
            res[k] = got[os.path.basename(files[k].path)]
            assert sum(t["nrows"] for t in res[k]) == files[k].rows, k
    return res


def test_without_a_column_the_flag_prints_the_name(files):
    """`--tiles` alone is `--tiles=_cardinalhq.name`; a file without the asked column prints no tile line."""
    subprocess.run(["make", "-C", ROOT, "build/load_check"], check=True, capture_output=True)
    exe = os.path.join(ROOT, "build", "load_check")
    paths = [files[("wide_33", "int", "plain")].path, files[("absent", "int", "plain")].path]
    run = lambda flag: subprocess.run([exe, flag, "1"] + paths, check=True, capture_output=True, text=True).stdout   # noqa: E731
    assert run("--tiles") == run(f"--tiles={tg.NAME}")
    tag = run(f"--tiles={tg.TAG}")
    assert sum(l.startswith("  tile ") for l in tag.splitlines()) == sum(l.startswith("  tile ") for l in run("--tiles").splitlines()) // 2
    assert [l for l in tag.splitlines() if not l.startswith("  tile ")] == [l for l in run("--tiles").splitlines() if not l.startswith("  tile ")]


def test_every_tile_is_what_expect_states(tiles):
    for (shape, flavour, variant), ts in tiles.items():
        for t in ts:
            assert t["kind"] == PAGE_DICT and 1 <= t["nruns"] <= tg.RUN_CAP and t["sorted"] == 1, (shape, t)
        got = {(t["dict_n"], t["bw"]) for t in ts}
        if shape == tg.BIG:
            assert got == {(tg.BIG_K, bw) for bw in tg.BIG_BW}, (shape, got)
        elif shape in tg.WIDE:
            k = tg.NVALUES[shape]
            assert got == {(k, tg.EXPECT[k])}, (shape, got)
            assert ts[-1]["nrows"] % 64 != 0 and len(ts) > 1
        if variant == "nulls" and shape != tg.BIG:   # (a page's flag: the file's last few rows may make a page without one)
            assert sum(t["has_nulls"] == 0 for t in ts) <= 1 and sum(t["has_nulls"] for t in ts) >= 20, shape
        elif variant == "nulls":   # the NULLs begin after the 65,537 rows that introduce the values: the 17-bit pages
            assert {t["bw"] for t in ts if t["has_nulls"]} == {17}
        else:
            assert not any(t["has_nulls"] for t in ts), shape


def test_growing(tiles):
    for f in ("int", "real"):
        ts = tiles[("growing_300", f, "plain")]
        assert {t["dict_n"] for t in ts} == {300}
        assert {t["bw"] for t in ts} == tg.GROWING_BW
        assert any(t["vbase"] > t["run0_start"] and t["run0_lit"] == 1 for t in ts)


@pytest.mark.parametrize("shape,expect", [("runs_129", (129, 8)), ("runs_1025", (1025, 11))])
def test_runs(tiles, shape, expect):
    for f in ("int", "real"):
        ts = tiles[(shape, f, "plain")]
        assert {(t["dict_n"], t["bw"]) for t in ts} == {expect}
        full = [t for t in ts if t["nruns"] == tg.RUN_CAP]
        assert len(full) >= 3 and {t["run0_lit"] for t in full} == {0, 1}, [(t["nruns"], t["run0_lit"]) for t in ts]
        # tiles that start inside a bit-packed run (cut by a page of another column), at a value index off the groups of 8
        inside = [t for t in ts if t["vbase"] > t["run0_start"] and t["run0_lit"] == 1]
        assert inside and any((t["vbase"] - t["run0_start"]) % 8 for t in inside), ts
        # RLE runs of 8..40 rows push the bit-packed runs off the multiples of 8
        assert any(t["run0_lit"] == 1 and t["run0_start"] % 8 for t in ts)


def test_two_dicts(tiles, files):
    import io

    import pyarrow.parquet as pq
    for f in ("int", "real"):
        ts = tiles[("two_dicts", f, "plain")]
        assert {(t["rg"], t["dict_n"], t["bw"]) for t in ts} == {(0, 129, 8), (1, 300, 9), (2, 11, 4)}
    fl = files[("two_dicts", "int", "plain")]
    pf = pq.ParquetFile(io.BytesIO(fl.blob), read_dictionary=[tg.TAG])
    assert pf.read_row_group(1, columns=[tg.TAG]).column(0).chunk(0).dictionary.to_pylist() == tg.TAGS[299::-1]
    assert pf.read_row_group(0, columns=[tg.TAG]).column(0).chunk(0).dictionary.to_pylist() == tg.TAGS[:129]


@pytest.mark.parametrize("shape", ["wide_129", "wide_257", "wide_4097", tg.BIG])
def test_codes_follow_the_values(files, shape):
    """pyarrow numbers the chunk dictionary by first occurrence: code c is TAGS[c], with and without NULLs."""
    import io

    import pyarrow.parquet as pq
    for variant in ("plain", "nulls"):
        f = files[(shape, "int", variant)]
        col = pq.ParquetFile(io.BytesIO(f.blob), read_dictionary=[f.col]).read_row_group(0, columns=[f.col]).column(0)
        assert col.chunk(0).dictionary.to_pylist() == tg.TAGS[:tg.NVALUES[shape]]
        assert (f.codes < 0).any() == (variant == "nulls")


def test_census(tiles):
    """Every width 1..17, and the 96-bit window's widths on both sides of the LDS lookup cap."""
    seen = {(t["dict_n"], t["bw"], t["has_nulls"]) for ts in tiles.values() for t in ts}
    assert {bw for _, bw, _ in seen} >= set(range(1, 18)), sorted({bw for _, bw, _ in seen})
    assert any(n <= tg.LUT_CAP and bw <= 8 for n, bw, _ in seen) and any(n > tg.LUT_CAP and bw <= 8 for n, bw, _ in seen)
    assert {(256, 8, 0), (257, 9, 0), (128, 7, 0), (129, 8, 0), (256, 8, 1), (257, 9, 1)} <= seen
    assert {bw for _, bw, nulls in seen if nulls} >= set(range(1, 14)) | {17}     # NULLs at every width of wide_K
    assert {bw for n, bw, _ in seen if n == 300} >= {2, 4, 6, 7, 8}               # narrow pages, global lookup


# ---- the data cannot hide one mis-decoded row ----
def _by_tag(f, step, window=None):
    """{agg: merged rows} of `name in (all four) :by tag` over the one file (`window`: startTs, endTs)."""
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    segs = tg.segs(1, step)
    if window:
        segs[0]["startTs"], segs[0]["endTs"] = window
    pr = dx.parse_pushdown(json.dumps(synth.pushdown(tg.all_names(), segs, "sum", [f.col])))
    cells = dx.evaluate_glob_cells(pr, 1, [f.path], sources=[f.blob])
    out = {}
    for agg in ("count", "sum", "min", "max"):
        pr.baseExpr.chart.aggregation = agg
        out[agg] = dx.merge_glob_cells(pr, cells)
    return out


def _differ(a, b, agg):
    try:
        assert_rows_equal(a, b, agg)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("shape", ["wide_129", "wide_257", "wide_4097"])
def test_one_wrong_code_changes_every_aggregate(files, tmp_path, shape):
    """One row's code becomes code ^ 1, code ^ (1 << (bw - 1)) and 0 (one change at a time; its value stays what the
    value column holds).  At a 1 s step (over the 20 s around the row), for a row alone in its (tag, second) cell, the
    :by tag rows of COUNT, SUM, MIN and MAX each differ from the unchanged file's.  At the 10 min step of the GPU test the groups are dense, so a row
    that joins another group cannot move both its extremes: COUNT and SUM differ, and MIN (wrong code above) or MAX
    (wrong code below) does -- 3 * code + row % 3 lies outside every other code's values."""
    base = files[(shape, "int", "plain")]
    k, bw = tg.NVALUES[shape], tg.shape_bw(shape)
    want = _by_tag(base, 10 * tg.MIN)
    sec = (base.ts - tg.T0) // 1000
    cell = sec * (1 << 20) + base.codes
    _, first, count = np.unique(cell, return_index=True, return_counts=True)
    alone = np.zeros(base.rows, bool)
    alone[first[count == 1]] = True
    alone[:k] = False
    changes = {"xor 1": lambda c: c ^ 1, "xor top": lambda c: c ^ (1 << (bw - 1)), "zero": lambda c: 0}
    for label, fn in changes.items():
        rows = [r for r in np.nonzero(alone)[0].tolist() if 0 <= fn(int(base.codes[r])) < k and fn(int(base.codes[r])) != base.codes[r]]
        assert rows, (shape, label)
        r = rows[len(rows) // 2]
        c0, c1 = int(base.codes[r]), fn(int(base.codes[r]))
        bad = tg.File(tmp_path, shape, "int", "plain", patch=(r, c1))
        assert bad.tags[r] == tg.TAGS[c1] and (bad.val == base.val).all() and sum(a != b for a, b in zip(bad.tags, base.tags)) == 1
        around = (int(base.ts[r]) // 1000 * 1000 - 10_000, int(base.ts[r]) // 1000 * 1000 + 10_000)
        got, near = _by_tag(bad, 1000, around), _by_tag(base, 1000, around)
        for agg in ("count", "sum", "min", "max"):
            assert len(near[agg]) > 100 and _differ(got[agg], near[agg], agg), (shape, label, agg, r, c0, c1)
        got = _by_tag(bad, 10 * tg.MIN)
        assert _differ(got["count"], want["count"], "count") and _differ(got["sum"], want["sum"], "sum")
        side = "min" if c1 > c0 else "max"
        assert _differ(got[side], want[side], side), (shape, label, c0, c1)


# ---- the two oracles agree ----
@pytest.mark.parametrize("key", [("wide_257", "int", "nulls"), ("wide_257", "real", "nulls"), ("runs_1025", "int", "plain"),
                                 ("runs_1025", "real", "plain")])
def test_cpu_restatement_agrees(files, key):
    """oracle/cpu (the bench's validator) == the Python oracle on the NULL file at the LUT_CAP edge and on the short
    runs, by tag and under a tag leaf, per glob and merged."""
    from lakeside_amd import synth
    from oracle import cpu, dataexpr as dx
    f = files[key]
    calls = [(tg.all_names(), [f.col], "sum"), (tg.all_names(), [f.col], "min"), (tg.tag_filters(key[0])[0][1], [tg.NAME, f.col], "max"),
             (tg.tag_filters(key[0])[2][1], [tg.NAME], "count"), (tg.tag_filters(key[0])[3][1], [tg.NAME], "avg")]
    if key[2] == "nulls":
        calls += [(q, [tg.NAME], "count") for _, q in tg.null_filters(key[0])]
    for filt, gbs, agg in calls:
        pr = dx.parse_pushdown(json.dumps(synth.pushdown(filt, tg.segs(1, 4 * tg.MIN), agg, gbs)))
        want = dx.evaluate_per_glob(pr, [f.path], 1, sources=[f.blob])
        got = cpu.evaluate_per_glob(pr, [f.blob], 1, threads=4)
        assert len(want) == len(got) == 1
        assert_rows_equal(got[0], want[0], agg, f"cpu {key} {agg} {gbs}")
        assert_rows_equal(cpu.evaluate_merged(pr, [f.blob], 1, threads=4), dx.evaluate_merged(pr, [f.path], 1, sources=[f.blob]),
                          agg, f"cpu merged {key} {agg} {gbs}")
