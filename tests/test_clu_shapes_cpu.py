"""Pins the fixtures of tests/clu_shapes.py without a GPU, so that a pyarrow that cuts other pages, or a seed that makes
other trees, is noticed here and not as a silently weaker tests/test_gpu_clu_shapes.py.

The files' tiles are read with `build/load_check --tiles` (tools/load_check.cpp: the loader's own TileDesc / TileCol of
the name column, what Engine::build_cluster and the kernels see); the whole-segment rule is lk_clu_segment_taken of
liblakeside_text.so (clu.hpp).  The name-only trees are pinned against the oracle alone (oracle/dataexpr.py), by the
rule DESIGN section 3.1 states for the filter fuzz: per file set at most a quarter of the trees pass no row or every
row, one passes under 5 % of the rows and one over 60 %."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import clu_shapes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
PAGE_DICT, RUN_CAP = 2, 128


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return cs.make_files(tmp_path_factory.mktemp("clu_shapes"))


@pytest.fixture(scope="module")
def tiles(files):
    """{(shape, flavour): [tile: {field: int}]} from one run of the harness over every file."""
    subprocess.run(["make", "-C", ROOT, "build/load_check"], check=True, capture_output=True)
    keys = list(files)
    out = subprocess.run([os.path.join(ROOT, "build", "load_check"), "--tiles", "1"] + [files[k].path for k in keys],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    by_base = {os.path.basename(files[k].path): k for k in keys}
    res, cur = {}, None
    for line in out.splitlines():
        head = line.split(" ", 1)[0]
        if head in by_base:
            assert " error" not in line, line
            cur = res.setdefault(by_base[head], [])
        elif line.startswith("  tile "):
            f = line.split()
            t = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
            assert int(f[1]) == len(cur)
            cur.append(t)
    assert out.splitlines()[-1] == "failures=0" and set(res) == set(keys)
    for k in keys:
        assert sum(t["nrows"] for t in res[k]) == files[k].rows, k
    return res


def _shape(tiles, shape):
    """The tiles of a shape's flavours (the flavours differ by their values alone: the same pages)."""
    return [tiles[k] for k in tiles if k[0] == shape]


def test_without_the_flag_nothing_changes(files):
    subprocess.run(["make", "-C", ROOT, "build/load_check"], check=True, capture_output=True)
    exe = os.path.join(ROOT, "build", "load_check")
    paths = [files[("uniform_05", "int")].path, files[("two_dicts_4k", "real")].path]
    plain = subprocess.run([exe, "1"] + paths, check=True, capture_output=True, text=True).stdout
    flag = subprocess.run([exe, "--tiles", "1"] + paths, check=True, capture_output=True, text=True).stdout
    assert "  tile " not in plain
    assert [l for l in flag.splitlines() if not l.startswith("  tile ")] == plain.splitlines()
    assert sum(l.startswith("  tile ") for l in flag.splitlines()) > 20


def test_every_tile_is_sorted_and_null_free(tiles):
    for k, ts in tiles.items():
        for t in ts:
            assert t["sorted"] == 1 and t["has_nulls"] == 0 and t["kind"] == PAGE_DICT and 1 <= t["nruns"] <= RUN_CAP, (k, t)
            assert t["span"] >= 0


def test_widest_tile_is_below_two_steps(tiles):
    """Every file is taken whole by scan_clu at every step it is queried at (the 65-name file by its tiles' width: it
    gets no copy for its dictionary)."""
    L = ctypes.CDLL(LIB)
    L.lk_clu_segment_taken.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    L.lk_clu_segment_taken.restype = ctypes.c_int
    for k, ts in tiles.items():
        widest = max(t["span"] for t in ts)
        for step in cs.STEPS[k[0]]:
            assert L.lk_clu_segment_taken(1, widest, step) == 1, (k, widest, step)
        assert L.lk_clu_segment_taken(1, widest, widest // 2) == 0   # (the rule does refuse a tile of two steps)


@pytest.mark.parametrize("k", cs.UNIFORM_K)
def test_uniform(tiles, k):
    for ts in _shape(tiles, f"uniform_{k:02d}"):
        assert {(t["dict_n"], t["bw"]) for t in ts} == {cs.EXPECT[k]}, k
        assert 15 <= len(ts) <= 25 and all(t["rg"] == 0 for t in ts)
        assert ts[-1]["nrows"] % 64 != 0


def test_growing(tiles):
    for ts in _shape(tiles, "growing"):
        assert {t["dict_n"] for t in ts} == {64}
        assert {t["bw"] for t in ts} == {1, 2, 3, 4, 5, 6}
        # a tile that starts inside a run of its page: the first run begins before the tile's first value
        assert any(t["vbase"] > t["run0_start"] for t in ts)
        assert any(t["vbase"] > t["run0_start"] and t["run0_lit"] == 1 for t in ts)


def test_short_runs(tiles):
    for ts in _shape(tiles, "short_runs"):
        full = [t for t in ts if t["nruns"] == RUN_CAP]
        assert len(full) >= 3 and {t["run0_lit"] for t in full} == {0, 1}, [(t["nruns"], t["run0_lit"]) for t in ts]
        assert {(t["dict_n"], t["bw"]) for t in ts} == {(40, 6)}


def test_two_dicts(tiles):
    for shape in ("two_dicts_4k", "two_dicts_1m"):
        for ts in _shape(tiles, shape):
            assert [(t["dict_n"], t["bw"]) for t in ts if t["rg"] == 0][0] == (5, 3)
            assert {(t["rg"], t["dict_n"], t["bw"]) for t in ts} == {(0, 5, 3), (1, 33, 6), (2, 5, 3)}
            if shape == "two_dicts_1m":
                assert [t["nrows"] for t in ts] == [cs.TWO_DICTS_RG, cs.TWO_DICTS_RG, cs.ROWS - 2 * cs.TWO_DICTS_RG]
            else:
                assert len(ts) >= 15


@pytest.mark.parametrize("k", [7, 64])
def test_big_tile(tiles, files, k):
    for ts in _shape(tiles, f"big_tile_{k:02d}"):
        assert len(ts) == 1 and ts[0]["nrows"] == cs.ROWS and (ts[0]["dict_n"], ts[0]["bw"]) == cs.EXPECT[k]
    # the 10 min boundary's row lies strictly inside the third of five sub-blocks
    f = files[(f"big_tile_{k:02d}", "nan")]
    cut = int(np.searchsorted(f.ts, cs.T0 + 10 * cs.MIN))
    assert 2 * cs.SUB < cut < 3 * cs.SUB and (cs.ROWS + cs.SUB - 1) // cs.SUB == 5
    nan_rows = np.nonzero(np.isnan(f.val))[0]
    assert set((nan_rows // cs.SUB).tolist()) == {1, 3} and set(f.names[nan_rows].tolist()) == {cs.NAMES[k - 1]}


@pytest.mark.parametrize("k", [7, 64])
def test_codes_follow_the_names(files, k):
    """pyarrow numbers the chunk dictionary by first occurrence: the files open with their names in order, so code c is
    metric_c and the NaN flavours' NaNs sit in the last code (lane dict_n - 1, bit dict_n - 1 of the tile's NaN mask)."""
    import io

    import pyarrow.parquet as pq
    for shape in (f"uniform_{k:02d}", f"big_tile_{k:02d}"):
        f = files[(shape, "nan")]
        col = pq.ParquetFile(io.BytesIO(f.blob), read_dictionary=[cs.NAME]).read_row_group(0, columns=[cs.NAME]).column(0)
        assert col.chunk(0).dictionary.to_pylist() == cs.NAMES[:k]
        assert set(f.names[np.isnan(f.val)].tolist()) == {cs.NAMES[k - 1]}
    f = files[(f"uniform_{k:02d}", "nan")]
    last = f.names == cs.NAMES[k - 1]
    early = f.ts < cs.T0 + 5 * cs.MIN
    assert np.isnan(f.val[last & early]).all() and last[early].sum() >= 10       # cells of NaN alone
    late = f.val[last & ~early]
    assert np.isnan(late).any() and not np.isnan(late).all()                      # and cells that mix


def test_descending_codes(files):
    import io

    import pyarrow.parquet as pq
    f = files[("two_dicts_4k", "int")]
    col = pq.ParquetFile(io.BytesIO(f.blob), read_dictionary=[cs.NAME]).read_row_group(1, columns=[cs.NAME]).column(0)
    assert col.chunk(0).dictionary.to_pylist() == cs.NAMES[52:19:-1]


# ---- the name-only trees, against the oracle alone ----
def _passing(files, shapes, flavour, tree, window):
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    fs = [files[(s, flavour)] for s in shapes]
    segs = [synth.segment_request(j, step=60_000, hour=0) for j in range(len(fs))]
    for s in segs:
        s["startTs"], s["endTs"] = window
    pr = dx.parse_pushdown(json.dumps(synth.pushdown(tree, segs, "count", [])))
    cells = dx.evaluate_glob_cells(pr, len(fs), [f.path for f in fs], sources=[f.blob for f in fs])
    rows = sum(int(((f.ts >= window[0]) & (f.ts < window[1])).sum()) for f in fs)
    return sum(c.rows for g in cells for c in g), rows


def test_trees_are_not_vacuous(files):
    per_set = {}
    for i in range(cs.N_TREES):
        si, flavour, _, _, _, _, cut = cs.tree_case(i)
        lo, hi = cs.cut_window(cs.TREE_SETS[si]) if cut else (0, 0)
        got, rows = _passing(files, cs.TREE_SETS[si], flavour, cs.tree(i), (cs.T0 + lo, cs.T0 + cs.ft.HOUR - hi))
        per_set.setdefault(si, []).append((got, rows))
    assert sorted(per_set) == list(range(len(cs.TREE_SETS)))
    for si, pr in per_set.items():
        frac = [g / r for g, r in pr]
        degenerate = sum(g == 0 or g == r for g, r in pr)
        assert 4 * degenerate <= len(pr), f"set {si}: {degenerate} of {len(pr)} trees pass no row or every row"
        assert min(f for f in frac if f > 0) < 0.05 and max(f for f in frac if f < 1) > 0.60, f"set {si}: {sorted(frac)}"


def test_hand_written_trees(files):
    """The literal trees pass what their text says, on the 33-name file and the file of two dictionaries."""
    shapes = ["uniform_33", "two_dicts_4k"]
    fs = [files[(s, "int")] for s in shapes]
    names = np.concatenate([f.names for f in fs])
    want = {"not in": ~np.isin(names, ["metric_00", "metric_02", "metric_21", "metric_33"]),
            "ne or regex": names != "metric_01", "exists": np.ones(len(names), bool),
            "not exists": np.zeros(len(names), bool)}
    has = lambda sub: np.array([sub in n for n in names])   # noqa: E731
    want["six leaves"] = (has("c_0") & (names != "metric_01")) | ~has("7")
    for label, tree in cs.HAND_TREES:
        got, rows = _passing(files, shapes, "int", tree, (cs.T0, cs.T0 + cs.ft.HOUR))
        assert rows == len(names) and got == int(want[label].sum()), label
