"""scan_clu's boundary search fed from the clustered copy's timestamp sample tables (clu.hpp: entry s of a tile's table
is the timestamp of row (s * nrows) >> 8, written at load by clu_samp_build in front of the sub-block area) on the
MI355X.

Files: sorted one- to three-tile Parquet files (pyarrow: a row group of one page per tile) with tiles of NROWS rows.
Tile i of a file covers [B, B + 3 steps), B = T0 + 3 i steps, at a 5 min step: rows [0, c0) in the last 10 s of the
first bucket, rows [c0, c1) over the second bucket (row c0 exactly on its first millisecond), rows [c1, n) in the first
5 s of the third (row c1 exactly on its first millisecond).  The cuts (c0, c1) of a tile are one of PATTERNS: a bucket
boundary on row 0, on the last row, exactly on a sample row and one row either side of one, on the 4,096-row sub-block
edges, and in the middle -- one or two boundaries inside the tile.  Every file is evaluated over the whole hour and
with the window cut inside the first tile's first rows and inside the last tile's last rows (a third boundary in those
tiles, and classes outside the window).

Each evaluation (sum, min, max, count, avg; two of three names pass, grouped by name; integral values, so sums are exact
in any order) is made as it stands, with LK_NO_CLU_SAMP=1, LK_NO_CLU_SUB=1 and LK_NO_CLU_AGG=1 on the session's engine,
and as it stands on an engine created with {"cluster_samples": false} (the sub-block area alone, no table): the
oracle's rows each time, the same rows bit for bit.

Plan bytes (LK_PLAN_BYTES) are the evidence of the route.  The table costs a split tile 16 lines whatever its rows; the
search without it counts the distinct 128-B lines its 256 samples touch in the timestamp column, which depends on the
stream's alignment: between lines(n, a) over the alignments a -- 256 for a tile of 4,096 rows or more, 16 or 17 at 256
and 257 rows (the samples are rows 0 .. 255), one line for a row or two.  So over the split tiles of a call
    128 * sum(min_a lines - 16)  <=  plan_bytes(LK_NO_CLU_SAMP=1) - plan_bytes  <=  128 * sum(max_a lines - 16)
and the difference is positive wherever a split tile has 4,095 rows or more and negative where it has a few rows; the engine
without the tables counts what LK_NO_CLU_SAMP=1 counts, with and without the switch."""
import json
import os

import numpy as np
import pytest

from tests.parity import assert_rows_equal
from tests.test_gpu_clustered import NAME, _bits, _Env

pytestmark = pytest.mark.gpu

STEP = 300_000
HOUR = 3_600_000
SUB = 4096
NSAMP = 256
NROWS = [1, 2, 255, 256, 257, 4095, 4096, 4097, 65535, 65536]
AGGS = ["sum", "min", "max", "count", "avg"]
MODES = (("table", {}), ("nosamp", {"LK_NO_CLU_SAMP": 1}), ("nosub", {"LK_NO_CLU_SUB": 1}), ("noagg", {"LK_NO_CLU_AGG": 1}))


def tiles_per_file(n):
    return 3 if n <= 4097 else (2 if n == 65535 else 1)


def patterns(n):
    """The cuts (c0, c1), 0 <= c0 <= c1 <= n, of the tiles of n rows, without repeats."""
    rs = (100 * n) >> 8                                  # a sample row away from the ends (row 0 below 3 rows)
    mid = n // 2
    raw = [(0, mid),                                     # the tile opens on a bucket's first millisecond: boundary on row 0
           (mid, n - 1),                                 # the last row alone in the third bucket
           (rs, n),                                      # a boundary exactly on a sample row
           (rs - 1, rs + 1),                             # one row either side of it
           (SUB, 2 * SUB),                               # on sub-block edges
           (mid // 2, mid + 1)]
    out = []
    for c0, c1 in raw:
        c0 = min(max(c0, 0), n)
        c1 = min(max(c1, c0), n)
        if (c0, c1) not in out:
            out.append((c0, c1))
    return out


def tile_ts(rng, n, cuts, base):
    c0, c1 = cuts
    a = np.sort(rng.integers(STEP - 10_000, STEP, c0))
    b = np.sort(rng.integers(STEP, 2 * STEP, c1 - c0))
    c = np.sort(rng.integers(2 * STEP, 2 * STEP + 5_000, n - c1))
    if len(b):
        b[0] = STEP
    if len(c):
        c[0] = 2 * STEP
    return base + np.concatenate([a, b, c]).astype(np.int64)


class File:
    def __init__(self, root, n, index, cuts_of_tiles):
        import pyarrow as pa
        import pyarrow.parquet as pq
        from lakeside_amd import synth
        from oracle import dataexpr as dx
        rng = np.random.default_rng([977, n, index])
        self.n, self.tiles = n, len(cuts_of_tiles)
        self.ts = [tile_ts(rng, n, c, synth.T0 + 3 * STEP * i) for i, c in enumerate(cuts_of_tiles)]
        rows = n * self.tiles
        if n > 2 * SUB:
            # names in runs of 1,024 rows: a tile's name column stays below the loader's cap of 128 runs, which would
            # otherwise cut a row group of this size into two tiles
            names = np.concatenate([np.repeat(np.concatenate([["a", "b"], rng.choice(["a", "b", "c"], (n + 1023) // 1024 - 2)]),
                                              1024)[:n] for _ in range(self.tiles)]).astype(object)
        else:
            names = rng.choice(["a", "b", "c"], rows).astype(object)
            for i in range(self.tiles):                  # every tile holds a passing name
                names[i * n] = "a"
                if n > 1:
                    names[i * n + 1] = "b"
        val = rng.integers(-500, 500, rows).astype(np.float64)
        self.path = os.path.join(str(root), f"samp_{n}_{index}.parquet")
        t = pa.table({dx.TIMESTAMP: pa.array(np.concatenate(self.ts), pa.int64()), dx.VALUE: pa.array(val, pa.float64()),
                      dx.NAME: pa.array(list(names), pa.string())})
        pq.write_table(t, self.path, compression="NONE", use_dictionary=[dx.NAME], row_group_size=n,
                       data_page_size=1 << 22, max_rows_per_page=1 << 20,
                       column_encoding={dx.TIMESTAMP: "PLAIN", dx.VALUE: "PLAIN"})
        with open(self.path, "rb") as f:
            self.blob = f.read()
        self.cells = {}                                  # window -> oracle cells

    def windows(self):
        """The whole hour, and a window that opens 5 s before the first tile's second bucket and closes 2.5 s into
        the last tile's third."""
        return [None, (STEP - 5_000, HOUR - (3 * STEP * (self.tiles - 1) + 2 * STEP + 2_500))]

    def split_tiles(self, window):
        """The tiles the clustered copy's rule (clu.hpp, clu_classify) makes split tiles in this window."""
        from lakeside_amd import synth
        lo = synth.T0 + (window[0] if window else 0)
        hi = synth.T0 + HOUR - (window[1] if window else 0)
        out = 0
        for ts in self.ts:
            tmin, tmax = int(ts[0]), int(ts[-1])
            if tmax < lo or tmin >= hi:
                continue
            if tmin >= lo and tmax < hi and tmin // STEP == tmax // STEP:
                continue
            out += 1
        return out


def lines_range(n):
    """(fewest, most) distinct 128-B lines the 256 sampled rows of a tile of n rows touch, over the stream's
    alignments (8-B steps)."""
    rows = sorted({(s * n) >> 8 for s in range(NSAMP)})
    counts = [len({(a + 8 * r) // 128 for r in rows}) for a in range(0, 128, 8)]
    return min(counts), max(counts)


def test_lines_of_the_scattered_samples():
    assert lines_range(65536) == (256, 256) and lines_range(4096) == (256, 256)
    assert lines_range(4095)[0] >= 240 and lines_range(257) == lines_range(256) == (16, 17) and lines_range(1) == (1, 1)


@pytest.fixture(scope="module")
def old_engine():
    from lakeside_amd.evaluator import Engine
    e = Engine(0, cluster_samples=False)
    yield e
    e.close()


_files = {}


@pytest.fixture(scope="module")
def files(engine, old_engine, tmp_path_factory):
    root = tmp_path_factory.mktemp("clu_samples")

    def get(n):
        if n not in _files:
            pats, k = patterns(n), tiles_per_file(n)
            _files[n] = [File(root, n, i, pats[j:j + k]) for i, j in enumerate(range(0, len(pats), k))]
            for f in _files[n]:
                engine.load_segment(f.path)
                old_engine.load_segment(f.path)
        return _files[n]
    yield get
    _files.clear()


def test_engine_sample_bytes(engine, old_engine, files):
    """2,048 B per tile, reported as `clu_samp_bytes` and part of `segment_bytes`; the sub-block areas keep their size
    (three names: clu_sub_bytes(3) = 1,792 B per tile).  None on an engine created without the tables.  The tables
    belong to the timestamp column, so an engine without the value copy keeps them too."""
    from lakeside_amd.evaluator import Engine
    fs = files(257)
    tiles = sum(f.tiles for f in fs)
    weight = {}
    for cs, cv, sub, samp in ((None, None, 1792, 2048), (False, None, 1792, 0), (None, False, 0, 2048), (False, False, 0, 0)):
        eng = Engine(0, cluster_samples=cs, cluster_values=cv)
        try:
            for f in fs:
                eng.load_segment(f.path)
            st = eng.stats
            assert st["clu_sub_bytes"] == tiles * sub and st["clu_samp_bytes"] == tiles * samp, (cs, cv, st)
            weight[(cs, cv)] = eng.segment_bytes
        finally:
            eng.close()
    assert weight[(None, None)] - weight[(False, None)] == tiles * 2048 == weight[(None, False)] - weight[(False, False)]
    assert old_engine.stats["clu_samp_bytes"] == 0 and engine.stats["clu_samp_bytes"] > 0


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("nrows", NROWS)
def test_sample_table_route(engine, old_engine, files, nrows, agg):
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES, synth
    from oracle import dataexpr as dx
    lo, hi = lines_range(nrows)
    filt = synth.leaf(NAME, "in", "a", "b")
    split_seen = 0
    for f in files(nrows):
        for window in f.windows():
            seg = synth.segment_request(0, step=STEP, hour=0)
            if window:
                seg["startTs"] += window[0]
                seg["endTs"] -= window[1]
            req = json.dumps(synth.pushdown(filt, [seg], agg, [NAME]))
            pr = dx.parse_pushdown(req)
            if window not in f.cells:
                f.cells[window] = dx.evaluate_glob_cells(pr, 10, [f.path], sources=[f.blob])
            want = dx.merge_glob_cells(pr, f.cells[window])
            label = f"{nrows} rows, file {os.path.basename(f.path)}, window {window}, {agg}"
            out = {}
            for mode, env in MODES:
                with _Env(**env):
                    out[mode] = engine.eval_pushdown(req, [f.path], 10, LK_MERGED | LK_PLAN_BYTES)
            out["old"] = old_engine.eval_pushdown(req, [f.path], 10, LK_MERGED | LK_PLAN_BYTES)
            with _Env(LK_NO_CLU_SAMP=1):
                out["old nosamp"] = old_engine.eval_pushdown(req, [f.path], 10, LK_MERGED | LK_PLAN_BYTES)
            ref = out["table"]
            for mode, r in out.items():
                assert_rows_equal(r.rows(), want, agg, f"{label} {mode}")
                assert r.stats["clustered"] == 1 and r.stats["clustered_tiles"] == r.stats["tiles"] == f.tiles, (label, mode, r.stats)
                assert r.ts.tolist() == ref.ts.tolist() and r.tags == ref.tags, (label, mode)
                assert _bits(r.values) == _bits(ref.values), f"{label}: {mode} rows differ"
            # the route: 16 lines per split tile from the table, the samples' own lines without it
            split = f.split_tiles(window)
            split_seen += split
            pb = {m: r.stats["plan_bytes"] for m, r in out.items()}
            print(label, "split tiles", split, "plan bytes", pb)
            d = pb["nosamp"] - pb["table"]
            assert 128 * split * (lo - 16) <= d <= 128 * split * (hi - 16), (label, split, pb)
            if nrows >= 4095 and split:
                assert d > 0, (label, pb)
            assert pb["old"] == pb["old nosamp"] == pb["nosamp"], (label, pb)
    assert split_seen > 0 or nrows == 1                  # a tile of one row is pinned or outside the window
