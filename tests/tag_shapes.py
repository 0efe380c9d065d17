"""Small Parquet files that give a TAG column -- a filter key and group dim, not the name -- every index width from 1 to
17 bits and chunk dictionaries on both sides of the kernels' LDS lookup cap (LUT_CAP, 256 entries), and the requests
that run over them: shared by the CPU pin (test_tag_shapes_cpu.py, through `load_check --tiles=<column>`) and the GPU
test (test_gpu_tag_shapes.py).  No test in here.

Every file is written with pyarrow: no compression, dictionary pages on the string columns, PLAIN timestamps, values
and attr.dur, sorted NULL-free timestamps from synth.T0 over ten minutes, four names metric_00..03 without a NULL (so
scan_lean takes the tiles and the tag is its late column), attr.dur INT64 >= 0 without a NULL (the `rows` route's
numeric leaf passes every row), a message column (exemplar rows project it), row counts odd and no multiple of 64,
everything seeded.  pyarrow numbers a chunk dictionary by first occurrence, so a row group opens with the tag's values
in code order: code c is the value t%06d % c (TAGS[c]).

Values: `int` is 3 * code + row % 3 (NULL: code -1), so a row decoded as another code moves a value no other code
holds from one group to another; `real` is lognormal.

Shapes (SHAPES: label -> builder), 20,011 rows and 8,192-B pages unless stated:
  wide_K       K values, K = 2^(w-1) + 1 for w = 1..13 (bw = w) and the full widths 64, 128, 256; wide_256 / wide_257 is
               the LUT_CAP edge, wide_128 / wide_129 the edge of scan_lean's per-chunk late decode (bw <= 7)
  wide_65537   70,001 rows: the pages' bw grows 13..17 with the dictionary
  growing_300  30,011 rows, 2,048-B pages: the rows draw from the first 2, 4, 16, 64, 128, 200, 256, 257, 300 values in
               stages, so narrow pages (the 96-bit window) lie under one 300-entry chunk dictionary (no LDS lookup)
  runs_129 / runs_1025
               one tag page (32-KiB pages: the other columns have several): RLE runs of 8-40 rows mixed with literal
               stretches of 1-29 (clu_shapes._short_runs), so bit-packed runs start at rows that are no multiple of 8,
               tiles are cut at RUN_CAP (128) runs, and the tiles cut by another column's page start inside a run
  two_dicts    row groups of 10,000 rows: 129 values, then 300 introduced in descending order, then an 11-row group
  absent       wide_33 without the tag column
Every wide_* shape also exists with 10 % NULLs in the tag column (`nulls`; the first K rows are spared, or pyarrow's
dictionary loses entries): the value index then differs from the row index.

Column names: the engine numbers an unrestricted group dim over every value its dictionary of that column NAME holds,
so shapes up to K = 513 (with growing_300, runs_129, two_dicts) share attr.tag and the wider ones attr.tagw."""
import os

import numpy as np

from tests import filter_trees as ft

NAME, VALUE, TIMESTAMP, DUR = ft.NAME, ft.VALUE, ft.TIMESTAMP, ft.DUR
MESSAGE = "_cardinalhq.message"
TAG, TAGW = "attr.tag", "attr.tagw"
T0 = ft.T0
MIN = 60_000
ROWS = 20011
NAMES = [f"metric_{i:02d}" for i in range(4)]
TAGS = [f"t{c:06d}" for c in range(65537)]
NO_SUCH = "t999999"
LUT_CAP, RUN_CAP = 256, 128

WIDE_K = [2, 3, 5, 9, 17, 33, 64, 65, 128, 129, 256, 257, 513, 1025, 2049, 4097]
BIG_K, BIG_ROWS = 65537, 70001
# wide_K: K -> the bw of every tile (dict_n == K), as pyarrow writes the pages (pinned by test_tag_shapes_cpu.py)
EXPECT = {k: max(1, (k - 1).bit_length()) for k in WIDE_K}
BIG_BW = {13, 14, 15, 16, 17}
GROWING_ROWS = 30011
GROWING_STAGES = [(2, 2600), (4, 2600), (16, 3000), (64, 3200), (128, 3400), (200, 3600), (256, 3800), (257, 3400), (300, None)]
GROWING_BW = {2, 4, 6, 7, 8, 9}
TWO_DICTS_RG = 10000


def tag_column(shape):
    if shape.startswith("wide_"):
        return TAG if int(shape[5:]) <= 513 else TAGW
    return TAGW if shape == "runs_1025" else TAG


def _draw(rng, k, n):
    """n codes below k, the first min(k, n) being 0, 1, 2 ..: code == position."""
    c = rng.integers(0, k, n)
    c[:min(n, k)] = np.arange(min(n, k))
    return c


def _wide(k, rows=ROWS):
    def build(rng):
        return _draw(rng, k, rows), dict(row_group_size=rows, data_page_size=8192)
    return build


def _growing(rng):
    parts, have, left = [], 0, GROWING_ROWS
    for k, rows in GROWING_STAGES:
        rows = left if rows is None else rows
        p = rng.integers(0, k, rows)
        p[:k - have] = np.arange(have, k)      # the stage's new values, in order: code == value index
        parts.append(p)
        have, left = k, left - rows
    return np.concatenate(parts), dict(row_group_size=GROWING_ROWS, data_page_size=2048)


def _runs(k):
    def build(rng):
        codes = list(range(k))
        while len(codes) < ROWS:
            if rng.random() < 0.7:
                codes += [int(rng.integers(0, k))] * int(rng.integers(8, 41))
            else:
                codes += [int(c) for c in rng.integers(0, k, int(rng.integers(1, 30)))]
        return np.asarray(codes[:ROWS]), dict(row_group_size=ROWS, data_page_size=32768, max_rows_per_page=1 << 20)
    return build


def _two_dicts(rng):
    """The codes here are VALUE indices (TAGS[c]); the second group's chunk codes run opposite to them."""
    a = _draw(rng, 129, TWO_DICTS_RG)
    b = 299 - _draw(rng, 300, TWO_DICTS_RG)
    c = _draw(rng, 129, ROWS - 2 * TWO_DICTS_RG)
    return np.concatenate([a, b, c]), dict(row_group_size=TWO_DICTS_RG, data_page_size=8192)


SHAPES = {f"wide_{k}": _wide(k) for k in WIDE_K}
SHAPES.update({f"wide_{BIG_K}": _wide(BIG_K, BIG_ROWS), "growing_300": _growing, "runs_129": _runs(129),
               "runs_1025": _runs(1025), "two_dicts": _two_dicts, "absent": _wide(33)})
WIDE = [s for s in SHAPES if s.startswith("wide_")]
BIG = f"wide_{BIG_K}"
# the values a shape's file holds, and the width of its widest page (the leaves of stratum (b) are cut from it)
NVALUES = {s: int(s.split("_")[1]) for s in SHAPES if s != "two_dicts" and s != "absent"}
NVALUES.update({"two_dicts": 300, "absent": 0})
# per shape: the seed's last word, chosen once so that the pins of test_tag_shapes_cpu.py hold
SALT = {"runs_1025": 2}


def labels():
    """[(shape, flavour, variant)] of every file."""
    out = []
    for s in SHAPES:
        for f in ("int", "real"):
            out.append((s, f, "plain"))
            if s in WIDE:
                out.append((s, f, "nulls"))
    return out


class File:
    """One file.  `patch` = (row, code): that row carries another code's value (the CPU sensitivity test: what a
    decoder that got one row wrong would have read); its value column is unchanged."""

    def __init__(self, dirpath, shape, flavour, variant="plain", patch=None):
        import pyarrow as pa
        import pyarrow.parquet as pq
        si = sorted(SHAPES).index(shape)
        rng = np.random.default_rng([41, si, SALT.get(shape, 0)])
        self.shape, self.flavour, self.variant = shape, flavour, variant
        self.col = tag_column(shape)
        codes, opts = SHAPES[shape](rng)
        n = self.rows = len(codes)
        self.ts = T0 + np.sort(rng.integers(0, 10 * MIN, n))
        self.names = np.asarray(NAMES, dtype=object)[rng.integers(0, len(NAMES), n)]
        self.dur = rng.integers(0, 5_000_000, n)
        self.msg = rng.integers(0, 9, n)
        null = np.zeros(n, bool)
        if variant == "nulls":
            null = np.random.default_rng([43, si]).random(n) < 0.1
            null[:NVALUES[shape]] = False
        self.codes = np.where(null, -1, codes)
        vrng = np.random.default_rng([47, si, ("int", "real").index(flavour), variant == "nulls"])
        self.val = ((3 * self.codes + np.arange(n) % 3).astype(np.float64) if flavour == "int"
                    else vrng.lognormal(0.0, 2.0, n))
        if patch is not None:
            assert self.codes[patch[0]] >= 0 and patch[0] >= NVALUES[shape]
            self.codes = self.codes.copy()
            self.codes[patch[0]] = patch[1]
        self.tags = [None if c < 0 else TAGS[c] for c in self.codes.tolist()]
        cols = {TIMESTAMP: pa.array(self.ts, pa.int64()), VALUE: pa.array(self.val, pa.float64()),
                NAME: pa.array(self.names.tolist(), pa.string())}
        if shape != "absent":
            cols[self.col] = pa.array(self.tags, pa.string())
        cols[DUR] = pa.array(self.dur, pa.int64())
        cols[MESSAGE] = pa.array([f"line {k}" for k in self.msg], pa.string())
        strings = [c for c in cols if c in (NAME, TAG, TAGW, MESSAGE)]
        tail = "" if patch is None else f"_{patch[0]}_{patch[1]}"
        self.path = os.path.join(str(dirpath), f"tag_{shape}_{flavour}_{variant}{tail}.parquet")
        pq.write_table(pa.table(cols), self.path, compression="NONE", use_dictionary=strings,
                       column_encoding={c: "PLAIN" for c in cols if c not in strings}, **opts)
        with open(self.path, "rb") as f:
            self.blob = f.read()

    def present(self):
        """The tag values of the file, in value order."""
        return sorted({t for t in self.tags if t is not None})


def make_files(dirpath, which=None):
    """{(shape, flavour, variant): File} of `which` (default: every file)."""
    return {k: File(dirpath, *k) for k in (labels() if which is None else which)}


# ---- requests ----
def leaf(col, op, *v):
    return {"k": col, "v": list(v), "op": op, "extracted": False, "computed": False, "dataType": "string"}


def all_names():
    return leaf(NAME, "in", *NAMES)


def with_names(q):
    """`name in (all four) and q`: the name is the early column, the tag's conjunct the late filter."""
    return {"op": "and", "q1": all_names(), "q2": q}


def shape_bw(shape):
    """The width of the shape's widest page."""
    return max(1, (NVALUES[shape] - 1).bit_length())


def edge_values(shape):
    """The values of code 0, of code 2^(bw-1) - 1, of code 2^(bw-1) (the first that needs the top bit) and of the last
    code, and a value no file holds.  (two_dicts: value indices; its second chunk numbers them from the other end.
    Two or three values: the last code alone, or `not (in ..)` would pass no row.)"""
    k, bw = NVALUES[shape], shape_bw(shape)
    half = 1 << (bw - 1)
    if k <= 3:
        return [TAGS[k - 1], NO_SUCH]
    return sorted({TAGS[0], TAGS[min(k - 1, max(0, half - 1))], TAGS[min(k - 1, half)], TAGS[k - 1]}) + [NO_SUCH]


def tag_filters(shape):
    """Stratum (b): [(label, filter)] with a leaf on the shape's tag column."""
    col, k = tag_column(shape), NVALUES[shape]
    edge = leaf(col, "in", *edge_values(shape))
    return [("in edges", with_names(edge)), ("ne last", with_names(leaf(col, "!=", TAGS[k - 1]))),
            ("regex half", with_names(leaf(col, "regex", "[02468]$"))), ("not in edges", with_names({"not": edge}))]


def null_filters(shape):
    """Stratum (c): exists / not exists on the tag column."""
    col = tag_column(shape)
    return [("exists", with_names(leaf(col, "exists"))), ("not exists", with_names({"not": leaf(col, "exists")}))]


def with_dur(q):
    """The `rows` route: a numeric leaf every row passes sends every segment to the general row scan (ex_scan AGG)."""
    return {"op": "and", "q1": q, "q2": {"k": DUR, "v": ["0"], "op": "ge", "extracted": False, "computed": False,
                                         "dataType": "number"}}


def segs(n, step):
    from lakeside_amd import synth
    return [synth.segment_request(j, step=step, hour=0) for j in range(n)]


def widths(shape):
    """The index widths of the shape's tag-column tiles (pinned by test_tag_shapes_cpu.py)."""
    if shape in (BIG, "growing_300", "two_dicts", "absent"):
        return {BIG: BIG_BW, "growing_300": GROWING_BW, "two_dicts": {4, 8, 9}, "absent": set()}[shape]
    return {shape_bw(shape)}
