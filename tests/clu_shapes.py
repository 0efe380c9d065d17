"""Small Parquet files that give the name-clustered value copy (clu_build / scan_clu; with LK_NO_CLUSTER=1 scan_lean and
scan_tiles) every chunk-dictionary size and index width it admits, and the name-only filter trees that run over them:
shared by the CPU pin (test_clu_shapes_cpu.py, through `load_check --tiles`) and the GPU test (test_gpu_clu_shapes.py).
No test in here.

Every file is written with pyarrow: no compression, dictionary pages on the name column only, PLAIN timestamps and
values, sorted NULL-free timestamps from synth.T0, names metric_00 .. metric_64 (so filter_trees' literals, patterns
and substrings apply), row counts odd and no multiple of 64, everything seeded.  pyarrow numbers a chunk dictionary by
first occurrence, so wherever a code must be a known name the row group opens with the names in code order.

Files (SHAPES: label -> builder), each in an integral (`int`: integers in [-500, 500)) and a real (`real`: lognormal)
flavour; `nan` is the real flavour with NaNs in the rows of the row group's last code:

  uniform_KK   KK names, 20,011 rows over 10 min, one row group, 4,096-B pages: about 20 tiles of 1,024 rows and 30 s
               (EXPECT: the dict_n / bw of every KK; 65 names are one past build_cluster's rule: no copy)
  growing      26,003 rows over 13 min, 1,024-B pages; the rows draw from the first 2, 4, 8, 16, 32, 64 names in
               stages, so the pages' bw grows from 1 to 6 under one 64-entry chunk dictionary
  short_runs   40 names in short runs, one page: tiles cut by RUN_CAP (128 runs), RLE and bit-packed runs mixed
  two_dicts_4k / two_dicts_1m
               row groups of 10,000 rows: metric_00..04 (dict_n 5), then metric_52..20 introduced in descending order
               (dict_n 33, codes opposite to the names' order), then an 11-row group; 4,096-B pages / one page a group
  big_tile_KK  20,011 rows in one page over [T0 + 5 min, T0 + 15 min): at a 10 min step the one tile is split by a
               boundary that falls inside its third sub-block (five sub-blocks of 4,096 rows).  `nan`: the last code's
               rows of sub-blocks 1 and 3 are NaN
  uniform_07 / uniform_64 `nan`: every row of the last code is NaN in the first five minutes (cells of NaN alone), three
               in ten of them afterwards."""
import os

import numpy as np

from tests import filter_trees as ft

NAME, VALUE, TIMESTAMP = ft.NAME, ft.VALUE, ft.TIMESTAMP
T0 = ft.T0
MIN = 60_000
ROWS = 20011
SUB = 4096
NAMES = [f"metric_{i:02d}" for i in range(65)]
UNIFORM_K = [1, 2, 3, 5, 7, 8, 17, 32, 33, 63, 64, 65]
# uniform_KK: KK -> (dict_n, bw) of every tile, as pyarrow writes the pages (pinned by test_clu_shapes_cpu.py)
EXPECT = {1: (1, 1), 2: (2, 1), 3: (3, 2), 5: (5, 3), 7: (7, 3), 8: (8, 3), 17: (17, 5), 32: (32, 5), 33: (33, 6),
          63: (63, 6), 64: (64, 6), 65: (65, 7)}
GROWING_ROWS = 26003
GROWING_STAGES = [(2, 9000), (4, 4800), (8, 3200), (16, 2600), (32, 2200), (64, None)]
TWO_DICTS_RG = 10000
TREE_SEED = 3163
N_TREES = 40


def _values(vrng, n, flavour):
    if flavour == "int":
        return vrng.integers(-500, 500, n).astype(np.float64)
    return vrng.lognormal(0.0, 2.0, n)


def _pick(rng, names, n):
    """n draws from `names`, the first len(names) rows being the names in order."""
    out = np.asarray(names, dtype=object)[rng.integers(0, len(names), n)]
    out[:min(n, len(names))] = names[:n]
    return out


def _uniform(k):
    def build(rng, vrng, flavour):
        ts = T0 + np.sort(rng.integers(0, 10 * MIN, ROWS))
        names = _pick(rng, NAMES[:k], ROWS)
        val = _values(vrng, ROWS, flavour)
        if flavour == "nan":
            last = names == NAMES[k - 1]
            early = ts < T0 + 5 * MIN
            val[last & (early | (vrng.random(ROWS) < 0.3))] = np.nan
        return ts, names, val, dict(row_group_size=ROWS, data_page_size=4096)
    return build


def _growing(rng, vrng, flavour):
    n = GROWING_ROWS
    ts = T0 + np.sort(rng.integers(0, 13 * MIN, n))
    parts, have, left = [], 0, n
    for k, rows in GROWING_STAGES:
        rows = left if rows is None else rows
        p = np.asarray(NAMES[:k], dtype=object)[rng.integers(0, k, rows)]
        p[:k - have] = NAMES[have:k]      # the stage's new names, in order: code == name index
        parts.append(p)
        have, left = k, left - rows
    return ts, np.concatenate(parts), _values(vrng, n, flavour), dict(row_group_size=n, data_page_size=1024)


def _short_runs(rng, vrng, flavour):
    names = list(NAMES[:40])
    while len(names) < ROWS:
        if rng.random() < 0.7:
            names += [NAMES[int(rng.integers(0, 40))]] * int(rng.integers(8, 41))
        else:
            names += [NAMES[int(c)] for c in rng.integers(0, 40, int(rng.integers(1, 30)))]
    ts = T0 + np.sort(rng.integers(0, 10 * MIN, ROWS))
    return ts, np.asarray(names[:ROWS], dtype=object), _values(vrng, ROWS, flavour), dict(row_group_size=ROWS,
                                                                                         data_page_size=1 << 20, max_rows_per_page=1 << 20)


def _two_dicts(page):
    def build(rng, vrng, flavour):
        ts = T0 + np.sort(rng.integers(0, 10 * MIN, ROWS))
        names = np.concatenate([_pick(rng, NAMES[0:5], TWO_DICTS_RG), _pick(rng, NAMES[52:19:-1], TWO_DICTS_RG),
                                _pick(rng, NAMES[0:5], ROWS - 2 * TWO_DICTS_RG)])
        return ts, names, _values(vrng, ROWS, flavour), dict(row_group_size=TWO_DICTS_RG, data_page_size=page, max_rows_per_page=1 << 20)
    return build


def _big_tile(k):
    def build(rng, vrng, flavour):
        ts = T0 + 5 * MIN + np.sort(rng.integers(0, 10 * MIN, ROWS))
        names = _pick(rng, NAMES[:k], ROWS)
        val = _values(vrng, ROWS, flavour)
        if flavour == "nan":
            sub = np.arange(ROWS) // SUB
            val[(names == NAMES[k - 1]) & ((sub == 1) | (sub == 3))] = np.nan
        return ts, names, val, dict(row_group_size=ROWS, data_page_size=1 << 20, max_rows_per_page=1 << 20)
    return build


SHAPES = {f"uniform_{k:02d}": _uniform(k) for k in UNIFORM_K}
SHAPES.update({"growing": _growing, "short_runs": _short_runs, "two_dicts_4k": _two_dicts(4096),
               "two_dicts_1m": _two_dicts(1 << 20), "big_tile_07": _big_tile(7), "big_tile_64": _big_tile(64)})
NAN_SHAPES = ["uniform_07", "uniform_64", "big_tile_07", "big_tile_64"]
# the steps (ms) every file is queried at: the widest tile must lie below two of the smallest
STEPS = {label: (20_000, 60_000, 10 * MIN) for label in SHAPES}
STEPS["short_runs"] = (50_000, 60_000, 10 * MIN)
STEPS.update({label: (10 * MIN,) for label in ("big_tile_07", "big_tile_64")})
STEPS["two_dicts_1m"] = (200_000, 10 * MIN)


# per shape: the seed's last word, chosen once so that the pins of test_clu_shapes_cpu.py hold
SALT = {"short_runs": 3}


def labels():
    """[(shape, flavour)] of every file."""
    return [(s, f) for s in SHAPES for f in ("int", "real")] + [(s, "nan") for s in NAN_SHAPES]


def columns(shape, flavour):
    """(timestamps, names, values, pyarrow write options) of a file: timestamps and names are a function of the shape
    (so a shape's flavours have the same pages and tiles), the values of both labels."""
    si = sorted(SHAPES).index(shape)
    vrng = np.random.default_rng([37, si, ("int", "real", "nan").index(flavour)])
    return SHAPES[shape](np.random.default_rng([31, si, SALT.get(shape, 0)]), vrng, flavour)


class File:
    def __init__(self, dirpath, shape, flavour):
        import pyarrow as pa
        import pyarrow.parquet as pq
        self.shape, self.flavour = shape, flavour
        self.ts, self.names, self.val, opts = columns(shape, flavour)
        self.rows = len(self.ts)
        self.path = os.path.join(str(dirpath), f"clu_{shape}_{flavour}.parquet")
        t = pa.table({TIMESTAMP: pa.array(self.ts, pa.int64()), VALUE: pa.array(self.val, pa.float64()),
                      NAME: pa.array(self.names.tolist(), pa.string())})
        pq.write_table(t, self.path, compression="NONE", use_dictionary=[NAME],
                       column_encoding={TIMESTAMP: "PLAIN", VALUE: "PLAIN"}, **opts)
        with open(self.path, "rb") as f:
            self.blob = f.read()

    def present(self):
        """The file's names in name order."""
        return sorted(set(self.names.tolist()))


def make_files(dirpath, which=None):
    """{(shape, flavour): File} of `which` (default: every file)."""
    return {k: File(dirpath, *k) for k in (labels() if which is None else which)}


def leaf(op, *v):
    return {"k": NAME, "v": list(v), "op": op, "extracted": False, "computed": False, "dataType": "string"}


# ---- stratum (e): name-only filter trees ----
# file sets (shapes) the trees rotate over; every set holds a file of many names, so a tree can pass few rows
TREE_SETS = [["uniform_05", "uniform_33"], ["uniform_33", "growing"], ["growing", "two_dicts_4k", "uniform_05"],
             ["two_dicts_4k", "uniform_33", "uniform_05", "growing"]]
TREE_AGGS = ["sum", "min", "max", "count", "avg"]


def tree(i):
    return ft.random_tree(np.random.default_rng([TREE_SEED, i]), 1 + i % 6, [NAME])


def cut_window(shapes):
    """(ms off the start, ms off the end) of the hour the requests cover, so that the window opens 7 s into the first
    tile and closes 11 s before the end of the shortest file (10 minutes; `growing`: 13), inside a tile of every file."""
    span = min(13 if s == "growing" else 10 for s in shapes)
    return 7_013, ft.HOUR - span * MIN + 11_007


def tree_case(i):
    """Tree i's call: (file set index, flavour, aggregate, groupBys, glob_size, step, cut the window?)."""
    return (i % 4, "int" if (i // 4) % 2 == 0 else "real", TREE_AGGS[i % 5], [NAME] if (i // 2) % 2 else [], 1 + i % 3,
            20_000 if i % 4 == 3 else 60_000, i % 4 == 3)


def _absent(op, *v):
    return {"k": "attr.absent", "v": list(v), "op": op, "extracted": False, "computed": False, "dataType": "string"}


HAND_TREES = [
    ("not in", {"not": leaf("in", "metric_00", "metric_02", "metric_21", "metric_33")}),
    ("ne or regex", {"op": "or", "q1": leaf("!=", "metric_01"), "q2": leaf("regex", "^metric_0[02]$")}),
    ("exists", leaf("exists")),
    ("not exists", {"not": leaf("exists")}),
    ("six leaves", {"op": "or",
                    "q1": {"op": "and", "q1": leaf("contains", "c_0"), "q2": leaf("not_in", "metric_01", "nope")},
                    "q2": {"op": "and", "q1": {"not": leaf("contains", "7")},
                           "q2": {"op": "or", "q1": leaf("not_in", "nope"),
                                  "q2": {"op": "and", "q1": leaf("contains", "_02"), "q2": leaf("eq", "nope")}}}}),
]
# trees over a field no file has (the glob compiles its leaf to `false`: QSeg::leaf_false); see the GPU test's docstring
ABSENT_TREES = [
    ("absent or name", {"op": "or", "q1": _absent("eq", "x"), "q2": leaf("in", "metric_00", "metric_03", "metric_32")}),
    ("(absent or name) and name", {"op": "and", "q1": {"op": "or", "q1": _absent("exists"), "q2": leaf("contains", "_0")},
                                   "q2": leaf("!=", "metric_01")}),
]
