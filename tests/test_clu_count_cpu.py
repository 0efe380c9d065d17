"""COUNT over a split tile of the clustered copy without a GPU (liblakeside_text.so only): lk_clu_count_sim runs
clu_count_split of lakeside_amd/csrc/clu.hpp -- the arithmetic scan_clu<AGG_COUNT> mirrors -- for one code of one
tile, and numpy says what it must return: np.bincount of each element's class, the class of a row being the number
of boundary rows at or below it.

With the sub-block area a whole 4,096-row sub-block (clu_sub_class) adds the difference of two csub entries to its
class without looking at a row; only the elements of a sub-block that holds a boundary strictly inside are classed
one by one.  Without it every element is.  Both must give numpy's counts, and so each other's."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
SUB = 4096
NCLS = 5
NROWS = [1, 63, 64, 4095, 4096, 4097, 20011, 65535, 65536]

_L = None


def _lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(LIB)
        u32, vp = ctypes.c_uint32, ctypes.c_void_p
        L.lk_clu_count_sim.argtypes = [u32, vp, u32, vp, u32, ctypes.c_int, vp]
        L.lk_clu_count_sim.restype = ctypes.c_int
        _L = L
    return _L


def _sim(nrows, rows, sb, use_sub):
    rows = np.ascontiguousarray(rows, np.uint16)
    b = np.ascontiguousarray(sb, np.uint32)
    cnt = np.full(NCLS, 0xDEAD, np.uint32)
    assert _lib().lk_clu_count_sim(nrows, rows.ctypes.data, len(rows), b.ctypes.data, len(b), 1 if use_sub else 0,
                                   cnt.ctypes.data) == NCLS
    return cnt.tolist()


def _want(rows, sb):
    cls = np.searchsorted(np.asarray(sb, np.int64), np.asarray(rows, np.int64), side="right")
    return np.bincount(cls, minlength=NCLS).tolist()


def _patterns(nrows):
    """The rows of one code: dense, every 16th, a single element (first row, last row, the middle), none."""
    return {"dense": np.arange(nrows), "every16": np.arange(3 % nrows, nrows, 16), "first": np.array([0]),
            "last": np.array([nrows - 1]), "middle": np.array([nrows // 2]), "none": np.array([], np.int64)}


def _candidates(nrows):
    """Boundary rows: row 0, the first row of a sub-block, rows strictly inside one (two per sub-block, so that a pair
    lies inside the same one), a sub-block's last row, and nrows (a class with no row)."""
    last_sub = (nrows - 1) // SUB * SUB
    c = {0, nrows, nrows - 1, nrows // 2, nrows // 2 + 1}
    for base in {0, SUB, last_sub}:
        for r in (base, base + 7, base + 9, base + SUB - 1):
            if r <= nrows:
                c.add(r)
    return sorted(c)


def _boundary_sets(nrows):
    cand = _candidates(nrows)
    rng = random.Random(nrows)
    out = []
    for nsb in (2, 3, 4):
        combos = list(itertools.combinations_with_replacement(cand, nsb))   # ascending, equal boundaries included
        if len(combos) > 160:
            combos = rng.sample(combos, 160)
        out += combos
    return out


@pytest.mark.parametrize("nrows", NROWS)
def test_counts_are_numpys(nrows):
    pats = _patterns(nrows)
    for sb in _boundary_sets(nrows):
        for name, rows in pats.items():
            want = _want(rows, sb)
            assert sum(want) == len(rows)
            whole = _sim(nrows, rows, sb, False)
            area = _sim(nrows, rows, sb, True)
            assert whole == want, (nrows, sb, name, "streamed whole")
            assert area == want, (nrows, sb, name, "sub-block area")
            assert area == whole


@pytest.mark.parametrize("nrows", [4097, 20011, 65536])
def test_named_boundaries(nrows):
    """The cases by name, whatever the sampling above drew: a boundary at row 0, on the first row of a sub-block,
    strictly inside one, on its last row, at nrows; two equal boundaries (an empty class); two inside one sub-block."""
    inside = SUB + 100 if nrows > SUB + 101 else SUB // 2
    sets = [(0, nrows), (SUB, nrows), (inside, nrows), (SUB - 1, nrows), (0, SUB - 1, SUB, nrows), (inside, inside, nrows),
            (inside - 50, inside, nrows), (0, 0), (nrows, nrows, nrows, nrows), (0, inside - 50, inside, nrows),
            (SUB, SUB, SUB), (SUB - 1, SUB), (nrows - 1, nrows)]
    for sb in sets:
        for name, rows in _patterns(nrows).items():
            want = _want(rows, sb)
            assert _sim(nrows, rows, sb, True) == want, (nrows, sb, name)
            assert _sim(nrows, rows, sb, False) == want, (nrows, sb, name)
    # two equal boundaries leave the class between them empty, a boundary at nrows the class after it
    dense = np.arange(nrows)
    assert _sim(nrows, dense, (inside, inside, nrows), True) == [inside, 0, nrows - inside, 0, 0]
    assert _sim(nrows, dense, (0, SUB), True) == [0, SUB, nrows - SUB, 0, 0]


def test_random_codes():
    """Random subsets of a tile's rows (a code among others) against random ascending boundaries."""
    rng = np.random.default_rng(20261)
    for _ in range(300):
        nrows = int(rng.choice(NROWS[3:]))
        rows = np.flatnonzero(rng.random(nrows) < rng.choice([0.001, 1 / 16, 0.5]))
        nsb = int(rng.integers(2, 5))
        if rng.random() < 0.5:   # near sub-block edges
            sb = np.sort(np.clip(rng.integers(0, nrows // SUB + 1, nsb) * SUB + rng.integers(-2, 3, nsb), 0, nrows))
        else:
            sb = np.sort(rng.integers(0, nrows + 1, nsb))
        want = _want(rows, sb)
        assert _sim(nrows, rows, sb, True) == want, (nrows, sb.tolist())
        assert _sim(nrows, rows, sb, False) == want, (nrows, sb.tolist())


def test_arguments_outside_the_bounds():
    rows = np.array([3, 2], np.uint16)   # not ascending
    cnt = np.zeros(NCLS, np.uint32)
    sb = np.array([1, 2], np.uint32)
    L = _lib()
    assert L.lk_clu_count_sim(10, rows.ctypes.data, 2, sb.ctypes.data, 2, 1, cnt.ctypes.data) == -1
    assert L.lk_clu_count_sim(0, rows.ctypes.data, 0, sb.ctypes.data, 2, 1, cnt.ctypes.data) == -1
    assert L.lk_clu_count_sim(65537, rows.ctypes.data, 0, sb.ctypes.data, 2, 1, cnt.ctypes.data) == -1
    assert L.lk_clu_count_sim(10, rows.ctypes.data, 0, sb.ctypes.data, 5, 1, cnt.ctypes.data) == -1
