"""The clustered value copy's tile rule without a GPU (liblakeside_text.so only): lk_clu_sim runs clu_classify of
lakeside_amd/csrc/clu.hpp -- the function scan_clu inlines per tile -- and Python integer arithmetic with explicit
truncating division says what it must return; lk_clu_segment_taken is the host's whole-segment rule (eval_plan.cpp),
which must imply that every tile meeting a window is pinned or split.

Kinds: 0 outside the window, 1 pinned, 2 split, 3 inside the window but not taken.  A split tile has at most
SPLIT_MAX = 4 class boundaries, that is at most three buckets."""
import ctypes
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
NONE, PINNED, SPLIT, UNTAKEN = 0, 1, 2, 3
SPLIT_MAX = 4
T0 = 1_700_000_000_000
STEP = 60_000


def _lib():
    L = ctypes.CDLL(LIB)
    i64, u64, vp = ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
    L.lk_clu_sim.argtypes = [vp, vp, vp, ctypes.c_size_t, i64, i64, i64, i64, u64, ctypes.c_int, vp, vp, vp]
    L.lk_clu_sim.restype = None
    L.lk_clu_segment_taken.argtypes = [ctypes.c_int, i64, i64]
    L.lk_clu_segment_taken.restype = ctypes.c_int
    return L


def sim(tiles, win, step, base, nbuckets, split_ok=True):
    """tiles: [(ts_min, ts_max, sorted)] -> [(kind, b0, nsb)]"""
    lo = np.ascontiguousarray([t[0] for t in tiles], np.int64)
    hi = np.ascontiguousarray([t[1] for t in tiles], np.int64)
    so = np.ascontiguousarray([1 if t[2] else 0 for t in tiles], np.uint8)
    kind, b0, nsb = np.empty(len(tiles), np.uint8), np.empty(len(tiles), np.int64), np.empty(len(tiles), np.uint32)
    _lib().lk_clu_sim(lo.ctypes.data, hi.ctypes.data, so.ctypes.data, len(tiles), win[0], win[1], step, base, nbuckets,
                      int(split_ok), kind.ctypes.data, b0.ctypes.data, nsb.ctypes.data)
    return [(int(k), int(b), int(n)) for k, b, n in zip(kind, b0, nsb)]


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def trem(a, b):
    return a - tdiv(a, b) * b


def bucket(ts, step, base):
    return tdiv((ts - trem(ts, step)) - base, step)


def want(ts_min, ts_max, sorted_, win, step, base, nbuckets, split_ok=True):
    """The rule in Python integers (lean_kernel.hpp's zone-map pin and split-tile test)."""
    if ts_max < win[0] or ts_min >= win[1]:
        return (NONE, 0, 0)
    if ts_min >= win[0] and ts_max < win[1]:
        b0, b1 = bucket(ts_min, step, base), bucket(ts_max, step, base)
        if b0 == b1 and 0 <= b0 < nbuckets:
            return (PINNED, b0, 0)
    if sorted_ and split_ok:
        lo, hi = max(ts_min, win[0]), min(ts_max, win[1] - 1)
        bl, bh = bucket(lo, step, base), bucket(hi, step, base)
        if lo <= hi and bl >= 0 and bh < nbuckets and bh - bl + 2 <= SPLIT_MAX:
            return (SPLIT, bl, bh - bl + 2)
    return (UNTAKEN, 0, 0)


def check(tiles, win, step, base, nbuckets, split_ok=True):
    got = sim(tiles, win, step, base, nbuckets, split_ok)
    exp = [want(a, b, s, win, step, base, nbuckets, split_ok) for a, b, s in tiles]
    assert got == exp
    return got


WIN = (T0 - T0 % STEP, T0 - T0 % STEP + 60 * STEP)
BASE = WIN[0]


def test_inside_one_bucket():
    b = BASE + 5 * STEP
    got = check([(b, b, True), (b, b + STEP - 1, True), (b + 17, b + 40_000, False), (b + STEP - 1, b + STEP - 1, False)],
                WIN, STEP, BASE, 60)
    assert [g[0] for g in got] == [PINNED] * 4 and [g[1] for g in got] == [5] * 4


def test_touching_a_boundary():
    b = BASE + 5 * STEP
    got = check([(b - 1, b, True),                 # the first timestamp is the last of the bucket before
                 (b, b + STEP, True),              # the last timestamp is the first of the next bucket
                 (b - 1, b + STEP, True),          # both: three buckets
                 (b - 1, b, False)],               # unsorted: nobody can split it
                WIN, STEP, BASE, 60)
    assert got == [(SPLIT, 4, 3), (SPLIT, 5, 3), (SPLIT, 4, 4), (UNTAKEN, 0, 0)]


def test_span_of_two_steps():
    """A range of 2 * step - 1 meets at most three buckets wherever it starts; 2 * step can meet four at no start
    (three full boundaries need 2 * step + 1 timestamps), but the host rule stops below 2 * step."""
    L = _lib()
    assert L.lk_clu_segment_taken(1, 2 * STEP - 1, STEP) == 1
    assert L.lk_clu_segment_taken(1, 2 * STEP, STEP) == 0
    assert L.lk_clu_segment_taken(0, 10, STEP) == 0
    assert L.lk_clu_segment_taken(1, 0, STEP) == 1
    assert L.lk_clu_segment_taken(1, 10, 0) == 0
    for start in (0, 1, STEP - 1, STEP // 2):
        a = BASE + 7 * STEP + start
        got = check([(a, a + 2 * STEP - 1, True), (a, a + 2 * STEP, True), (a, a + 3 * STEP, True)], WIN, STEP, BASE, 60)
        assert got[0][0] == SPLIT and got[0][2] <= SPLIT_MAX
        assert got[2][0] == UNTAKEN   # four or five buckets: too many boundaries


def test_windows_cut_or_miss():
    lo, hi = WIN
    got = check([(lo - 5000, lo + 5000, True),        # cut at the window's start
                 (hi - 5000, hi + 5000, True),        # ... at its end
                 (lo - 5000, lo - 1, True),           # misses: before
                 (hi, hi + 5000, True),               # misses: at / after the end
                 (lo - 5000, lo, True),               # only its last timestamp inside
                 (hi - 1, hi + 9, True),              # only its first timestamp inside
                 (lo - 5000, lo + 5000, False)],      # cut and unsorted: not taken
                WIN, STEP, BASE, 60)
    assert [g[0] for g in got] == [SPLIT, SPLIT, NONE, NONE, SPLIT, SPLIT, UNTAKEN]
    assert got[0] == (SPLIT, 0, 2) and got[1] == (SPLIT, 59, 2)
    # a window narrower than the bucket space (per-glob windows inside the call's space)
    win = (lo + 90_000, hi - 90_000)
    check([(lo, lo + 89_999, True), (lo + 60_000, lo + 100_000, True), (hi - 100_000, hi - 1, True)], win, STEP, BASE, 60)


def test_negative_base_offset_and_overflow():
    # a base above the window's first bucket: those buckets are negative and no rule takes them
    got = check([(WIN[0] + 10, WIN[0] + 20, True), (WIN[0] + 10, WIN[0] + STEP + 20, True),
                 (WIN[0] + 2 * STEP, WIN[0] + 2 * STEP + 5, True)], WIN, STEP, BASE + 2 * STEP, 60)
    assert [g[0] for g in got] == [UNTAKEN, UNTAKEN, PINNED] and got[2][1] == 0
    # buckets at or beyond nbuckets
    got = check([(BASE + 9 * STEP, BASE + 9 * STEP + 5, True), (BASE + 10 * STEP, BASE + 10 * STEP + 5, True),
                 (BASE + 9 * STEP + 5, BASE + 10 * STEP + 5, True)], WIN, STEP, BASE, 10)
    assert [g[0] for g in got] == [PINNED, UNTAKEN, UNTAKEN]


def test_split_off():
    b = BASE + 5 * STEP
    got = check([(b - 1, b, True), (b, b + 1, True)], WIN, STEP, BASE, 60, split_ok=False)
    assert [g[0] for g in got] == [UNTAKEN, PINNED]


@pytest.mark.parametrize("step", [1, 7, 1000, 10_000, 60_000, 3_600_000])
def test_random_against_python(step):
    rng = random.Random(step)
    lo = T0 - T0 % step
    for _ in range(40):
        nb = rng.randint(1, 50)
        win = (lo + rng.randint(0, step), lo + nb * step - rng.randint(0, step - 1) if nb > 1 else lo + step)
        if win[0] >= win[1]:
            continue
        base = lo + rng.choice([0, 0, 0, step, -step])
        tiles = []
        for _ in range(200):
            a = lo + rng.randint(-2 * step, (nb + 2) * step)
            tiles.append((a, a + rng.choice([0, 1, step - 1, step, 2 * step - 1, 2 * step, rng.randint(0, 4 * step)]),
                          rng.random() < 0.8))
        check(tiles, win, step, base, nb)


@pytest.mark.parametrize("step", [1, 2, 7, 10_000, 60_000])
def test_host_rule_implies_taken(step):
    """Whatever the host accepts (every tile sorted with a copy, widest range < 2 * step), scan_clu takes: every tile
    that meets a glob window lying inside the call's bucket space is pinned or split."""
    rng = random.Random(1000 + step)
    L = _lib()
    for _ in range(60):
        nb = rng.randint(1, 40)
        base = T0 - T0 % step + rng.randint(0, 5) * step
        space_hi = base + nb * step
        wl = rng.randint(base, space_hi - 1)
        win = (wl, rng.randint(wl + 1, space_hi))
        widest = rng.randint(0, 2 * step - 1)
        assert L.lk_clu_segment_taken(1, widest, step) == 1
        tiles = []
        for _ in range(300):
            a = rng.randint(base - 3 * step, space_hi + 3 * step)
            tiles.append((a, a + rng.choice([0, widest, rng.randint(0, widest)]), True))
        got = check(tiles, win, step, base, nb)
        assert all(g[0] in (NONE, PINNED, SPLIT) for g in got)
        for (a, b, _), g in zip(tiles, got):
            assert (g[0] == NONE) == (b < win[0] or a >= win[1])
