"""The row -> bucket rule without a GPU (liblakeside_text.so only): lk_bucket_sim runs bucket_row / bucket_mono of
lakeside_amd/csrc/bucket.hpp -- the functions scan_tiles, scan_lean and ex_scan inline -- and Python integer
arithmetic with explicit truncating division and remainder says what they must return.

fast_div (the 32-bit quotient from the double reciprocal with its one-step correction) is checked against the exact
path over its whole domain, 0 <= ts - base < 2^32, with bases >= 0: for negative timestamps `ts - ts % step` truncates
toward zero, which no quotient of ts - base reproduces, and the evaluator's bases are epoch times."""
import ctypes
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
IN, OUTSIDE, UNALIGNED, RANGE = 0, 1, 2, 3      # bucket.hpp BucketStatus
STEPS = [1, 2, 3, 7, 1000, 10_000, 60_000, 3_600_000, 2**31 - 1]
D_END = 2**32                                   # fast_div's domain: d = ts - base in [0, D_END)
T0 = 1_700_000_000_000


def _lib():
    L = ctypes.CDLL(LIB)
    i64, u64, vp = ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
    L.lk_bucket_sim.argtypes = [vp, ctypes.c_size_t, i64, i64, i64, i64, u64, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    L.lk_bucket_sim.restype = None
    return L


def sim(ts, win, step, base, nbuckets, metrics, fast):
    ts = np.ascontiguousarray(ts, np.int64)
    b, st, mono = np.empty(len(ts), np.int64), np.empty(len(ts), np.uint8), np.empty(len(ts), np.int64)
    _lib().lk_bucket_sim(ts.ctypes.data, len(ts), win[0], win[1], step, base, nbuckets, int(metrics), int(fast),
                         b.ctypes.data, st.ctypes.data, mono.ctypes.data)
    return b, st, mono


def tdiv(a, b):
    """a / b truncated toward zero (C, the JVM), on Python integers."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def trem(a, b):
    return a - b * tdiv(a, b)


def mono(ts, step, base, metrics):
    return tdiv(ts - base, step) if metrics else tdiv((ts - trem(ts, step)) - base, step)


def expect(ts, win, step, base, nbuckets, metrics):
    """(status, bucket); the bucket of a row outside the window is unspecified (None)."""
    if not (win[0] <= ts < win[1]):
        return OUTSIDE, None
    b = mono(ts, step, base, metrics)
    if metrics and trem(ts - base, step) != 0:
        return UNALIGNED, b
    if b < 0 or b >= nbuckets:
        return RANGE, b
    return IN, b


def check(ts, win, step, base, nbuckets, metrics, fast):
    b, st, mn = sim(ts, win, step, base, nbuckets, metrics, fast)
    for i, t in enumerate(ts):
        est, eb = expect(t, win, step, base, nbuckets, metrics)
        where = f"ts={t} step={step} base={base} win={win} nb={nbuckets} metrics={metrics} fast={fast}"
        assert st[i] == est, where
        if est == IN:       # the bucket the caller uses
            assert b[i] == eb, where
        assert mn[i] == mono(t, step, base, metrics), where


def bases(step):
    return [0, step * (T0 // step)]


def edge_ds(step):
    """d = ts - base at k * step - 1, k * step, k * step + 1 for k = 0, 1, a mid value, the largest k with d < 2^32;
    and d = 2^32 - 1."""
    kmax = (D_END - 1) // step
    ks = sorted({0, 1, kmax // 2, kmax})
    ds = {k * step + e for k in ks for e in (-1, 0, 1)}
    ds.add(D_END - 1)
    return sorted(ds)


@pytest.mark.parametrize("step", STEPS)
def test_edges_both_paths(step):
    """Every edge d through the exact path, and through fast_div where d is in its domain; the window holds the whole
    domain, so d = -1 and d = 2^32 show both window edges from outside."""
    nb = (D_END + step - 1) // step
    for base in bases(step):
        win = (base, base + D_END)
        for metrics in (False, True):
            ts = [base + d for d in edge_ds(step) + [D_END]]
            check(ts, win, step, base, nb, metrics, fast=False)
            # outside its domain fast_div's quotient is garbage, but such a row is outside every window the evaluator
            # enables it for: the verdict must still be "outside"
            check(ts, win, step, base, nb, metrics, fast=True)


@pytest.mark.parametrize("step", STEPS)
def test_fast_div_equals_exact_on_random_rows(step):
    """10^5 random d in [0, 2^32) per step: fast_div == exact == Python, metrics and not."""
    rng = random.Random(step)
    base = bases(step)[1]
    ds = [rng.randrange(D_END) for _ in range(50_000)]
    ds += [k * step + rng.choice((0, 0, 1, step - 1)) for k in (rng.randrange((D_END - 1) // step + 1) for _ in range(50_000))]
    ds = [d for d in ds if d < D_END]
    ts = np.array(ds, np.int64) + base
    win = (base, base + D_END)
    nb = (D_END + step - 1) // step
    eq = [d // step for d in ds]                 # d >= 0, ts >= 0: truncation and floor agree
    er = [d % step for d in ds]
    for metrics in (False, True):
        bx, sx, mx = sim(ts, win, step, base, nb, metrics, fast=False)
        bf, sf, mf = sim(ts, win, step, base, nb, metrics, fast=True)
        est = np.array([UNALIGNED if metrics and r else IN for r in er], np.uint8)
        assert np.array_equal(sx, est) and np.array_equal(sf, est)
        assert np.array_equal(bx, np.array(eq, np.int64))
        assert np.array_equal(bf, bx)
        assert np.array_equal(mx, bx) and np.array_equal(mf, bx)


def test_window_edges_lo_inclusive_hi_exclusive():
    step, base = 60_000, 60_000 * (T0 // 60_000)
    win = (base + 90_000, base + 150_000)
    ts = [win[0] - 1, win[0], win[0] + 1, win[1] - 1, win[1], win[1] + 1]
    for fast in (False, True):
        b, st, _ = sim(ts, win, step, base, 10, False, fast)
        assert st.tolist() == [OUTSIDE, IN, IN, IN, OUTSIDE, OUTSIDE]
        assert b[1:4].tolist() == [1, 1, 2]
        check(ts, win, step, base, 10, False, fast)
    # an empty and an inverted window hold no row
    for w in ((base, base), (base + 5, base)):
        assert set(sim(ts + [base], w, step, base, 10, False, False)[1].tolist()) == {OUTSIDE}


@pytest.mark.parametrize("step", [3, 7, 1000, 60_000])
def test_negative_timestamps_truncate_on_the_exact_path(step):
    """ts - ts % step rounds a negative ts toward zero (the JVM's %): buckets left of 0 are one step short."""
    rng = random.Random(step + 1)
    for base in (0, -5 * step, 3 * step):
        ts = [k * step + e for k in (-7, -2, -1, 0, 1, 2) for e in (-1, 0, 1)]
        ts += [rng.randrange(-10 * step, 10 * step) for _ in range(500)]
        win = (-20 * step, 20 * step)
        for metrics in (False, True):
            check(ts, win, step, base, 40, metrics, fast=False)     # b < 0: RANGE, by the same truncation
    assert sim([-1], (-10, 10), 7, 0, 4, False, False)[0][0] == 0     # -1 - (-1 % 7) = 0, not -7
    assert sim([-8], (-10, 10), 7, 0, 4, False, False)[1][0] == RANGE  # -8 - (-1) = -7: bucket -1


@pytest.mark.parametrize("fast", [False, True])
def test_metrics_unaligned_exactly_off_the_grid(fast):
    for step in STEPS:
        base = bases(step)[1]
        ds = [d for d in edge_ds(step) if 0 <= d < D_END]
        b, st, _ = sim([base + d for d in ds], (base, base + D_END), step, base, D_END, True, fast)
        for d, bi, si in zip(ds, b.tolist(), st.tolist()):
            assert si == (UNALIGNED if d % step else IN), (step, d)
            if si == IN:
                assert bi == d // step
    # outside the window nothing is reported unaligned
    assert sim([T0 + 1], (T0 + 2, T0 + 3), 1000, 1000 * (T0 // 1000), 10, True, fast)[1][0] == OUTSIDE


@pytest.mark.parametrize("fast", [False, True])
def test_out_of_range_exactly_outside_the_cell_space(fast):
    for step in STEPS:
        base = bases(step)[1]
        nb = 5 if step > 1 else 2**20
        for metrics in (False, True):
            ds = [k * step for k in (0, 1, nb - 1, nb, nb + 1) if k * step < D_END]
            b, st, _ = sim([base + d for d in ds], (base, base + D_END), step, base, nb, metrics, fast)
            assert st.tolist() == [RANGE if d // step >= nb else IN for d in ds], (step, metrics)
    # b < 0 (a window that starts before the base: the exact path only)
    assert sim([T0 - 1], (T0 - 10, T0 + 10), 1, T0, 10, True, False)[1][0] == RANGE
