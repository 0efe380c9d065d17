"""Exemplar row selection without a GPU (liblakeside_text.so only): lk_ex_select_sim drives the functions of
lakeside_amd/csrc/ex_select.hpp that the evaluator calls between ex_scan HIST passes -- zone-map probe boundaries, the
histogram split that keeps limit == above + need, the candidate-cap closure -- over a CPU histogram, one glob at a
time; numpy says what the emitted range must hold."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
XBINS = 2048                    # kernels.hpp
CAP, PROBE_ROWS = 1 << 24, 1 << 20   # the evaluator's defaults
T0 = 1_700_000_000_000
HOUR = 3_600_000


def _lib():
    L = ctypes.CDLL(LIB)
    i64, u64, vp = ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
    L.lk_ex_select_sim.argtypes = [vp, ctypes.c_size_t, i64, i64, vp, ctypes.c_size_t, u64, ctypes.c_int, u64, u64,
                                   ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(u64),
                                   ctypes.POINTER(ctypes.c_int)]
    L.lk_ex_select_sim.restype = ctypes.c_int
    return L


def sim(ts, win, limit, desc, cap=CAP, tiles=None, probe_rows=PROBE_ROWS):
    ts = np.ascontiguousarray(ts, np.int64)
    tiles = np.ascontiguousarray(tiles if tiles is not None else np.zeros((0, 3)), np.int64)
    elo, ehi, count, passes = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_int()
    rc = _lib().lk_ex_select_sim(ts.ctypes.data, len(ts), win[0], win[1], tiles.ctypes.data, len(tiles), limit,
                                 int(desc), cap, probe_rows, ctypes.byref(elo), ctypes.byref(ehi), ctypes.byref(count),
                                 ctypes.byref(passes))
    assert rc == 0
    return elo.value, ehi.value, count.value, passes.value


def probe_list(tiles, win, desc, probe_rows):
    """The probe boundaries (ex_select.hpp probe_boundaries): tiles from the ordered end, a boundary whenever the rows
    covered reach probe_rows, 8 * probe_rows, ...; boundaries on the window's far edge are no probes."""
    lo, hi = win
    tl = [(-mx if desc else mn, mn if desc else mx, n) for mn, mx, n in tiles.tolist() if not (mx < lo or mn >= hi)]
    tl.sort(key=lambda t: t[0])
    out, rows, goal, edge = [], 0, probe_rows, None
    for _, other, n in tl:
        rows += n
        edge = other if edge is None else min(edge, other) if desc else max(edge, other)
        if rows >= goal:
            b = max(edge, lo) if desc else min(edge + 1, hi)
            if (desc and b > lo) or (not desc and b < hi):
                out.append(b)
            goal *= 8
    return out


def refining_passes(span):
    """ceil(log(span) / log(2048)): each refining pass divides the span by 2048."""
    r = 0
    while XBINS ** r < span:
        r += 1
    return r


def check(ts, win, limit, desc, cap=CAP, tiles=None, probe_rows=PROBE_ROWS):
    """The properties every selection has; returns the passes taken."""
    lo, hi = win
    elo, ehi, count, passes = sim(ts, win, limit, desc, cap, tiles, probe_rows)
    what = (lo, hi, limit, desc, cap, elo, ehi, count, passes)
    inw = np.sort(ts[(ts >= lo) & (ts < hi)])
    n_w = len(inw)
    assert count == int(((ts >= elo) & (ts < ehi)).sum()), what
    if limit == 0:                                  # the evaluator opens no such glob
        assert (count, passes) == (0, 0), what
        return passes
    assert (ehi == hi) if desc else (elo == lo), what
    assert lo <= elo <= ehi <= hi, what
    k = min(limit, n_w)
    if k:
        kth = int(inw[n_w - k] if desc else inw[k - 1])      # the k-th newest (DESC) / oldest (ASC) row
        assert (elo <= kth) if desc else (ehi > kth), what
    if n_w < limit:
        assert (elo, ehi) == (lo, hi), what
    else:
        # closure: the split bin is taken whole iff its surplus cum + h[split] - need stays under the cap, or it is one
        # millisecond wide, when it holds the k-th row's ties and need >= cum + 1; and limit == above + need
        ties = int((inw == kth).sum())
        assert count - limit <= max(cap, ties - 1), what + (ties,)
    nprobes = len(probe_list(tiles, win, desc, probe_rows)) if tiles is not None else 0
    assert 1 <= passes <= nprobes + refining_passes(hi - lo) + 1, what + (nprobes,)
    return passes


def _uniform(rng):
    return T0 + rng.integers(0, HOUR, 20_000), (T0, T0 + HOUR), {}


def _ties(rng):
    return T0 + 100 * rng.integers(0, 200, 20_000), (T0, T0 + HOUR), {"cap": 50}   # a 100 ms grid: ~100 rows per timestamp


def _all_tied(rng):
    return np.full(20_000, T0 + 1_234_567), (T0, T0 + HOUR), {"cap": 50}


def _wide(rng):
    base = (1 << 61) + 987_654_321
    ts = np.concatenate([base + rng.integers(0, 1000, 5_000), [0, (1 << 62) - 1]])
    return ts, (0, 1 << 62), {"cap": 50}


def _edges(rng):
    lo, hi = T0, T0 + HOUR
    inside = lo + rng.integers(0, HOUR, 3_000)
    pins = [lo] * 3 + [hi - 1] * 3 + [lo - 1] * 4 + [hi] * 4 + [lo - HOUR, hi + HOUR]
    return np.concatenate([inside, pins]), (lo, hi), {}


def _tiled(rng, overlap):
    """40 tiles of 1,000 rows, ~10 % of the rows passing the filter; probe boundaries every 3,000 / 24,000 rows."""
    allts = np.sort(T0 + rng.integers(0, HOUR, 40_000))
    if overlap:                                    # neighbouring tiles share a stretch of time, and arrive shuffled
        allts = allts[np.argsort(np.arange(40_000) + rng.integers(0, 2_500, 40_000), kind="stable")]
    rows = allts.reshape(40, 1000)
    tiles = np.stack([rows.min(1), rows.max(1), np.full(40, 1000)], 1)
    if overlap:
        tiles = tiles[rng.permutation(40)]
    return allts[rng.random(40_000) < 0.1], (T0, T0 + HOUR), {"tiles": tiles, "probe_rows": 3000}


CASES = {"uniform": _uniform, "ties_small_cap": _ties, "all_tied": _all_tied, "wide_window": _wide, "edges": _edges,
         "probes_in_order": lambda rng: _tiled(rng, False), "probes_overlapping": lambda rng: _tiled(rng, True)}


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_selection(case, desc):
    ts, win, kw = CASES[case](np.random.default_rng(20250307))
    n = len(ts)
    passes = {limit: check(ts, win, limit, desc, **kw) for limit in (0, 1, 7, 1000, n, n + 5)}
    if case == "ties_small_cap":
        assert passes[1000] >= 2 and passes[7] >= 2          # down to single milliseconds, as the GPU test asserts
    if case == "all_tied":
        assert passes[7] >= 2                                # 20,000 ties exceed the cap until the bin is 1 ms wide
    if case == "wide_window":
        assert passes[7] >= 4                                # 2^62 ms -> one second takes several refining passes
    if case.startswith("probes"):
        # a few hundred passing rows behind the first boundary: enough for 7, too few for 1,000 (a wider range follows)
        tiles, lo, hi = kw["tiles"], win[0], win[1]
        first = probe_list(tiles, win, desc, 3000)[0]
        behind = int(((ts >= first) & (ts < hi)).sum() if desc else ((ts >= lo) & (ts < first)).sum())
        assert 7 <= behind < 1000 and len(probe_list(tiles, win, desc, 3000)) == 2
        assert passes[1000] >= 2
        elo, ehi, _, _ = sim(ts, win, 7, desc, tiles=tiles, probe_rows=3000)
        assert (elo >= first) if desc else (ehi <= first)    # the emit range stayed inside the probed range


def test_small_windows_by_hand():
    """One row per millisecond, 1 ms bins, no surplus allowed: exactly the top `limit`, the split bin included; a window
    without rows, no rows at all, a window of one millisecond."""
    ts = T0 + np.arange(100)
    assert sim(ts, (T0, T0 + 100), 5, True, cap=0) == (T0 + 95, T0 + 100, 5, 1)
    assert sim(ts, (T0, T0 + 100), 5, False, cap=0) == (T0, T0 + 5, 5, 1)
    assert sim(ts, (T0 + 10, T0 + 90), 80, True, cap=0) == (T0 + 10, T0 + 90, 80, 1)
    for desc in (True, False):
        assert sim(ts, (T0 + 1000, T0 + 2000), 5, desc) == (T0 + 1000, T0 + 2000, 0, 1)
        assert sim(np.zeros(0, np.int64), (T0, T0 + HOUR), 5, desc) == (T0, T0 + HOUR, 0, 1)
        assert sim(ts, (T0, T0 + 1), 5, desc) == (T0, T0 + 1, 1, 1)
