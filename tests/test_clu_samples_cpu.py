"""The clustered copy's timestamp sample table without a GPU (liblakeside_text.so only): lk_clu_samples_sim returns a
tile's table as clu_build lays it out -- entry s is the timestamp of row (s * nrows) >> 8, s = 0 .. 255, the rows
scan_clu's boundary search samples (clu.hpp, clu_samp_row) -- and lk_clu_samp_layout the place of tile t's table in
the segment's area of tables: 2,048 B each, one behind the other, so every table starts on a 128-B line (16 lines)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
NROWS = [1, 2, 255, 256, 257, 4095, 4096, 4097, 65535, 65536]
NSAMP, SAMP_BYTES, ALIGN = 256, 2048, 128

_L = None


def _lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(LIB)
        u32, vp = ctypes.c_uint32, ctypes.c_void_p
        L.lk_clu_samples_sim.argtypes = [vp, u32, vp]
        L.lk_clu_samples_sim.restype = ctypes.c_int
        L.lk_clu_samp_layout.argtypes = [u32, vp]
        L.lk_clu_samp_layout.restype = ctypes.c_uint64
        L.lk_clu_sub_bytes.argtypes = [u32, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        L.lk_clu_sub_bytes.restype = u32
        _L = L
    return _L


def samples(ts):
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    out = np.full(NSAMP, -12345, dtype=np.int64)
    n = _lib().lk_clu_samples_sim(ts.ctypes.data, len(ts), out.ctypes.data)
    return n, out


@pytest.mark.parametrize("nrows", NROWS)
def test_table_is_the_sampled_rows(nrows):
    rng = np.random.default_rng(nrows)
    ts = 1_700_000_000_000 + np.sort(rng.integers(0, 120_000, nrows))
    n, got = samples(ts)
    assert n == NSAMP
    rows = (np.arange(NSAMP, dtype=np.uint64) * np.uint64(nrows)) >> np.uint64(8)
    assert rows[0] == 0 and rows[-1] == (255 * nrows) >> 8 < nrows
    assert got.tolist() == ts[rows.astype(np.int64)].tolist()
    assert np.all(np.diff(got) >= 0)                      # sorted timestamps: a sorted table
    if nrows < NSAMP:                                     # fewer rows than samples: rows repeat, every row is sampled
        assert len(set(rows.tolist())) == nrows
        counts = np.bincount(rows.astype(np.int64), minlength=nrows)
        assert counts.min() >= NSAMP // nrows and counts.max() <= -(-NSAMP // nrows)
    else:
        assert len(set(rows.tolist())) == NSAMP


def test_values_are_copied_bit_for_bit():
    ts = np.array([np.iinfo(np.int64).min, -1, 0, 1, np.iinfo(np.int64).max], dtype=np.int64)
    n, got = samples(ts)
    assert n == NSAMP
    assert got.tolist() == [int(ts[(s * 5) >> 8]) for s in range(NSAMP)]


def test_bad_row_counts_are_refused():
    ts = np.zeros(4, dtype=np.int64)
    out = np.zeros(NSAMP, dtype=np.int64)
    assert _lib().lk_clu_samples_sim(ts.ctypes.data, 0, out.ctypes.data) == -1
    assert _lib().lk_clu_samples_sim(ts.ctypes.data, 65537, out.ctypes.data) == -1


def test_layout_of_the_tables():
    L = _lib()
    nb = ctypes.c_uint32()
    for t in (0, 1, 17, 17897, (1 << 21) - 1):
        off = L.lk_clu_samp_layout(t, ctypes.byref(nb))
        assert nb.value == SAMP_BYTES == NSAMP * 8
        assert off == t * SAMP_BYTES and off % ALIGN == 0     # every table starts on a 128-B line: 16 lines
    # the sub-block area that follows the tables in their allocation keeps its size and its alignment
    assert L.lk_clu_sub_bytes(65536, 16, 0, 0, None, None, None, None, None, None) == 9344
