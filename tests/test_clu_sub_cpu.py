"""The clustered copy's sub-block area without a GPU (liblakeside_text.so only): lk_clu_sub_bytes is clu_sub_bytes and
its offsets of lakeside_amd/csrc/clu.hpp against Python integers, and lk_clu_sub_sim runs clu_sub_class -- the
whole-or-straddling rule scan_clu applies to a split tile's sub-blocks -- against a per-row classification.

Area of one tile (16 sub-blocks of 4,096 rows at most, whatever the tile's rows): [sagg: 16 entries of 32 B per code |
csub: 17 uint32 per code | one uint16 NaN mask per code], padded to 128 B.  The area starts on a 128-B line (hipMalloc
alignment, a stride that is a multiple of 128)."""
import ctypes
import itertools
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
SUB_ROWS, SUB_MAX, AGG_ENTRY, ALIGN = 4096, 16, 32, 128
STRADDLE = 0xFFFFFFFF
NROWS = [1, 4095, 4096, 4097, 65535, 65536]
DICT_N = [1, 16, 63, 64]

_L = None


def _lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(LIB)
        u32, vp = ctypes.c_uint32, ctypes.c_void_p
        L.lk_clu_sub_bytes.argtypes = [u32, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        L.lk_clu_sub_bytes.restype = u32
        L.lk_clu_sub_sim.argtypes = [u32, vp, u32, vp]
        L.lk_clu_sub_sim.restype = u32
        _L = L
    return _L


def area(nrows, dict_n, c=0, j=0):
    o = [ctypes.c_uint32() for _ in range(6)]
    n = _lib().lk_clu_sub_bytes(nrows, dict_n, c, j, *[ctypes.byref(x) for x in o])
    nsub, sub_rows, sub_max, sagg, csub, nan = (x.value for x in o)
    return int(n), nsub, sub_rows, sub_max, sagg, csub, nan


@pytest.mark.parametrize("dict_n", DICT_N)
@pytest.mark.parametrize("nrows", NROWS)
def test_sub_bytes_and_offsets(nrows, dict_n):
    n, nsub, sub_rows, sub_max, _, csub, nan = area(nrows, dict_n)
    assert (sub_rows, sub_max) == (SUB_ROWS, SUB_MAX)
    assert nsub == (nrows + SUB_ROWS - 1) // SUB_ROWS and 1 <= nsub <= SUB_MAX
    assert csub == dict_n * SUB_MAX * AGG_ENTRY
    assert nan == csub + dict_n * (SUB_MAX + 1) * 4
    assert n == (nan + 2 * dict_n + ALIGN - 1) // ALIGN * ALIGN and n % ALIGN == 0
    assert csub % 4 == 0 and nan % 2 == 0
    for c in range(dict_n):
        for j in range(SUB_MAX):
            off = area(nrows, dict_n, c, j)[4]
            assert off == (c * SUB_MAX + j) * AGG_ENTRY
            assert off % AGG_ENTRY == 0 and off + AGG_ENTRY <= csub            # aligned, before csub
            assert off // ALIGN == (off + AGG_ENTRY - 1) // ALIGN              # no entry straddles a 128-B line


def test_dict_n_is_taken_within_1_to_64():
    assert area(100, 0) == area(100, 1)
    assert area(100, 65) == area(100, 64) == area(100, 1 << 20)
    # C2's shape: about 9.3 KB per tile beside a 655 KB block
    assert area(65536, 16)[0] == 9344


def _sim(nrows, sb):
    cls = (ctypes.c_uint32 * SUB_MAX)(*([0xDEAD] * SUB_MAX))
    arr = (ctypes.c_uint32 * 4)(*(list(sb) + [0xFFFFFFFF] * (4 - len(sb))))
    n = _lib().lk_clu_sub_sim(nrows, arr, len(sb), cls)
    assert n == (nrows + SUB_ROWS - 1) // SUB_ROWS
    return [cls[j] for j in range(n)]


def _check(nrows, sb):
    """Brute force: row r's class is the number of boundaries at or below it.  Every whole sub-block's rows all have
    the class the rule returns; a straddling one has rows of more than one class; and the whole sub-blocks' classes
    plus the streamed rows' classes give the per-row class counts."""
    sb = sorted(sb)
    bounds = [0] + [min(b, nrows) for b in sb] + [nrows]                       # class k: rows [bounds[k], bounds[k+1])
    want = [max(0, bounds[k + 1] - bounds[k]) for k in range(len(sb) + 1)]
    assert sum(want) == nrows
    row_class = lambda r: sum(1 for b in sb if b <= r)                         # noqa: E731
    got = [0] * (len(sb) + 1)
    for j, c in enumerate(_sim(nrows, sb)):
        lo, hi = j * SUB_ROWS, min((j + 1) * SUB_ROWS, nrows)
        inside = [b for b in sb if lo < b < hi]
        if c == STRADDLE:
            assert inside, (nrows, sb, j)
            for k in range(len(sb) + 1):                                       # streamed: each row by its own class
                got[k] += max(0, min(hi, bounds[k + 1]) - max(lo, bounds[k]))
        else:
            assert not inside and c == row_class(lo) == row_class(hi - 1), (nrows, sb, j, c)
            got[c] += hi - lo
    assert got == want, (nrows, sb)


@pytest.mark.parametrize("nrows", [1, 4096, 4097, 12288, 65536])
def test_whole_or_straddling_every_placement(nrows):
    places = sorted({r for r in (0, 1, 4095, 4096, 4097, nrows - 1, nrows) if 0 <= r <= nrows})
    for k in (1, 2, 3):
        for sb in itertools.combinations_with_replacement(places, k):          # equal boundaries: an empty class
            _check(nrows, sb)


def test_whole_or_straddling_random():
    rnd = random.Random(20240101)
    for _ in range(2000):
        nrows = rnd.choice([1, 37, 4096, 4097, 12288, 12325, 65535, 65536, rnd.randint(1, 65536)])
        k = rnd.randint(1, 3)
        sb = [rnd.choice([rnd.randint(0, nrows), rnd.randint(0, nrows) // SUB_ROWS * SUB_ROWS]) for _ in range(k)]
        if rnd.random() < 0.2:
            sb[-1] = sb[0]
        _check(nrows, sb)


def test_boundary_on_a_first_row_leaves_the_sub_block_whole():
    assert _sim(12288, [4096]) == [0, 1, 1]
    assert _sim(12288, [4097]) == [0, STRADDLE, 1]
    assert _sim(12288, [4095]) == [STRADDLE, 1, 1]
    assert _sim(12325, [4096, 10000]) == [0, 1, STRADDLE, 2]
    assert _sim(12325, [12325]) == [0, 0, 0, 0]                                # a boundary no row reaches
