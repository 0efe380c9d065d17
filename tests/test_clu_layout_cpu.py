"""The clustered value copy's tile block layout without a GPU (liblakeside_text.so only): lk_clu_block_bytes is
clu_block_bytes of lakeside_amd/csrc/clu.hpp -- the one function Engine::build_cluster sizes a block with and clu_build
and scan_clu take their offsets from -- against Python integers.

Block: [65 uint32 prefix counts, the 64-bit NaN mask at byte 264 | cagg at 288: dict_n entries of 32 B | cvals: nrows
x 8 B | crows: nrows x 2 B], padded to 128 B (blocks start on an HBM line, and the copy area's first block follows the
128-B-aligned descriptor array).  The engine's `clu_bytes` as the sum over a known segment's tiles needs a device:
tests/test_gpu_clu_agg.py, test_engine_clu_bytes_is_the_sum_over_tiles."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
PREF, NAN_OFF, AGG_OFF, AGG_ENTRY, ALIGN = 272, 264, 288, 32, 128
NROWS = [1, 63, 64, 65, 65536]
DICT_N = [1, 16, 63, 64]


def block(nrows, dict_n):
    L = ctypes.CDLL(LIB)
    L.lk_clu_block_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.lk_clu_block_bytes.restype = ctypes.c_uint64
    a, v, r = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    n = L.lk_clu_block_bytes(nrows, dict_n, ctypes.byref(a), ctypes.byref(v), ctypes.byref(r))
    return int(n), a.value, v.value, r.value


@pytest.mark.parametrize("dict_n", DICT_N)
@pytest.mark.parametrize("nrows", NROWS)
def test_block_bytes(nrows, dict_n):
    n, agg, vals, rows = block(nrows, dict_n)
    assert agg == AGG_OFF
    assert vals == AGG_OFF + AGG_ENTRY * dict_n
    assert rows == vals + 8 * nrows
    assert n == (rows + 2 * nrows + ALIGN - 1) // ALIGN * ALIGN
    assert n - ALIGN < rows + 2 * nrows <= n


@pytest.mark.parametrize("dict_n", DICT_N)
@pytest.mark.parametrize("nrows", NROWS)
def test_alignment(nrows, dict_n):
    """Blocks are multiples of 128 B from a 128-B-aligned start, so within a block: cvals on 16 B, every cagg entry
    inside one 128-B line (32-B aligned) and behind the prefix counts and the NaN mask, crows on 2 B."""
    n, agg, vals, rows = block(nrows, dict_n)
    assert n % ALIGN == 0 and vals % 16 == 0 and rows % 2 == 0
    assert 65 * 4 <= NAN_OFF and NAN_OFF % 8 == 0 and NAN_OFF + 8 <= PREF <= agg
    for c in range(dict_n):
        assert (agg + AGG_ENTRY * c) % AGG_ENTRY == 0
        assert (agg + AGG_ENTRY * c) // ALIGN == (agg + AGG_ENTRY * (c + 1) - 1) // ALIGN


def test_dict_n_is_taken_within_1_to_64():
    assert block(100, 0) == block(100, 1)
    assert block(100, 65) == block(100, 64) == block(100, 1 << 20)
