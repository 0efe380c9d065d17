"""The two rules the ranks of a distributed numeric groupBy apply to agreed data (lakeside_amd/csrc/numgroup_agree.cpp,
through liblakeside_text.so; the evaluator calls the same functions), without a GPU.

Classes: every subset of {INT32, INT64, FLOAT, DOUBLE, BOOLEAN, VARCHAR, absent} as one glob's files, dealt over 2 and 3
ranks in every way, against the kind rule of numgroup_ref.glob_kinds / dx.numeric_tag_text.
Values: the value sets of numgroup_data.KINDS as canonical keys, split over ranks in every order, against the sorted set
of dx.numeric_tag_text."""
import ctypes
import itertools
import os
import struct

import numpy as np
import pytest

from tests import numgroup_data as nd
from tests import numgroup_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
BOOLEAN, INT32, INT64, FLOAT, DOUBLE, BYTE_ARRAY = 0, 1, 2, 4, 5, 6   # Parquet physical types (parquet.hpp)
# file kind (numgroup_data.KINDS) -> Parquet physical type of its status column (None: no column)
PTYPE = {"D": INT32, "A": INT64, "C": FLOAT, "B": DOUBLE, "E": BOOLEAN, "V": BYTE_ARRAY, "F": None}
ARROW = {"D": "int32", "A": "int64", "C": "float32", "B": "float64", "E": "bool_", "V": "string"}
REFUSED_TEXT, REFUSED_BOOLEAN = 1, 2


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(LIB)
    lib.lk_numgroup_file_class.restype = ctypes.c_int
    lib.lk_numgroup_file_class.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)]
    lib.lk_numgroup_classes_sim.restype = ctypes.c_int
    lib.lk_numgroup_classes_sim.argtypes = [ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    lib.lk_numgroup_values_sim.restype = ctypes.c_long
    lib.lk_numgroup_values_sim.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t]
    return lib


# ---- classes ----

def _rank_bytes(L, kinds):
    """One rank's class bytes: the element-wise max over its files' bytes."""
    out = [0, 0, 0]
    for k in kinds:
        if PTYPE[k] is None:
            continue
        b = (ctypes.c_uint8 * 3)()
        assert L.lk_numgroup_file_class(int(k == "V"), PTYPE[k], b) == 0
        out = [max(x, int(y)) for x, y in zip(out, b)]
    return out


def _union(L, per_rank):
    flat = (ctypes.c_uint8 * (3 * len(per_rank)))(*[b for r in per_rank for b in r])
    ut = ctypes.c_int(99)
    return L.lk_numgroup_classes_sim(flat, len(per_rank), ctypes.byref(ut)), ut.value


def _expected_union(files):
    """(refusal, union type) by the oracle's kind rule over the glob's tables."""
    import pyarrow as pa
    tables = [pa.table({nd.STATUS: pa.array([], getattr(pa, ARROW[k])())} if PTYPE[k] is not None else {"x": pa.array([], pa.int64())})
              for k in files]
    kinds = nr.glob_kinds(tables, nd.STATUS)
    if "text" in kinds and len(kinds) > 1:
        return REFUSED_TEXT, -1
    if "bool" in kinds and len(kinds) > 1:        # (numgroup_ref.write_twins / dx._read_glob raise on both)
        return REFUSED_BOOLEAN, -1
    if not kinds:
        return 0, -1
    if kinds == {"text"}:
        return 0, BYTE_ARRAY
    if kinds == {"bool"}:
        return 0, BOOLEAN
    if "float64" in kinds:
        return 0, DOUBLE
    if "float32" in kinds:
        return 0, FLOAT
    return 0, (INT64 if "A" in files else INT32)   # kinds == {"int"}: INTEGER < BIGINT, printed alike


def test_classes_every_subset_over_two_and_three_ranks(L):
    kinds = list(PTYPE)
    checked = 0
    for n in range(1, len(kinds) + 1):
        for files in itertools.combinations(kinds, n):
            want = _expected_union(files)
            for world in (2, 3):
                seen = set()
                for deal in itertools.product(range(world), repeat=len(files)):   # which rank holds which file
                    per_rank = [_rank_bytes(L, [f for f, r in zip(files, deal) if r == w]) for w in range(world)]
                    got = _union(L, per_rank)
                    assert got == want, (files, deal, got, want)
                    seen.add(got)
                    checked += 1
                assert len(seen) == 1   # the result does not depend on the deal
    assert checked > 5000


def test_classes_text_rule_matches_numeric_tag_text(L):
    """The union type picks the printer: the same value prints as dx.numeric_tag_text prints it under the glob's kinds."""
    from oracle import dataexpr as dx
    kind_of = {"D": "int", "A": "int", "C": "float32", "B": "float64"}
    for files in [("D",), ("D", "A"), ("D", "C"), ("A", "C"), ("D", "B"), ("C", "B"), ("D", "A", "C", "B")]:
        rc, ut = _union(L, [_rank_bytes(L, [f]) for f in files])
        assert rc == 0
        texts, _ = _values(L, [[(ut, _key(ut, 200))]])
        assert texts == [dx.numeric_tag_text({kind_of[f] for f in files}, 200)], files


def test_classes_bad_rank_byte(L):
    assert _union(L, [[0, 0, 5]])[0] == -1


# ---- values ----

def _key(ut, v):
    """The canonical key of value v under union type ut (ex_kernels.hip: tag_key)."""
    if ut == BOOLEAN:
        return int(bool(v))
    if ut in (INT32, INT64):
        return int(v) & (2 ** 64 - 1)
    if ut == FLOAT:
        f = np.float32(v)
        if f != f:
            return 0x7FC00000
        return 0 if f == 0 else struct.unpack("<I", struct.pack("<f", float(f)))[0]
    d = float(v)
    if d != d:
        return 0x7FF8000000000000
    return 0 if d == 0 else struct.unpack("<Q", struct.pack("<d", d))[0]


def _values(L, per_rank):
    """per_rank: lists of (union type, key) -> (texts, ids per rank)."""
    flat = [e for r in per_rank for e in r]
    n = max(1, len(flat))
    uts = (ctypes.c_int32 * n)(*[e[0] for e in flat])
    keys = (ctypes.c_uint64 * n)(*[e[1] for e in flat])
    counts = (ctypes.c_size_t * len(per_rank))(*[len(r) for r in per_rank])
    ids = (ctypes.c_uint32 * n)()
    out = ctypes.create_string_buffer(1 << 16)
    rc = L.lk_numgroup_values_sim(uts, keys, counts, len(per_rank), ids, out, len(out))
    assert rc >= 0, out.value
    texts = out.value.decode().split("\n") if rc else []
    assert len(texts) == rc
    got_ids, at = [], 0
    for r in per_rank:
        got_ids.append([int(ids[at + i]) for i in range(len(r))])
        at += len(r)
    return texts, got_ids


# glob union (kinds of dx.numeric_tag_text, union type) -> the file kinds whose values it reads
UNIONS = [({"int"}, INT64, ["A", "D"]), ({"int"}, INT32, ["D"]), ({"int", "float64"}, DOUBLE, ["A", "B", "D"]),
          ({"int", "float32"}, FLOAT, ["D", "C"]), ({"float32", "float64"}, DOUBLE, ["C", "B"]), ({"bool"}, BOOLEAN, ["E"])]


def _entries():
    """Every (union type, key, expected text) of the KINDS value sets under the unions above."""
    from oracle import dataexpr as dx
    out = []
    for kinds, ut, files in UNIONS:
        for f in files:
            for v in nd.KINDS[f][1]:
                if f == "C":
                    v = float(np.float32(v))
                out.append((ut, _key(ut, v), dx.numeric_tag_text(kinds, v)))
    return out


def test_values_split_over_ranks_in_every_order(L):
    ents = _entries()
    want = sorted({t.encode() for _, _, t in ents})          # byte order, as std::string compares
    want = [t.decode() for t in want]
    assert {"9.007199254740992E15", "1.6777216E7", "NaN", "0.0", "-1", "-9223372036854775808", "200", "200.0", "true"} <= set(want)
    assert "-0.0" not in want                                 # -0.0 groups and prints as 0.0 under both float types
    # 2^24 + 1 (INT32) is 2^24 under FLOAT, itself under DOUBLE
    assert _values(L, [[(FLOAT, _key(FLOAT, 2 ** 24 + 1))], [(DOUBLE, _key(DOUBLE, 2 ** 24 + 1))]])[0] == ["1.6777216E7", "1.6777217E7"]
    # 2^53 + 1 (INT64) and 2^53 (DOUBLE) are one text under DOUBLE, apart under BIGINT
    assert "9007199254740993" in want
    rng = np.random.default_rng(5)
    splits = []
    for world in (1, 2, 3):
        for _ in range(4):
            deal = rng.integers(0, world, len(ents))
            ranks = [[e for e, r in zip(ents, deal) if r == w] for w in range(world)]
            for order in itertools.permutations(range(world)):
                splits.append([ranks[w] for w in order])
    splits.append([ents, ents])                               # every text on both ranks
    splits.append([ents, []])                                 # a rank without a value
    splits.append([list(reversed(ents)), ents[::2]])
    for ranks in splits:
        texts, ids = _values(L, [[(ut, k) for ut, k, _ in r] for r in ranks])
        assert texts == want
        for r, rid in zip(ranks, ids):
            assert [texts[i] for i in rid] == [t for _, _, t in r]   # id = position of the entry's text


def test_same_text_from_two_ranks_is_one_id(L):
    # "200.0": a DOUBLE glob's 200.0 on rank 0, a FLOAT glob's 200 on rank 1, a DOUBLE glob's INT-born 200 on rank 2
    ranks = [[(DOUBLE, _key(DOUBLE, 200.0)), (INT64, _key(INT64, 200))], [(FLOAT, _key(FLOAT, 200))], [(DOUBLE, _key(DOUBLE, 200))]]
    texts, ids = _values(L, ranks)
    assert texts == ["200", "200.0"]
    assert ids == [[1, 0], [1], [1]]
    # the all-ones key: INT64 -1 from one rank only
    texts, ids = _values(L, [[(INT64, _key(INT64, 200))], [(INT64, 2 ** 64 - 1), (INT64, _key(INT64, -2 ** 63))]])
    assert texts == ["-1", "-9223372036854775808", "200"] and ids == [[2], [0, 1]]
    assert _values(L, [[], []]) == ([], [[], []])


def test_values_refuse_a_glob_without_the_column(L):
    uts = (ctypes.c_int32 * 1)(-1)
    keys = (ctypes.c_uint64 * 1)(5)
    counts = (ctypes.c_size_t * 1)(1)
    ids = (ctypes.c_uint32 * 1)()
    out = ctypes.create_string_buffer(256)
    assert L.lk_numgroup_values_sim(uts, keys, counts, 1, ids, out, len(out)) == -4 and b"without the column" in out.value
