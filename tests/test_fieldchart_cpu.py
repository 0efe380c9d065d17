"""Field charts (chart.fieldName / fieldType), the parts that need no GPU: the text -> double classifier the evaluator
links (lk_field_number, lakeside_amd/csrc/fieldnum.cpp via liblakeside_text.so) and the expectation builder of the GPU
tests (tests/fieldchart_ref.py) on a 12-row table whose cells are written out by hand."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from tests import fieldchart_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")

NUMBERS = ["0", "-0", "7", "-12", "007", "1.5", "-0.25", "3.14159265358979323846", "1e3", "1E3", "2e-3", "6.02E+23",
           "-1.0e-7", "0.1", "123456789012345678901234567890", "1e308", "1.7976931348623157e308", "4.9e-324", "1e-400",
           "9007199254740993", "0.30000000000000004", "5e-324", "2.2250738585072011e-308"]
NULLS = ["abc", "word", "Zebra", "e5", "E", "x1", "hello world", "true", "False", "k", "a.b", "d1e3"]
NEITHER = ["", " 12", "12 ", "\t5", "+5", "inf", "Infinity", "-inf", "nan", "NaN", "-nan", "Inf", "0x10", "1_000", "1e999",
           "-1e999", "12.", ".5", "-", "-.5", "1e", "1e+", "1.5.2", "1,5", "--1", "1-", "5%", "½", "١٢", "$5", "-abc",
           "1.5x", "n/a", "null", "None", "i"]


def _lib():
    L = ctypes.CDLL(LIB)
    L.lk_field_number.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)]
    L.lk_field_number.restype = ctypes.c_int
    return L


def _classify(L, s):
    b = s.encode()
    out = ctypes.c_double(-1.0)
    return L.lk_field_number(b, len(b), ctypes.byref(out)), out.value


def test_classifier_three_classes():
    L = _lib()
    for s in NUMBERS:
        rc, v = _classify(L, s)
        assert rc == 1, s
        assert struct.pack("<d", v) == struct.pack("<d", float(s)), (s, v, float(s))   # bit for bit
        assert fr.text_value(s) == float(s)
    for s in NULLS:
        assert _classify(L, s)[0] == 0, s
        assert fr.text_value(s) is None
    for s in NEITHER:
        assert _classify(L, s)[0] == -1, repr(s)
        with pytest.raises(ValueError):
            fr.text_value(s)
    # the length is honoured (no NUL needed), and out may be NULL
    assert L.lk_field_number(b"12x", 2, None) == 1
    assert L.lk_field_number(b"12\x00", 3, None) == -1


T0 = 1704067200000
SVC = "resource.service.name"


def _table(tmp_path):
    """12 rows in two files of one glob; the second file has no dur$duration column."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    f0 = {dx.TIMESTAMP: [T0 + 1000, T0 + 2000, T0 + 3000, T0 + 61000, T0 + 62000, T0 + 63000, T0 + 64000],
          dx.VALUE: [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
          dx.NAME: ["a", "a", "a", "a", "b", "b", "a"],
          SVC: ["x", "x", "y", "x", "x", "y", "y"],
          "dur$duration": [2_000_000, None, 4_000_000, None, 6_000_000, 1_000_000, None],
          "txt$number": ["1.5", "abc", None, "2e1", "-3", "oops", None]}
    f1 = {dx.TIMESTAMP: [T0 + 5000, T0 + 65000, T0 + 66000, T0 + 125000, T0 + 126000],
          dx.VALUE: [1.0, 1.0, 1.0, 1.0, 1.0],
          dx.NAME: ["a", "b", "b", "a", "a"],
          SVC: ["x", "x", "y", "x", "x"],
          "txt$number": ["10", "0.25", None, "word", "zzz"]}
    paths = []
    for i, cols in enumerate((f0, f1)):
        types = {dx.TIMESTAMP: pa.int64(), dx.VALUE: pa.float64(), "dur$duration": pa.int64()}
        t = pa.table({k: pa.array(v, types.get(k, pa.string())) for k, v in cols.items()})
        paths.append(str(tmp_path / f"hand{i}.parquet"))
        pq.write_table(t, paths[-1])
    return paths


def _req(agg, field, gbs=(SVC,)):
    from lakeside_amd import synth
    segs = [synth.segment_request(i, hour=0) for i in range(2)]
    return json.dumps(synth.pushdown(synth.leaf(synth.NAME, "in", "a", "b"), segs, agg, list(gbs), field=field))


def _rows(rows):
    return sorted((ts, v, tuple(sorted(tags.items()))) for ts, v, tags in rows)


def test_twin_expectation_by_hand(tmp_path):
    paths = _table(tmp_path)
    tag = lambda n, s: (("name", n), (SVC, s))   # noqa: E731
    # dur$duration, sum / 1e6: rows with a NULL field -- and every row of the file without the column -- are not there
    pr, cells, scale = fr.expected_cells(_req("sum", ("dur", "duration")), paths, 2, str(tmp_path / "twin_dur"))
    assert scale == 1e6
    want = [(T0, 2.0, tag("a", "x")), (T0, 4.0, tag("a", "y")),
            (T0 + 60000, 6.0, tag("b", "x")), (T0 + 60000, 1.0, tag("b", "y"))]
    assert _rows(fr.per_glob_rows(pr, cells, scale, "sum")[0]) == sorted(want)
    assert _rows(fr.merged_rows(pr, cells, scale, "sum")) == sorted(want)
    assert _rows(fr.per_glob_rows(pr, cells, scale, "avg")[0]) == sorted(want)   # one value per cell
    # txt$number, max: text that casts to NULL keeps its row (the cell exists, 0.0 when it holds nothing else)
    pr, cells, scale = fr.expected_cells(_req("max", ("txt", "number")), paths, 2, str(tmp_path / "twin_txt"))
    assert scale is None
    want = [(T0, 10.0, tag("a", "x")), (T0 + 60000, 20.0, tag("a", "x")), (T0 + 60000, 0.25, tag("b", "x")),
            (T0 + 60000, 0.0, tag("b", "y")), (T0 + 120000, 0.0, tag("a", "x"))]
    assert _rows(fr.per_glob_rows(pr, cells, scale, "max")[0]) == sorted(want)
    counts = {(ts, tags): v for ts, v, tags in _rows(fr.per_glob_rows(pr, cells, scale, "count")[0])}
    assert counts == {(T0, tag("a", "x")): 2.0, (T0 + 60000, tag("a", "x")): 1.0, (T0 + 60000, tag("b", "x")): 2.0,
                      (T0 + 60000, tag("b", "y")): 0.0, (T0 + 120000, tag("a", "x")): 0.0}
    # a glob none of whose files has the column is empty: glob size 1 puts the second file alone
    pr, cells, scale = fr.expected_cells(_req("sum", ("dur", "duration")), paths, 1, str(tmp_path / "twin_dur1"))
    assert len(cells) == 2 and len(cells[0]) == 4 and cells[1] == []
    assert np.isclose(sum(v for _, v, _ in fr.merged_rows(pr, cells, scale, "sum")), 13.0)
