"""Tag-name queries (isTagQuery without a tagDataType) on the CPU: the restatement (tests/tagnames_ref.py) against a literal
run of the worker's steps, the engine's gate and row fold through liblakeside_text.so, and a census of the probe data.

`oracle/sqlplan.run_sql` does not take the shape (it builds a chart's SELECT from chart.groupBys / aggregation and this
request has no chart), so the literal run here builds the reference's text itself -- `SELECT * FROM (SELECT * FROM t WHERE
<window>) WHERE <filter>` from sqlplan's timestamp_filter / filter_sql -- and runs it on SQLite over sqlplan's glob table.
SQLite decides which rows pass and in which order (rowid order: the insertion order stand-in); a row's cells are then read
from the Parquet tables, because SQLite stores a NaN as NULL and a BOOLEAN as 0 / 1.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from lakeside_amd import synth
from oracle import dataexpr as dx
from oracle import exemplar as ex
from oracle import sqlplan
from tests import tagnames_data as td
from tests import tagnames_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "tag queries without a tagDataType: "
UNSUPPORTED = -2


@pytest.fixture(scope="module")
def text_lib():
    L = ctypes.CDLL(os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so"))
    L.lk_tagnames_gate_sim.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.lk_tagnames_gate_sim.restype = ctypes.c_int
    L.lk_tagnames_rows_sim.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    L.lk_tagnames_rows_sim.restype = ctypes.c_long
    return L


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tagnames_cpu")
    return {fl: td.write_files(d, fl) for fl in ("double", "int")}


@pytest.fixture(scope="module")
def ref_rows(files):
    """The restatement's rows per (flavour, filter), computed once."""
    out = {}
    for fl, (paths, blobs) in files.items():
        for name, filt in td.FILTERS.items():
            pr = dx.parse_pushdown(json.dumps(td.request(filt)))
            out[fl, name] = ref.evaluate(pr, paths, td.GLOB_SIZE, sources=blobs)
    return out


def _literal(pr, paths, glob_size):
    """SELECT * on SQLite, then Commons.toDataPoint (branch T) and TagNameCompressionStage.eval, row by row."""
    import pyarrow.parquet as pq
    seen = set()                                   # TagNameCompressionStage.seenTags, one per call
    emitted = []
    for gi, g in enumerate(dx.globs_of(pr, glob_size)):
        gpaths = [paths[i] for i in g]
        segs = [pr.segmentRequests[i] for i in g]
        con, union = sqlplan._load_glob(gpaths)
        nonexistent = dx.field_set(pr.baseExpr) - set(union)
        window = sqlplan.timestamp_filter(min(s.startTs for s in segs), max(s.endTs for s in segs))
        sql = (f"SELECT rowid, * FROM (SELECT rowid, * FROM t WHERE {window}) "
               f"WHERE {sqlplan.filter_sql(pr.baseExpr.filter, nonexistent)}")
        rowids = [r[0] for r in con.execute(sql).fetchall()]
        con.close()
        assert rowids == sorted(rowids)            # SQLite scans in rowid order: the insertion-order stand-in
        tables = [pq.read_table(p) for p in gpaths]
        lists = [{c: t.column(c).to_pylist() for c in t.column_names} for t in tables]
        offs = np.cumsum([0] + [t.num_rows for t in tables])
        types = {}
        for t in tables:
            for f in t.schema:
                types[f.name] = ex.union_type(types.get(f.name), ex._kind(f.type))
        assert union[0] == dx.TIMESTAMP
        for rid in rowids:
            f = int(np.searchsorted(offs, rid - 1, side="right") - 1)
            r = rid - 1 - int(offs[f])
            tb = tables[f]
            cells = [lists[f][c][r] if c in lists[f] else None for c in union]
            timestamp = int(cells[0])                                  # getLong(1)
            value = 0.0 if cells[1] is None else float(cells[1])       # getDouble(2)
            tags = {}
            for c, x in zip(union[2:], cells[2:]):
                s = None if x is None else ex._text(x, ex._kind(tb.schema.field(c).type), types[c])   # getString
                if s is not None and s != "null" and s != "":
                    tags[c] = s
            remove = [t for t in list(tags) if (t in seen or seen.add(t)) or tags[t] is None or tags[t] == ""]
            for t in remove:
                del tags[t]
            if tags:
                emitted.append((timestamp, value, tags, gi, (gi, f, r)))
    emitted.sort(key=lambda x: x[4])
    emitted.sort(key=lambda x: x[0], reverse=pr.reverseSort)
    return emitted


@pytest.mark.parametrize("flavour", ["double", "int"])
def test_restatement_matches_literal_run(files, ref_rows, flavour):
    paths, _ = files[flavour]
    for name, filt in td.FILTERS.items():
        pr = dx.parse_pushdown(json.dumps(td.request(filt)))
        want = _literal(pr, paths, td.GLOB_SIZE)
        got = ref_rows[flavour, name]
        assert len(got) == len(want), (flavour, name)
        for g, w in zip(got, want):
            assert g[0] == w[0] and g[2] == w[2] and g[3] == w[3] and g[4] == w[4], (flavour, name, g, w)
            assert np.float64(g[1]).tobytes() == np.float64(w[1]).tobytes(), (flavour, name, g, w)
    # reverseSort and the merged glob column
    pr = dx.parse_pushdown(json.dumps(td.request(td.FILTERS["keep"], reverse=True)))
    want = _literal(pr, paths, td.GLOB_SIZE)
    got = ref.evaluate(pr, paths, td.GLOB_SIZE, per_glob=False)
    assert [(g[0], g[2], g[4]) for g in got] == [(w[0], w[2], w[4]) for w in want]
    assert all(g[3] == 0 for g in got) and [g[0] for g in got] == sorted((g[0] for g in got), reverse=True)


def test_census_of_probe_cases(ref_rows):
    """Every probe case occurs in the data and, under the reference, lands where its column's name says."""
    for fl in ("double", "int"):
        rows = ref_rows[fl, "pass_all"]
        at = {k: r[4] for r in rows for k in r[2]}
        text = {k: r[2][k] for r in rows for k in r[2]}
        by_row = {r[4]: r for r in rows}
        for r0 in td.FROM_ROWS:                                   # rows 0, 63, 64, 255, 256, 299 of the first tile; 300: the next
            assert at[f"p.row{r0}"] == (0, 0, r0)
        assert at["only.second"] == (0, 1, 0) and at["appended.col"] == (0, 1, 3)
        assert at["only.glob2"] == (1, 0, 5)
        assert at["fail.only"] == (0, 0, 0)
        for absent in ("all.null", "all.empty", "all.nulltext", "mix.nothing"):
            assert absent not in at
        assert at["late.real"] == (0, 0, 100) and text["late.real"] == "real"
        assert at["plain.nulls"] == (0, 0, 41) and at["plain.full"] == (0, 0, 0) and at["dict.nulls"] == (0, 0, 3)
        for c, r0 in td.NUM_FROM.items():
            assert at[c] == (0, 0, r0), c
        assert text["n.f64"] == "NaN" and text["n.i32"] == str(td.NUM_FROM["n.i32"] - 400) and text["n.bool"] == "false"
        assert text["n.f32"] == ex.java_float_text(float(np.float32(td.NUM_FROM["n.f32"] * 0.1)))
        assert at["twin.a"] == at["twin.b"] == (0, 0, 200) and set(by_row[0, 0, 200][2]) >= {"twin.a", "twin.b"}
        assert at["tie.a"] == (0, 0, 120) and at["tie.b"] == (0, 1, 120)
        assert by_row[0, 0, 120][0] == by_row[0, 1, 120][0]       # tied timestamps, file order kept
        i = [r[4] for r in rows]
        assert i.index((0, 0, 120)) + 1 == i.index((0, 1, 120))
        assert by_row[0, 0, 64][1] == 0.0                          # NULL value column on an emitted row
        assert td.TS not in at and td.VALUE not in at
        assert not any(r[4][2] % 50 == 7 for r in rows)            # timestamps outside the window never emit
        # the keep filter: rows i % 3 == 0 fail, i % 7 == 0 are UNKNOWN
        keep = {k: r[4] for r in ref_rows[fl, "keep"] for k in r[2]}
        assert "fail.only" not in keep and td.KEEP in keep
        assert keep["p.row0"] == (0, 0, 1) and keep["p.row63"] == (0, 0, 64) and keep["p.row64"] == (0, 0, 64)
        assert keep["p.row255"] == (0, 0, 256) and keep["p.row256"] == (0, 0, 256) and keep["p.row299"] == (0, 0, 299)
        assert keep["p.row300"] == (0, 0, 302)
        by_keep = {r[4]: r for r in ref_rows[fl, "keep"]}
        assert by_keep[0, 0, 1][1] == 0.0 and by_keep[0, 0, 64][1] == 0.0
        assert ref_rows[fl, "pass_none"] == [] and ref_rows[fl, "nonexistent"] == []
        assert {r[4][2] for r in ref_rows[fl, "numeric_gt"]} and all(r[4][2] >= 450 for r in ref_rows[fl, "numeric_gt"])
        assert ref_rows[fl, "regex"] == ref_rows[fl, "keep"]
    vals = {fl: [r[1] for r in ref_rows[fl, "pass_all"]] for fl in ("double", "int")}
    assert any(v != int(v) for v in vals["double"]) and all(v == int(v) for v in vals["int"])


def _gate(L, req, schemas, dist=0):
    out = ctypes.create_string_buffer(1 << 16)
    rc = L.lk_tagnames_gate_sim(json.dumps(req).encode(), json.dumps(schemas).encode(), dist, out, len(out))
    return rc, out.value.decode()


def test_gate_refusals(text_lib):
    T, I64, F64, BA, BOOL, I32 = td.TS, 2, 5, 6, 0, 1
    good = [[[[T, I64], ["v", F64], ["a", BA]], [[T, I64], ["v", F64], ["b", BA], ["a", BA]]],
            [[[T, I64], ["w", I32]]]]
    keep = td.FILTERS["keep"]
    rc, out = _gate(text_lib, td.request(keep), good)
    assert rc == 0 and json.loads(out) == {"unions": [[T, "v", "a", "b"], [T, "w"]]}
    refusals = [
        (td.request(keep, processor=False), good, 0, "processor.tagNameCompressionEnabled"),
        (td.request(keep, extra={"processor": {"tagNameCompressionEnabled": False}}), good, 0,
         "processor.tagNameCompressionEnabled"),
        (td.request(keep, extra={"processor": {"tagNameCompressionEnabled": True, "resetValueToField": "a"}}), good, 0,
         "processor.resetValueToField"),
        (td.request(keep, base_extra={"extract": {"x": 1}}), good, 0, "extract / compute are not on the hot path"),
        (td.request(keep, base_extra={"compute": {"x": 1}}), good, 0, "extract / compute are not on the hot path"),
        (td.request(keep), [[[["a", BA], [T, I64], ["v", F64]]]], 0, "the first column of glob 0 is a"),
        (td.request(keep), good[:1] + [[[[T, I64], ["s", BA]]]], 0, "the second column s of glob 1"),
        (td.request(keep), [[[[T, I64], ["b", BOOL]]]], 0, "the second column b of glob 0"),
        (td.request(keep), [[[[T, I64], ["v", F64]], [[T, I64], ["v", I64]]]], 0, "different numeric types"),
        (td.request(keep), good, 1, "lk_eval_pushdown_dist"),
    ]
    for req, schemas, dist, why in refusals:
        rc, out = _gate(text_lib, req, schemas, dist)
        assert rc == UNSUPPORTED and out.startswith(PREFIX) and why in out, (why, rc, out)


def _rows_sequential(first):
    """The sequential emulation: walk the keys in ascending order as the rows arrive; a row is emitted when a column's
    first key is that row, with every such column."""
    rows, row_of = [], {}
    for key in sorted(set(k for k in first if k != 2**64 - 1)):
        cols = [c for c, k in enumerate(first) if k == key]
        for c in cols:
            row_of[c] = len(rows)
        rows.append(key)
    return rows, row_of


def test_rows_fold_against_sequential_emulation(text_lib):
    rng = np.random.default_rng(20240607)
    none = 2**64 - 1
    for _ in range(2000):
        n = int(rng.integers(0, 24))
        pool = [int(x) for x in rng.integers(0, 2**63, max(1, int(rng.integers(1, 8))), dtype=np.int64)]
        pool += [(int(rng.integers(0, 4)) << 48) | (int(rng.integers(0, 3)) << 16) | int(rng.integers(0, 300))]
        first = [none if rng.random() < 0.3 else pool[int(rng.integers(0, len(pool)))] for _ in range(n)]   # ties, absent
        arr = (ctypes.c_uint64 * max(1, n))(*first)
        keys = (ctypes.c_uint64 * max(1, n))()
        row_of = (ctypes.c_uint32 * max(1, n))()
        got = text_lib.lk_tagnames_rows_sim(arr, n, keys, row_of, max(1, n))
        want_rows, want_of = _rows_sequential(first)
        assert got == len(want_rows) and list(keys[:got]) == want_rows
        for c in range(n):
            assert row_of[c] == want_of.get(c, 0xffffffff)
    one = (ctypes.c_uint64 * 2)(5, 9)
    assert text_lib.lk_tagnames_rows_sim(one, 2, (ctypes.c_uint64 * 1)(), (ctypes.c_uint32 * 2)(), 1) == -5
