"""+inf, -inf, NaN, overflowing sums and signed zeros in the value column through every aggregation path on the MI355X,
against the oracle.  Data and row classes: tests/nonfinite_data.py (checked on the CPU in tests/test_oracle_nonfinite.py).

Every run compares per-glob and merged rows with the oracle (assert_rows_equal) and, independently of that comparator,
asserts the class of every row (finite, +inf, -inf, NaN, -0.0, +0.0) and the number of rows per name, so that a slip of
the comparator cannot let an infinite sum pass as a finite one or as NaN."""
import collections
import json
import os

import numpy as np
import pytest

from tests import nonfinite_data as nf
from tests.parity import assert_rows_equal

pytestmark = pytest.mark.gpu

AGGS = ["sum", "avg", "min", "max", "count"]
NAME = "_cardinalhq.name"
VALUE = "_cardinalhq.value"
EPILOGUE_MAX = 1 << 16   # kernels.hpp kEpilogueMax: dense tables up to this many cells finalize in epilogue_small


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def data(engine, tmp_path_factory):
    """The two file sets, written once and loaded into the session's engine; oracle cells are cached per request."""
    root = tmp_path_factory.mktemp("nonfinite_gpu")
    sets = {label: nf.write_files(root, label) for label in ("clean", "mixed")}
    for paths, _ in sets.values():
        for p in paths:
            engine.load_segment(p)
    return {"sets": sets, "cells": {}, "root": root}


def _num(k, op, v):
    return {"k": k, "v": [v], "op": op, "extracted": False, "computed": False, "dataType": "number"}


def _request(agg, filt=None, gbs=(NAME,), field=None, step=nf.STEP):
    from lakeside_amd import synth
    return json.dumps(synth.pushdown(filt or nf.all_names(), nf.segments(step), agg, list(gbs), field=field))


def _cells(data, label, filt, gbs, step=nf.STEP):
    """Per-glob oracle cells (with their raw values: one evaluation serves every aggregate of the request)."""
    from oracle import dataexpr as dx
    key = (label, json.dumps(filt, sort_keys=True), tuple(gbs), step)
    if key not in data["cells"]:
        paths, blobs = data["sets"][label]
        data["cells"][key] = dx.evaluate_glob_cells(dx.parse_pushdown(_request("sum", filt, gbs, step=step)), nf.GLOB, paths,
                                                    sources=blobs)
    return data["cells"][key]


def _histogram(rows, agg):
    """(name, class) -> rows; the sign of a zero sum is not pinned."""
    def cls(v):
        c = nf.value_class(v)
        return "0" if agg in ("sum", "avg") and c in ("-0", "+0") else c
    return collections.Counter((tags.get("name"), cls(v)) for _, v, tags in rows)


def _compare(got, want, agg, scope, label, classes, scale=None):
    if scale:
        want = [(t, v / scale, tags) for t, v, tags in want]
    assert_rows_equal(got, want, agg, label)
    assert _histogram(got, agg) == _histogram(want, agg), f"{label}: classes differ from the oracle's"
    if classes:
        nf.assert_classes(got, agg, scope, label)


def _run(engine, data, label, agg, filt=None, gbs=(NAME,), classes=True, field=None, scale=None, what="",
         step=nf.STEP):
    """One request per glob and merged against the oracle; returns (per-glob result, merged result)."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    from oracle import dataexpr as dx
    paths, _ = data["sets"][label]
    cells = _cells(data, label, filt, gbs, step)
    pr = dx.parse_pushdown(_request(agg, filt, gbs, step=step))
    req = _request(agg, filt, gbs, field, step)
    what = f"{what} {label} {agg}"
    pg = engine.eval_pushdown(req, paths, nf.GLOB, LK_PER_GLOB_ROWS)
    for gi, (g, cs) in enumerate(zip(pg.per_glob(len(cells)), cells)):
        _compare(g, [(c.ts, c.agg_value(agg), c.tags) for c in cs], agg, gi, f"{what} glob {gi}", classes, scale)
    if scale and agg == "avg":   # merged avg over a duration field is refused (its SUM / COUNT split)
        return pg, None
    mg = engine.eval_pushdown(req, paths, nf.GLOB, LK_MERGED)
    _compare(mg.rows(), dx.merge_glob_cells(pr, cells), agg, "merged", f"{what} merged", classes, scale)
    return pg, mg


def _same_rows(a, b, agg, what):
    assert list(a.ts) == list(b.ts) and a.tags == b.tags, what
    if agg not in ("sum", "avg"):
        assert np.array_equal(np.asarray(a.values).view(np.uint64), np.asarray(b.values).view(np.uint64)), what
    else:
        assert [nf.value_class(v) for v in a.values] == [nf.value_class(v) for v in b.values], what


@pytest.mark.parametrize("agg", AGGS)
def test_lean_dense_small_epilogue(engine, data, agg):
    """1. scan_lean into the dense table, finalized by epilogue_small; 3. the same through the LDS hash (LK_NO_DIRECT)
    instead of the per-tile direct table: the same rows, bit for bit for count / min / max."""
    pg, mg = _run(engine, data, "clean", agg, what="lean")
    for r in (pg, mg):
        st = r.stats
        assert st["general_segments"] == 0 and st["table"] == "dense" and st["cells"] <= EPILOGUE_MAX, st
        if agg == "sum":
            assert st["exact_sum"] == 0, st   # intinf is integral but for its +inf
    with _Env(LK_NO_DIRECT=1):
        pg2, mg2 = _run(engine, data, "clean", agg, what="lean lds hash")
    _same_rows(pg2, pg, agg, f"LK_NO_DIRECT per glob {agg}")
    _same_rows(mg2, mg, agg, f"LK_NO_DIRECT merged {agg}")


@pytest.mark.parametrize("agg", AGGS)
def test_tiles_with_nulls(engine, data, agg):
    """2. scan_tiles: f1 of `mixed` holds NULL values (has_nulls), so its tile leaves scan_lean."""
    pg, mg = _run(engine, data, "mixed", agg, what="tiles")
    assert mg.stats["general_segments"] == 0 and mg.stats["table"] == "dense", mg.stats


@pytest.mark.parametrize("label", ["clean", "mixed"])
@pytest.mark.parametrize("agg", AGGS)
def test_hash_table_sparse_finalize(engine, data, label, agg):
    """4. the hash-mode table and the sparse finalize (runs_write)."""
    with _Env(LK_DENSE_MAX_CELLS=0):
        pg, mg = _run(engine, data, label, agg, what="hash")
    assert pg.stats["table"] == "hash" and mg.stats["table"] == "hash", (pg.stats, mg.stats)


@pytest.mark.parametrize("agg", AGGS)
def test_large_dense_finalize(engine, data, agg):
    """5. `:by name, svc` at a 300 s step: 12 buckets x 13 names x 513 services (a NULL slot each) exceed kEpilogueMax
    in the merged table too (globs share its cells), so finalize_count / finalize_write run instead of epilogue_small.
    A (name, svc) cell holds a few rows of its name, so the per-name classes do not apply; the class histogram
    against the oracle's does."""
    pg, mg = _run(engine, data, "clean", agg, gbs=(NAME, nf.SVC), classes=False, what="large dense", step=300_000)
    assert pg.stats["table"] == "dense" and pg.stats["cells"] > EPILOGUE_MAX, pg.stats
    assert mg.stats["table"] == "dense" and mg.stats["cells"] > EPILOGUE_MAX, mg.stats
    if agg in ("sum", "avg", "max"):
        h = _histogram(mg.rows(), agg)
        assert h[("pinf", "+inf")] > 6 and h[("ovfp", "fin")] + h[("ovfp", "+inf")] > 6
        assert h[("naninf", "nan")] > 6 and h[("intinf", "+inf")] == 6


@pytest.mark.parametrize("agg", AGGS)
def test_general_row_scan(engine, data, agg):
    """6. a numeric leaf on an INT64 column sends every segment through the general row scan."""
    filt = {"op": "and", "q1": nf.all_names(), "q2": _num(nf.ATTR, "ge", "0")}
    pg, mg = _run(engine, data, "clean", agg, filt=filt, what="general")
    assert pg.stats["general_segments"] == 3 and mg.stats["general_segments"] == 3, (pg.stats, mg.stats)


@pytest.mark.parametrize("label", ["clean", "mixed"])
def test_value_leaves(engine, data, label):
    """7. comparisons of the value column itself: `gt 10` passes +inf and NaN (DuckDB orders NaN greatest) and not
    -inf; `lt -10` passes only -inf and ovfn's values."""
    files = {0: 2, 1: 1, "merged": 3}
    pg, mg = _run(engine, data, label, "count", filt=_num(VALUE, "gt", "10"), classes=False, what="gt 10")
    for scope, rows in list(enumerate(pg.per_glob(2))) + [("merged", mg.rows())]:
        by = collections.defaultdict(list)
        for _, v, tags in rows:
            by[tags["name"]].append(v)
        assert not {"negz", "zmix", "ovfn"} & set(by), sorted(by)
        for k in ("pinf", "both", "naninf", "ovfp", "ovfm", "bigfin"):
            assert len(by[k]) == nf.NBUCKETS, (scope, k)
        assert all(v >= 4 * files[scope] for v in by["naninf"])          # 2 NaN and 2 +inf per (file, bucket)
        assert all(v >= 2 * files[scope] for v in by["pinf"] + by["both"])
        assert all(v == 8 * files[scope] for v in by["ovfm"] + by["bigfin"])
    pg, mg = _run(engine, data, label, "count", filt=_num(VALUE, "lt", "-10"), classes=False, what="lt -10")
    for scope, rows in list(enumerate(pg.per_glob(2))) + [("merged", mg.rows())]:
        by = collections.defaultdict(list)
        for _, v, tags in rows:
            by[tags["name"]].append(v)
        assert set(by) == {"ninf", "both", "ovfn"}, sorted(by)
        assert by["ninf"] == by["both"] == [2.0 * files[scope]] * nf.NBUCKETS, (scope, by)
        assert len(by["ovfn"]) == nf.NBUCKETS and all(v >= 8 * files[scope] for v in by["ovfn"])
    # the sums of the passing values: +inf where an infinity passed
    pg, mg = _run(engine, data, label, "sum", filt=_num(VALUE, "gt", "10"), classes=False, what="sum gt 10")
    h = _histogram(mg.rows(), "sum")
    assert h[("pinf", "+inf")] == h[("both", "+inf")] == h[("ovfp", "+inf")] == h[("naninf", "nan")] == nf.NBUCKETS


@pytest.mark.parametrize("label", ["clean", "mixed"])
@pytest.mark.parametrize("agg", ["sum", "max"])
def test_field_chart(engine, data, label, agg):
    """8. the field chart over `lat$number` and over `lat$duration`, both copies of the value column (NULL where it is
    NULL: `IS NOT NULL` then only drops rows that hold no value): the value chart's rows, over 1e6 for the duration
    (inf / 1e6 stays inf)."""
    _run(engine, data, label, agg, field=("lat", "number"), what="lat$number")
    pg, mg = _run(engine, data, label, agg, field=("lat", "duration"), scale=1e6, classes=False, what="lat$duration")
    for scope, rows in list(enumerate(pg.per_glob(2))) + [("merged", mg.rows())]:
        h = _histogram(rows, agg)
        assert h[("pinf", "+inf")] == h[("ovfp", "+inf" if agg == "sum" else "fin")] == nf.NBUCKETS
        assert h[("ninf", "-inf" if agg == "sum" else "fin")] == h[("naninf", "nan")] == nf.NBUCKETS
        assert h[("ovfm", "+inf" if (agg == "sum" and scope == "merged") else "fin")] == nf.NBUCKETS


def test_formula_over_infinite_operands(engine, data):
    """9. a = sum by name, b = count by name (dense formula table): a / b has the classes of the merged avg; a - a is
    NaN for every infinite or NaN sum -- a row, not a dropped key -- and +0.0 elsewhere."""
    from tests import formula_ref as fr
    from tests.test_gpu_formula import be, expressions
    paths, _ = data["sets"]["clean"]
    bes = {"a": be(nf.all_names(), "sum", [NAME]), "b": be(nf.all_names(), "count", [NAME])}
    segs = {k: nf.segments() for k in bes}
    pths = {k: paths for k in bes}
    rows = {}
    for formula in ("a / b", "a - a"):
        want, _, gbs = fr.expected(engine, bes, formula, segs, pths, nf.STEP, nf.GLOB, 10 ** 14)
        res = engine.eval_formula(formula, expressions(bes, segs, pths), nf.GLOB)
        assert fr.assert_rows(res.rows(), want, gbs, formula) == len(res) == nf.NBUCKETS * len(nf.KINDS)
        assert res.stats["formula"]["mode"] == "dense", res.stats
        rows[formula] = res.rows()
    nf.assert_classes(rows["a / b"], "avg", "merged", "a / b")
    by = collections.defaultdict(list)
    for _, v, tags in rows["a - a"]:
        by[tags["name"]].append(nf.value_class(v))
    for k in nf.KINDS:
        nonfinite = nf.expected_class(k, "sum", "merged") & {"+inf", "-inf", "nan"}
        assert by[k] == ["nan" if nonfinite else "+0"] * nf.NBUCKETS, (k, by[k])


def _worker_nonfinite(rank, world, port, paths):
    """sum / min / max by name through the distributed path (host transport, world 2; the modulo shard puts f0
    and f2 on rank 0 and f1 on rank 1, so glob 0's cells are folded from both ranks): the dense tables through
    merge_tables, the hash tables' records through merge_records."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = Engine(0)
    try:
        eng.comm_init_host(world, rank)
        for reduce, env in (("gather_to_root", {}),
                            ("records_to_root", {"LK_DENSE_MAX_CELLS": "1", "LK_KEYRANGE_MIN_CELLS": str(1 << 60)})):
            with _Env(**env):
                for agg in ("sum", "min", "max"):
                    req = _request(agg)
                    try:
                        res = eng.eval_pushdown_dist(req, paths, None, nf.GLOB)
                    except Exception as e:   # both ranks' failures in the log (spawn reports only one)
                        print(f"rank {rank}: {reduce} {agg} failed: {e}", flush=True)
                        raise
                    if rank != 0:
                        assert len(res) == 0
                        continue
                    try:
                        assert res.stats["reduce"] == reduce, res.stats
                        want = dx.evaluate_merged(dx.parse_pushdown(req), paths, nf.GLOB)
                        _compare(res.rows(), want, agg, "merged", f"dist {reduce} {agg}", True)
                    except AssertionError as e:
                        print(f"rank 0: {reduce} {agg} mismatch: {str(e)[:2000]} stats {res.stats}", flush=True)
                        raise
        dist.barrier()
    finally:
        eng.close()
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_dist_world2(data):
    """10. world 2 over the host transport."""
    import torch.multiprocessing as mp

    from tests.test_gpu_dist import _free_port
    paths, _ = data["sets"]["clean"]
    mp.spawn(_worker_nonfinite, args=(2, _free_port(), paths), nprocs=2, join=True)
