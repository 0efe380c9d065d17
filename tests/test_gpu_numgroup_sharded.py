"""Numeric groupBys through the sharded path (lk_eval_pushdown_dist): the ranks agree on each groupBy's class per glob,
plan again from the agreed classes, and agree on the set of group values, so rank 0 answers what lk_eval_pushdown answers
over all the paths, whatever the shard ("distributed").

Host transport on one GPU (mp.spawn, a deadline and a kill per process as tests/test_gpu_numgroup_dist.py): three world-2
spawns, one world-3 spawn, one world-1 RCCL loopback.  Files: numgroup_data.write_file at 1,500-2,500 rows in 2,048-row
row groups.  Expectation: the oracle over numgroup_ref.write_twins, computed once here and handed to the ranks; bar:
tests/parity.py::assert_rows_equal as it stands."""
import copy
import json
import os
import socket
import time

import numpy as np
import pytest

from tests import numgroup_data as nd
from tests import numgroup_ref as nr

pytestmark = pytest.mark.gpu

LIMIT_S = 150   # per process
GLOB = 2
AGGS = ("sum", "min", "max", "count", "avg")
NAMES = ("metric_00", "metric_02")
EXTRA = "attr.m"   # a fifth numeric column (the refusal of five numeric groupBys)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _segs(n, step=60_000, dataset="logs"):
    from lakeside_amd import synth
    return [synth.segment_request(i, step=step, hour=0, dataset=dataset) for i in range(n)]


def _name_in():
    from lakeside_amd import synth
    return synth.leaf(synth.NAME, "in", *NAMES)


def _num(k, op, v):
    return {"k": k, "v": [v], "op": op, "extracted": False, "computed": False, "dataType": "number"}


def _request(agg, gbs, n, filt=None, step=60_000, dataset="logs", field=None, rollup=None):
    from lakeside_amd import synth
    d = synth.pushdown(filt or _name_in(), _segs(n, step, dataset), agg, list(gbs), dataset=dataset, field=field)
    if rollup:
        d["baseExpr"]["chart"]["rollup"] = rollup
    return json.dumps(d)


def _with_agg(pr, agg):
    pr = copy.deepcopy(pr)
    pr.baseExpr.chart.aggregation = agg
    return pr


def _texts(twin, column=nd.STATUS):
    """The texts (None: NULL, or no such column) of `column` over the twin's rows that pass the name filter."""
    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    t = pq.read_table(twin)
    keep = [n in NAMES for n in t.column(dx.NAME).to_pylist()]
    if column not in t.column_names:
        return {None} if any(keep) else set()
    return {v for v, k in zip(t.column(column).to_pylist(), keep) if k}


def _check_shards(twins, shard, world=2, both=True):
    """On the twins alone: a text only rank 1's shard holds, one both shards hold, a NULL group."""
    shard = shard if shard is not None else [i % world for i in range(len(twins))]
    per = [set().union(*([_texts(t) for t, r in zip(twins, shard) if r == w] or [set()])) for w in range(world)]
    assert (per[1] - per[0]) - {None}, "no text only rank 1 holds"
    if both:
        assert (per[0] & per[1]) - {None}, "no text both shards hold"
    assert None in set().union(*per), "no NULL group"
    return per


class Files:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The files, their twins and the oracle's rows of every aggregate case, once for the module."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    root = tmp_path_factory.mktemp("numgroup_sharded")
    F = Files()
    F.root = str(root)
    w = lambda name, kind, seed, rows, **kw: nd.write_file(root / name, kind, seed=seed, rows=rows, **kw)   # noqa: E731
    # row 1: glob 0 = INT32 (rank 0) + DOUBLE (rank 1) -> DOUBLE; glob 1 = INT64 + FLOAT -> FLOAT
    F.p1 = [w("d.parquet", "D", 701, 1500), w("b.parquet", "B", 702, 1700), w("a.parquet", "A", 703, 1900), w("c.parquet", "C", 704, 2100)]
    F.t1 = nr.write_twins(F.p1, [nd.STATUS, nd.RATIO], GLOB, str(root / "t1"))
    # row 2: BIGINT glob (no -1 on rank 0) | DOUBLE glob | absent + INT64 | all NULL + INT64
    F.p2 = [w("a_pos.parquet", "A", 711, 1500, values=[200, 404, 500, 2 ** 53 + 1]), w("d2.parquet", "D", 712, 1600),
            w("b2.parquet", "B", 713, 1700), w("d3.parquet", "D", 714, 1800),
            w("f.parquet", "F", 715, 1500), w("a2.parquet", "A", 716, 2500),
            w("g.parquet", "G", 717, 1500), w("a3.parquet", "A", 718, 2000)]
    F.t2 = nr.write_twins(F.p2, [nd.STATUS], GLOB, str(root / "t2"))
    # row 5: 300 distinct INT64 values on rank 1 alone (two of them rank 0's as well)
    wide = [200, 404] + [int(v) for v in np.random.default_rng(7).choice(10 ** 9, 298, replace=False) + 10 ** 6]
    F.p5 = [w("a5.parquet", "A", 721, 1500), w("wide.parquet", "A", 722, 2500, values=wide)]
    F.t5 = nr.write_twins(F.p5, [nd.STATUS], GLOB, str(root / "t5"))
    # world 3: {D, B} on ranks 0, 1 | {A, C} on ranks 2, 0 | {A, B} on ranks 1, 2
    F.p3 = F.p1 + [w("a4.parquet", "A", 731, 1600), w("b4.parquet", "B", 732, 1800)]
    F.t3 = nr.write_twins(F.p3, [nd.STATUS], GLOB, str(root / "t3"))
    # refusals
    F.bool_int = [w("e.parquet", "E", 741, 1500), F.p1[2]]
    F.text_num = [w("v1.parquet", "V", 742, 1500), w("v2.parquet", "V", 743, 1500), F.p1[2], F.p1[0]]
    F.five = []
    for i, p in enumerate(F.p1[:2]):
        t = pq.read_table(p)
        t = t.append_column(EXTRA, pa.array(np.arange(t.num_rows) % 3, pa.int64()))
        F.five.append(str(root / f"five_{i}.parquet"))
        pq.write_table(t, F.five[-1], compression="NONE", row_group_size=2048)
    F.metrics = [w("m0.parquet", "A", 751, 1500, metrics=True), w("m1.parquet", "A", 752, 1500, metrics=True)]

    def rows(paths_twins, gbs, filt=None, aggs=AGGS):
        pr = dx.parse_pushdown(_request("sum", gbs, len(paths_twins), filt))
        cells = dx.evaluate_glob_cells(pr, GLOB, paths_twins)
        return {a: dx.merge_glob_cells(_with_agg(pr, a), cells) for a in aggs}
    F.want1 = rows(F.t1, (nd.STATUS,))
    F.want2 = rows(F.t2, (nd.STATUS,), aggs=("sum", "count"))
    F.want5 = rows(F.t5, (nd.STATUS,), aggs=("count",))
    F.want3 = rows(F.t3, (nd.STATUS,), aggs=("sum", "avg"))
    F.want_two = rows(F.t1, (nd.STATUS, nd.RATIO, nd.SVC), aggs=("sum", "max"))
    # `status ge 400 :by status`: the twins hold text, so the original rows are filtered first (a comparison under the union
    # type: NaN orders greatest, NULL fails) and the oracle runs over the twins of what is left, without the leaf
    kept = []
    for i, p in enumerate(F.p1):
        t = pq.read_table(p)
        v = t.column(nd.STATUS).cast(pa.float64(), safe=False).to_numpy(zero_copy_only=False)
        valid = t.column(nd.STATUS).is_valid().to_numpy(zero_copy_only=False)
        kept.append(str(root / f"kept_{i}.parquet"))
        pq.write_table(t.filter(pa.array(valid & ((v >= 400.0) | np.isnan(v)))), kept[-1])
    F.want_leaf = rows(nr.write_twins(kept, [nd.STATUS], GLOB, str(root / "tk")), (nd.STATUS,), aggs=("count", "min"))
    from tests import fieldchart_ref as fr
    F.field_req = _request("avg", (nd.STATUS,), 4, field=("lat", "number"))
    pr, cells, scale = fr.expected_cells(F.field_req, F.t1, GLOB, str(root / "ft"))
    F.want_field = fr.merged_rows(pr, cells, scale, "avg")
    return F


def _case(label, req, paths, want=None, agg="sum", shard=None, kind="rows", env=None, reduce="gather_to_root", **kw):
    return dict(label=label, req=req, paths=list(paths), want=want, agg=agg, shard=shard, kind=kind, env=env or {},
                reduce=reduce, **kw)


def _tag_dictionary(res, column):
    import ctypes

    from lakeside_amd import _lib
    L = _lib.lib()
    h = res._owner.h
    c = res.tag_names.index(column)
    assert c < L.lk_result_num_group_columns(h)
    stride, ndim = ctypes.c_uint64(), ctypes.c_uint64()
    p = L.lk_result_tag_dictionary(h, c, ctypes.byref(stride), ctypes.byref(ndim))
    return [ctypes.string_at(p[d]) if p[d] else None for d in range(ndim.value)]


def _worker(rank, world, port, cases, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    from lakeside_amd import LakesideError
    from lakeside_amd._lib import LK_ERR_DEVICE, LK_ERR_UNSUPPORTED
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx, hll
    from tests.parity import assert_rows_equal
    from tests.test_gpu_features import _pct_rows_equal
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = Engine(0)
    report = {}
    try:
        eng.comm_init_host(world, rank)
        for c in cases:
            label = c["label"]
            for k, v in c["env"].items():
                os.environ[k] = v
            try:
                t0 = time.monotonic()
                if c["kind"] in ("refused", "fault"):
                    with pytest.raises(LakesideError) as e:
                        eng.eval_pushdown_dist(c["req"], c["paths"], c["shard"], GLOB)
                    assert time.monotonic() - t0 < LIMIT_S / 2, label
                    assert e.value.code == (LK_ERR_UNSUPPORTED if c["kind"] == "refused" else LK_ERR_DEVICE), (label, str(e.value))
                    assert c["needle"] in str(e.value), (label, str(e.value))
                    report[label] = {"message": str(e.value)}
                    continue
                res = eng.eval_pushdown_dist(c["req"], c["paths"], c["shard"], GLOB)
            finally:
                for k in c["env"]:
                    del os.environ[k]
            st = res.stats
            report[label] = {k: st.get(k) for k in ("reduce", "numeric_dims", "numdim_ms", "numdim_attempts", "numdim_exchange_ms",
                                                    "numdim_exchange_bytes", "scan_ms", "collectives", "allgathers")}
            assert st["reduce"] == c["reduce"], (label, st)
            assert st["numdim_attempts"] >= 1 and st["numdim_exchange_bytes"] > 0 and st["numdim_exchange_ms"] >= 0, (label, st)
            if rank != 0:
                assert len(res) == 0, label
                continue
            if c["kind"] == "rows":
                assert len(c["want"]) > 0, label
                assert_rows_equal(res.rows(), c["want"], c["agg"], label)
            elif c["kind"] == "p95":
                pr = dx.parse_pushdown(c["req"])
                want = dx.merge_percentile(pr, dx.evaluate_percentile_per_glob(pr, GLOB, c["twins"]))
                got = [(int(res.ts[r]), res.tags[r], float(res.values[r]), res.sketch(r)) for r in range(len(res))]
                assert len(got) > 10, label
                _pct_rows_equal(got, want, 0.95, label)
            elif c["kind"] == "ces":
                pr = dx.parse_pushdown(c["req"])
                want = dx.merge_ces(dx.evaluate_ces_per_glob(pr, GLOB, c["twins"]))
                got = [(int(t), float(v)) for t, v in zip(res.ts, res.values)]
                assert got == [(ts, hll.estimate(ks)) for ts, ks in want] and max(v for _, v in got) > 4, label
            for t in c.get("tags", ()):
                assert t in {x.get(nd.STATUS) for x in res.tags}, (label, t)
            if "dictionary" in c:   # rank 0 owns the union's strings, texts none of its own segments hold included
                d = _tag_dictionary(res, nd.STATUS)
                assert d[-1] is None and d[:-1] == c["dictionary"], (label, d)
        dist.barrier()
    finally:
        with open(os.path.join(out_dir, f"report_{rank}.json"), "w") as f:
            json.dump(report, f)
        eng.close()
        dist.destroy_process_group()


def _spawn(world, cases, out_dir):
    import torch.multiprocessing as mp
    os.makedirs(out_dir, exist_ok=True)
    ctx = mp.spawn(_worker, args=(world, _free_port(), cases, str(out_dir)), nprocs=world, join=False)
    deadline = time.monotonic() + LIMIT_S
    while not ctx.join(timeout=2):   # raises when a rank failed (and ends the other)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"a rank was still running after {LIMIT_S} s")
    reports = [json.load(open(os.path.join(out_dir, f"report_{r}.json"))) for r in range(world)]
    print(json.dumps(reports[min(1, world - 1)], indent=1))   # (rank 1's stats of every case, for the record)
    return reports


# ---- rows 1, 2, 5, 6: unions over ranks, shards, regrow on one rank, rank 0's dictionary ----

def test_unions_over_ranks_and_shards(files, tmp_path):
    F = files
    per = _check_shards(F.t1, None)
    _check_shards(F.t1, [1, 0, 1, 0])
    _check_shards(F.t1, [1, 1, 1, 1], both=False)
    assert "200.0" in per[0] & per[1] and "NaN" in per[1] - per[0]
    cases = []
    for agg in AGGS:
        for name, shard in (("modulo", None), ("last", [1, 1, 1, 1]), ("swapped", [1, 0, 1, 0])):
            cases.append(_case(f"row1 {agg} {name}", _request(agg, (nd.STATUS,), 4), F.p1, F.want1[agg], agg, shard,
                               tags=("200.0", "NaN", "1.6777216E7")))
    every = sorted(t.encode() for t in set().union(*[_texts(t) for t in F.t1]) - {None})
    cases[0]["dictionary"] = every          # modulo: rank 0 scanned the INT32 and INT64 files only
    cases[1]["dictionary"] = every          # last: rank 0 scanned nothing
    # row 2: "200" of the BIGINT globs and "200.0" of the DOUBLE glob stay apart; -1 (the all-ones key) on rank 1 only
    per2 = _check_shards(F.t2, None)
    assert "-1" in per2[1] - per2[0] and "-9223372036854775808" in per2[1] - per2[0]
    assert _texts(F.t2[4]) == {None} and _texts(F.t2[6]) == {None}   # the absent and the all-NULL file
    for agg in ("sum", "count"):
        cases.append(_case(f"row2 {agg}", _request(agg, (nd.STATUS,), 8), F.p2, F.want2[agg], agg,
                           tags=("200", "200.0", "-1", "-1.0", "9007199254740993", None)))
    # row 5: only rank 1's table regrows
    _check_shards(F.t5, None)
    cases.append(_case("row5 regrow", _request("count", (nd.STATUS,), 2), F.p5, F.want5["count"], "count",
                       env={"LK_NUMDIM_INIT_SLOTS": "64"}))
    cases.append(_case("row5 plain", _request("count", (nd.STATUS,), 2), F.p5, F.want5["count"], "count"))
    rep = _spawn(2, cases, tmp_path / "out")
    assert rep[0]["row5 regrow"]["numdim_attempts"] == 1 and rep[1]["row5 regrow"]["numdim_attempts"] > 1, rep
    assert rep[0]["row5 plain"]["numdim_attempts"] == rep[1]["row5 plain"]["numdim_attempts"] == 1
    assert rep[0]["row5 regrow"]["numeric_dims"] == rep[1]["row5 regrow"]["numeric_dims"] == \
        [{"column": nd.STATUS, "values": len(set().union(*[_texts(t) for t in F.t5]) - {None})}]
    for label in rep[0]:   # every rank built the same dimensions
        assert rep[0][label]["numeric_dims"] == rep[1][label]["numeric_dims"], label


# ---- rows 3, 4: several dimensions, a leaf on the group column, a field chart, sketches (records_to_root) ----

def test_shapes_by_status(files, tmp_path):
    F = files
    _check_shards(F.t1, None)
    two = (nd.STATUS, nd.RATIO, nd.SVC)
    leaf = {"op": "and", "q1": _name_in(), "q2": _num(nd.STATUS, "ge", "400")}
    cases = [_case(f"two {agg}", _request(agg, two, 4), F.p1, F.want_two[agg], agg) for agg in ("sum", "max")]
    cases += [_case(f"leaf {agg}", _request(agg, (nd.STATUS,), 4, leaf), F.p1, F.want_leaf[agg], agg, tags=("404.0", "NaN"))
              for agg in ("count", "min")]
    cases.append(_case("field avg", F.field_req, F.p1, F.want_field, "avg"))
    cases.append(_case("p95", _request("p95", (nd.STATUS,), 4, step=600_000, rollup="p95"), F.p1, kind="p95", twins=F.t1,
                       reduce="records_to_root"))
    cases.append(_case("ces", _request("ces", (nd.STATUS, nd.SVC), 4, step=600_000), F.p1, kind="ces", twins=F.t1,
                       reduce="records_to_root"))
    rep = _spawn(2, cases, tmp_path / "out")
    assert [d["column"] for d in rep[1]["two sum"]["numeric_dims"]] == [nd.STATUS, nd.RATIO]
    assert "200.0" not in {t.get(nd.STATUS) for _, _, t in F.want_leaf["count"]}


# ---- rows 7, 8: refusals and injected faults, the same on every rank; the communicator answers afterwards ----

def test_refusals_and_faults_on_every_rank(files, tmp_path):
    F = files
    ok = lambda i: _case(f"valid {i}", _request("sum", (nd.STATUS,), 4), F.p1, F.want1["sum"])   # noqa: E731
    by = lambda n, gbs=(nd.STATUS,): _request("sum", gbs, n)                                      # noqa: E731
    over = ", over the ranks of this distributed evaluation"
    refusals = [
        ("boolean", by(2), F.bool_int, "is BOOLEAN in some files and numeric in others of glob 0" + over),
        ("varchar glob", by(4), F.text_num, "is VARCHAR in glob 0 and numeric in glob 1 of the same call" + over),
        ("five", by(2, (nd.STATUS, nd.RATIO, nd.OTHER, nd.LAT, EXTRA)), F.five, "more than 4 numeric groupBys"),
        ("metrics p95", _request("p95", (nd.STATUS,), 2, dataset="metrics", rollup="max"), F.metrics,
         "metrics p<NN> / ces take no numeric groupBy"),
    ]
    cases = []
    for i, (label, req, paths, needle) in enumerate(refusals):
        cases.append(_case(label, req, paths, kind="refused", needle=needle))
        cases.append(ok(i))
    for i, spec in enumerate(("numdim@1", "numdim_ids@0")):
        cases.append(_case(f"fault {spec}", by(4), F.p1, kind="fault", needle="injected fault", env={"LK_FAULT": spec}))
        cases.append(ok(10 + i))
    rep = _spawn(2, cases, tmp_path / "out")
    for label, _, _, _ in refusals:
        assert rep[0][label]["message"] == rep[1][label]["message"] and "numeric groupBy" in rep[0][label]["message"], label


# ---- row 4: the key-range reduce at world 3 ----

def test_world3_keyrange_and_gather(files, tmp_path):
    F = files
    _check_shards(F.t3, None, world=3)
    cases = [_case(f"keyrange {agg}", _request(agg, (nd.STATUS,), 6), F.p3, F.want3[agg], agg, reduce="keyrange",
                   env={"LK_KEYRANGE_MIN_CELLS": "1"}) for agg in ("sum", "avg")]
    cases.append(_case("gather sum", _request("sum", (nd.STATUS,), 6), F.p3, F.want3["sum"], "sum"))
    rep = _spawn(3, cases, tmp_path / "out")
    assert rep[0]["gather sum"]["numeric_dims"] == rep[2]["gather sum"]["numeric_dims"]


# ---- row 9: the new all-gather through RCCL ----

def test_world1_rccl_loopback(files):
    from lakeside_amd.evaluator import Engine
    from tests.parity import assert_rows_equal
    F = files
    saved = os.environ.get("LK_COMM_LOOPBACK")
    os.environ["LK_COMM_LOOPBACK"] = "1"
    eng = Engine(0)
    try:
        eng.comm_init(Engine.unique_id(), 1, 0)
        for agg in ("sum", "min"):
            res = eng.eval_pushdown_dist(_request(agg, (nd.STATUS,), 4), F.p1, [0, 0, 0, 0], GLOB)
            assert_rows_equal(res.rows(), F.want1[agg], agg, f"loopback {agg}")
            st = res.stats
            assert st["numeric_dims"][0]["column"] == nd.STATUS and st["numdim_exchange_bytes"] > 0, st
    finally:
        eng.close()
        if saved is None:
            os.environ.pop("LK_COMM_LOOPBACK", None)
        else:
            os.environ["LK_COMM_LOOPBACK"] = saved
