"""Formulas over DataExprs through the sharded path (lk_eval_formula_dist): every operand is one sharded merged evaluation
whose rows land on rank 0's device, the join runs there.  World 2 and world 3 over the host transport on one GPU, world 1
through RCCL (loopback).

Data: that of tests/test_gpu_formula.py, made with the same generator arguments -- four synthetic segments of 2^14 rows
(hours 0, 0, 1, 2; value_mode 0: integer values, 30 % NULLs) and the small logs file; glob size 2, 60 s step.

Expectation: tests/formula_ref.expected over a second, plain engine (no communicator) on rank 0 that holds every segment:
operands through lk_eval_pushdown, then Formula.eval restated in Python -- nothing under test produces it.  Compared with
formula_ref.assert_rows, bit for bit.  Every operand is exact -- counts, min / max, sums and avg of integer values (one
division of two exact integers), p95 (integer bin counts), ces (register maxima) -- so the order in which the ranks'
partial tables fold cannot change a bit.  No real-valued sum is used: its bits would depend on that order.

Before the first distributed call rank 0 asserts, on the expectation alone, that it has rows on at least two timestamps,
that `+` has a key present on one side only and that `/` has a key with both sides: an empty comparison cannot pass."""
import os
import socket
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP, GLOB, NOW = 60_000, 2, 10 ** 14
HOURS = [0, 0, 1, 2]
LIMIT_S = 150   # per process
ENV_KEYS = ("LK_KEYRANGE_MIN_CELLS", "LK_DENSE_MAX_CELLS", "LK_FAULT")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The segments and the logs file of tests/test_gpu_formula.py's `data`, written once as files the ranks load."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lakeside_amd import synth
    from oracle import dataexpr as dx
    root = tmp_path_factory.mktemp("formula_dist")
    seg_files = []
    for i, h in enumerate(HOURS):
        seg = synth.make_segment(synth.segment_spec(i, rows=1 << 14, hour=h, null_frac=0.3, rg_rows=1 << 12,
                                                    page_rows=1 << 10))
        seg_files.append(str(root / f"seg{i}.parquet"))
        with open(seg_files[-1], "wb") as f:
            f.write(seg.bytes())
        seg.free()
    rng = np.random.default_rng(5)
    n = 6000
    ts = np.sort(synth.T0 + rng.integers(0, 10 * STEP, n))
    name_id = rng.integers(0, 3, n)
    svc_id = rng.integers(0, 4, n)
    logs = pa.table({
        dx.TIMESTAMP: pa.array(ts, pa.int64()),
        dx.VALUE: pa.array(rng.integers(1, 50, n).astype(np.float64), pa.float64()),
        dx.NAME: pa.array([f"m{k}" for k in name_id], pa.string(), mask=name_id == 0),
        synth.SERVICE: pa.array([("svc-qt", "svc-1", "svc-2", "x")[k] for k in svc_id], pa.string(), mask=svc_id == 3),
        "kind": pa.array(["k"] * n, pa.string()),
        "lat$number": pa.array(rng.integers(1, 900, n).astype(np.float64), pa.float64()),
    })
    logs_path = str(root / "logs.parquet")
    strings = [dx.NAME, synth.SERVICE, "kind"]
    pq.write_table(logs, logs_path, compression="NONE", use_dictionary=strings, row_group_size=2500,
                   data_page_size=1 << 20, column_encoding={c: "PLAIN" for c in logs.column_names if c not in strings})
    return {"hours": HOURS, "seg_files": seg_files, "logs": logs_path}


def _engine(files, **opts):
    from lakeside_amd.evaluator import Engine
    eng = Engine(0, **opts)
    for i, p in enumerate(files["seg_files"]):
        with open(p, "rb") as f:
            eng.put_segment(f"fx/{i}", f.read())
    eng.load_segment(files["logs"])
    return eng


def _cases(files):
    """name -> (formula, base expressions, {variable: (segment requests, paths)})."""
    from lakeside_amd import synth
    from tests.test_gpu_formula import all_names, be, synth_segs
    S, NS = synth.SERVICE, synth.NAMESPACE
    rate_f = {"op": "and", "q1": all_names(), "q2": synth.leaf(S, "regex", "^svc-0[0-4]")}
    m3 = synth.leaf(synth.NAME, "eq", "metric_03")
    fill_f = {"op": "and", "q1": m3, "q2": synth.leaf(S, "regex", "^svc-00")}
    one = synth.leaf(synth.NAME, "eq", "metric_02")
    s012, s0123 = synth_segs(files, [0, 1, 2]), synth_segs(files, [0, 1, 2, 3])
    rate = {"a": be(rate_f, "count", [S]), "b": be(all_names(), "count", [S])}
    k = synth.leaf("kind", "eq", "k")
    lseg = ([synth.segment_request(0, step=STEP, hour=0)], [files["logs"]])
    return {
        # b also reads the hour-2 segment: the operands' bucket bases differ
        "rate": ("a / b * 100", rate, {"a": s012, "b": s0123}),
        # a covers a subset of b's services: + keeps b's keys (one-sided)
        "fill": ("a + b", {"a": be(fill_f, "sum", [S]), "b": be(m3, "sum", [S])}, {"a": s012, "b": s012}),
        "minus": ("a - 5", rate, {"a": s012, "b": s0123}),
        "nogb": ("a / b", {"a": be(synth.leaf(synth.NAME, "in", "metric_01", "metric_02"), "sum"),
                           "b": be(synth.leaf(synth.NAME, "in", "metric_01", "metric_02", "metric_03"), "count")},
                 {"a": s012, "b": s0123}),
        "sumavg": ("a / b", {"a": be(one, "sum", [NS]), "b": be(one, "avg", [NS])}, {"a": s012, "b": s012}),
        "p95": ("p / n", {"p": be(one, "p95", [NS]), "n": be(one, "count", [NS])}, {"p": s012, "n": s012}),
        # c's rows carry no tags: under the groupBy they key as "", where n has the rows without a service
        "ces": ("c + n", {"c": be(one, "ces", [S]), "n": be(one, "count", [S])}, {"c": s012, "n": s012}),
        "logs": ("f / v", {"f": be(k, "sum", [S], field=("lat", "number")), "v": be(k, "count", [S])},
                 {"f": lseg, "v": lseg}),
    }


UPLOADED = {"p95": 1, "ces": 1}

SHARD_RULES = {
    "mod": lambda n: None,                                              # absent: i % world
    "rank1": lambda n: [1] * n,                                         # everything on rank 1
    "halves": lambda n: [0 if i < (n + 1) // 2 else 1 for i in range(n)],   # contiguous halves
}


def _expressions(case, shard_rule):
    from tests.test_gpu_formula import expressions
    _, bes, sp = case
    ex = expressions(bes, {k: sp[k][0] for k in bes}, {k: sp[k][1] for k in bes})
    for k in ex:
        sh = shard_rule(len(ex[k]["paths"]))
        if sh is not None:
            ex[k]["shard"] = sh
    return ex


def _expect(plain, case):
    from tests import formula_ref as fr
    formula, bes, sp = case
    return fr.expected(plain, bes, formula, {k: sp[k][0] for k in bes}, {k: sp[k][1] for k in bes}, STEP, GLOB, NOW)


def _guard(plain, cases, wants):
    """On the expectation alone: rows on two timestamps everywhere; one-sided keys under +; both-sided keys under /."""
    for name, (want, _, _) in wants.items():
        assert len(want) >= 2, f"{name}: the expectation has rows on {len(want)} timestamps"
    w, _, _ = _expect(plain, ("c + 0", cases["ces"][1], cases["ces"][2]))   # the ces operand alone: estimates, not zeros
    assert len(w) >= 2 and all(s.value >= 2.0 for cells in w.values() for s in cells.values()), "ces: no distinct keys"
    assert any(k in wants["ces"][0][ts] for ts, cells in w.items() for k in cells), "c + n: c's key is missing"
    for name in ("fill", "rate"):
        _, bes, sp = cases[name]
        side = {}
        for v in ("a", "b"):   # `v + 0`: the keys of v alone (a constant under groupBys takes the keys of the rows there are)
            w, _, _ = _expect(plain, (f"{v} + 0", bes, sp))
            side[v] = {(ts, key) for ts, cells in w.items() for key in cells}
        if name == "fill":
            assert side["a"] ^ side["b"], "a + b: no key present on one side only"
        else:
            assert side["a"] & side["b"], "a / b: no key with both sides"
            assert side["b"] - side["a"], "a / b: b has no key of its own"


def _run(eng, world, rank, name, case, rule, want, reduce=None):
    """One distributed call on this rank, checked: rank 0's rows against the expectation, 0 rows elsewhere, the stats."""
    from tests import formula_ref as fr
    formula = case[0]
    label = f"world {world} {name} shard {rule} mode {getattr(eng, 'mode', '')} reduce {reduce}"
    try:
        res = eng.eval_formula_dist(formula, _expressions(case, SHARD_RULES[rule] if isinstance(rule, str) else rule), GLOB)
    except Exception as e:   # every rank's failure in the log (spawn reports only one)
        print(f"rank {rank}: {label} failed: {e}", flush=True)
        raise
    st = res.stats["formula"]
    try:
        assert (st["world"], st["rank"]) == (world, rank), st
        assert [o["var"] for o in st["operands"]] == sorted(fr.variables(fr.parse(formula))), st   # evaluation order
        assert st["operands_uploaded"] == UPLOADED.get(name, 0), st
        assert sum(not o["kept"] for o in st["operands"]) == UPLOADED.get(name, 0), st
        if reduce is not None:
            assert [o["reduce"] for o in st["operands"] if o["kept"]] == [reduce] * st["operands_on_device"], st
        if rank == 0:
            w, _, gbs = want
            n = fr.assert_rows(res.rows(), w, gbs, label)
            assert n == len(res) > 0, (n, len(res))
            assert not res.globs.any()
            assert st["mode"] == getattr(eng, "mode", st["mode"]), st
        else:
            assert len(res) == 0 and all(o["rows"] == 0 for o in st["operands"]), st
    except AssertionError as e:
        print(f"rank {rank}: {label} mismatch: {str(e)[:2000]} stats {res.stats}", flush=True)
        raise
    return res


def _set_env(env):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)


def _worker2(rank, world, port, files):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    from lakeside_amd import LakesideError, synth
    from lakeside_amd._lib import LK_ERR_ARG, LK_ERR_DEVICE, LK_ERR_UNSUPPORTED
    from tests.test_gpu_formula import be
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _set_env({})
    engines = {"dense": _engine(files), "hash": _engine(files, formula_dense_max_cells=0)}
    plain = _engine(files) if rank == 0 else None
    try:
        for mode, e in engines.items():
            e.mode = mode
            e.comm_init_host(world, rank)
        cases = _cases(files)
        wants = {name: (_expect(plain, c) if rank == 0 else None) for name, c in cases.items()}
        if rank == 0:
            _guard(plain, cases, wants)
        # every formula under every shard rule (dense formula table), and once through the hash table
        for name, c in cases.items():
            for rule in SHARD_RULES:
                _run(engines["dense"], world, rank, name, c, rule, wants[name],
                     reduce="gather_to_root" if name in ("rate", "fill", "sumavg", "logs") else None)
            _run(engines["hash"], world, rank, name, c, "mod", wants[name])
        # the operands' tables hashed: their records gathered to rank 0, the rows kept there by sparse_write
        _set_env({"LK_DENSE_MAX_CELLS": "1"})
        for name in ("rate", "fill"):
            _run(engines["dense"], world, rank, name, cases[name], "halves", wants[name], reduce="records_to_root")
        _set_env({})
        eng = engines["dense"]
        good = ("rate", cases["rate"], "mod", wants["rate"])

        def refused(code, formula, ex, word):
            with pytest.raises(LakesideError) as err:
                eng.eval_formula_dist(formula, ex, GLOB)
            assert err.value.code == code and word in str(err.value), str(err.value)

        # refusals every rank reaches from the request alone (no rank is left in a collective); a good call follows
        _, bes, sp = cases["rate"]
        odd = dict(bes, c=be(bes["b"]["filter"], "count", [synth.NAMESPACE]))
        refused(LK_ERR_UNSUPPORTED, "a / c", _expressions(("a / c", odd, dict(sp, c=sp["b"])), SHARD_RULES["mod"]), "groupBy")
        _run(eng, world, rank, *good)
        refused(LK_ERR_ARG, "a / b", _expressions(cases["rate"], lambda n: [0] * (n + 1)), "shard")
        refused(LK_ERR_ARG, "a / b", _expressions(cases["rate"], lambda n: [world] * n), "shard")
        _run(eng, world, rank, *good)
        # a host exception injected on one rank at the first operand's closing stage fails the call on both ranks (no
        # rank starts the second operand alone); the communicator stays usable
        for spec in ("merge@1", "merge@0"):
            os.environ["LK_FAULT"] = spec
            try:
                refused(LK_ERR_DEVICE, "a / b * 100", _expressions(cases["rate"], SHARD_RULES["mod"]), "injected fault")
            finally:
                os.environ.pop("LK_FAULT", None)
            _run(eng, world, rank, *good)
        dist.barrier()
    finally:
        _set_env({})
        for e in list(engines.values()) + ([plain] if plain else []):
            e.close()
        dist.destroy_process_group()


def _worker3(rank, world, port, files):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _set_env({"LK_KEYRANGE_MIN_CELLS": "1"})
    eng = _engine(files)
    plain = _engine(files) if rank == 0 else None
    try:
        eng.comm_init_host(world, rank)
        cases = _cases(files)
        # i % 3, and a's three paths on ranks 0 and 1 only: rank 2's shard of a is empty, it still takes part
        rules = {"mod": lambda n: None, "empty2": lambda n: [i % 2 for i in range(n)] if n == 3 else None}
        for name in ("rate", "fill"):
            want = _expect(plain, cases[name]) if rank == 0 else None
            if rank == 0:
                assert len(want[0]) >= 2
            for rule in rules.values():
                res = _run(eng, world, rank, name, cases[name], rule, want, reduce="keyrange")
                assert all(o["kept"] for o in res.stats["formula"]["operands"])
        dist.barrier()
    finally:
        _set_env({})
        eng.close()
        if plain:
            plain.close()
        dist.destroy_process_group()


def _spawn(worker, world, files):
    import torch.multiprocessing as mp
    ctx = mp.spawn(worker, args=(world, _free_port(), files), nprocs=world, join=False)
    deadline = time.monotonic() + LIMIT_S
    while not ctx.join(timeout=2):   # raises when a rank failed (and ends the others)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"a rank was still running after {LIMIT_S} s")


def test_formula_dist_world2(files):
    """Both ranks on GPU 0: every formula x shard rule, both formula tables, the gather_to_root and records_to_root operand
    paths, refusals from the request alone and an injected operand failure, each followed by a good call."""
    _spawn(_worker2, 2, files)


def test_formula_dist_world3_keyrange(files):
    """Three ranks on GPU 0 with LK_KEYRANGE_MIN_CELLS=1: every kept operand takes the key-range reduce, its rows
    exchanged into rank 0's device; one shard rule leaves rank 2 without a segment of `a`."""
    _spawn(_worker3, 3, files)


def test_formula_dist_world1_rccl_loopback(files):
    """World 1 through RCCL with LK_COMM_LOOPBACK=1: the error rate over the three operand reduce paths."""
    from lakeside_amd.evaluator import Engine
    saved = {k: os.environ.get(k) for k in ("LK_COMM_LOOPBACK",) + ENV_KEYS}
    os.environ["LK_COMM_LOOPBACK"] = "1"
    eng = _engine(files)
    plain = _engine(files)
    try:
        eng.comm_init(Engine.unique_id(), 1, 0)
        case = _cases(files)["rate"]
        want = _expect(plain, case)
        assert len(want[0]) >= 2
        for reduce, env in [("gather_to_root", {"LK_KEYRANGE_MIN_CELLS": str(1 << 60)}), ("keyrange", {"LK_KEYRANGE_MIN_CELLS": "1"}),
                            ("records_to_root", {"LK_DENSE_MAX_CELLS": "1"})]:
            _set_env(env)
            _run(eng, 1, 0, "rate", case, lambda n: [0] * n, want, reduce=reduce)
        _set_env({})
        # queryapi.evaluate_formula(distributed=True): rank 0's payloads, against the expectation's
        from lakeside_amd import LakesideError, queryapi as qa
        from lakeside_amd._lib import LK_ERR_ARG
        from tests import formula_ref as fr
        formula, bes, sp = case
        segs, paths = {k: sp[k][0] for k in bes}, {k: sp[k][1] for k in bes}
        got = qa.evaluate_formula(eng, bes, formula, segs, paths, STEP, GLOB, NOW, distributed=True,
                                  shard_by_id={"a": [0] * len(paths["a"])})
        wantp = fr.expected_payloads(want[0], want[1], formula, bes)
        assert len(got) == len(wantp) > 0
        for g, w in zip(got, wantp):
            gm, wm = g["message"], w["message"]
            assert (g["id"], gm["timestamp"], gm["tags"], gm["label"]) == (formula, wm["timestamp"], wm["tags"], wm["label"])
            assert fr.same_value(gm["value"], wm["value"])
        # an engine without a communicator refuses as lk_eval_pushdown_dist does there
        with pytest.raises(LakesideError) as err:
            plain.eval_formula_dist(formula, _expressions(case, lambda n: None), GLOB)
        assert err.value.code == LK_ERR_ARG and "lk_comm_init" in str(err.value)
    finally:
        eng.close()
        plain.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
