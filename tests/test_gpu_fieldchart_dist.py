"""Field charts through the sharded path (lk_eval_pushdown_dist), world 2 over the host transport on one GPU: a numeric
and a VARCHAR chart field, merged rows on rank 0 against the same expectation as the single-GPU tests
(tests/fieldchart_ref.py).  The per-glob type class of the field travels with the glob unions every rank agrees on."""
import json
import os
import socket
import time

import pytest

pytestmark = pytest.mark.gpu

SVC = "resource.service.name"
LIMIT_S = 150   # per process


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, paths, twin_root):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    from lakeside_amd import synth
    from lakeside_amd.evaluator import Engine
    from tests import fieldchart_ref as fr
    from tests.parity import assert_rows_equal
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = Engine(0)
    try:
        eng.comm_init_host(world, rank)
        segs = [synth.segment_request(i, hour=0) for i in range(len(paths))]
        filt = synth.leaf(synth.NAME, "in", "metric_01", "metric_03")
        for field, agg in [(("dur", "duration"), "sum"), (("size", "datasize"), "max"), (("txt", "number"), "sum"),
                           (("txt", "number"), "min")]:
            req = json.dumps(synth.pushdown(filt, segs, agg, [SVC], field=field))
            try:
                res = eng.eval_pushdown_dist(req, paths, None, 2)
            except Exception as e:   # both ranks' failures in the log (spawn reports only one)
                print(f"rank {rank}: {field} {agg} failed: {e}", flush=True)
                raise
            if rank == 0:
                pr, cells, scale = fr.expected_cells(req, paths, 2, os.path.join(twin_root, f"{field[0]}_{agg}"))
                try:
                    assert len(res) > 0
                    assert_rows_equal(res.rows(), fr.merged_rows(pr, cells, scale, agg), agg, f"dist {field} {agg}")
                    assert res.stats["general_segments"] > 0, res.stats
                except AssertionError as e:
                    print(f"rank 0: {field} {agg} mismatch: {str(e)[:2000]} stats {res.stats}", flush=True)
                    raise
            else:
                assert len(res) == 0
        # a refusal every rank reaches from the request alone: no rank is left in a collective
        from lakeside_amd import LakesideError
        from lakeside_amd._lib import LK_ERR_UNSUPPORTED
        req = json.dumps(synth.pushdown(filt, segs, "avg", [SVC], field=("dur", "duration")))
        with pytest.raises(LakesideError) as e:
            eng.eval_pushdown_dist(req, paths, None, 2)
        assert e.value.code == LK_ERR_UNSUPPORTED
        dist.barrier()
    finally:
        eng.close()
        dist.destroy_process_group()


def test_dist_field_charts_world2(tmp_path):
    import torch.multiprocessing as mp

    from tests.test_gpu_fieldchart import write_files
    paths = write_files(tmp_path, rows=20_000)
    ctx = mp.spawn(_worker, args=(2, _free_port(), paths, str(tmp_path / "twins")), nprocs=2, join=False)
    deadline = time.monotonic() + LIMIT_S
    while not ctx.join(timeout=2):   # raises when a rank failed (and ends the other)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"a rank was still running after {LIMIT_S} s")
