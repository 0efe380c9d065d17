"""A numeric groupBy through the sharded path (lk_eval_pushdown_dist), world 2 over the host transport on one GPU.  Which
columns are numeric depends on each rank's own segments: only rank 1's shard holds a numeric `status` file, the flag
travels with the glob unions every rank agrees on, and both ranks refuse the call with the same message before any
later collective; a string groupBy on the same communicator then answers."""
import json
import os
import socket
import time

import pytest

pytestmark = pytest.mark.gpu

LIMIT_S = 150   # per process


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, paths, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    from lakeside_amd import LakesideError, synth
    from lakeside_amd._lib import LK_ERR_UNSUPPORTED
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    from tests import numgroup_data as nd
    from tests.parity import assert_rows_equal
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = Engine(0)
    try:
        eng.comm_init_host(world, rank)
        segs = [synth.segment_request(i, hour=0) for i in range(len(paths))]
        filt = synth.leaf(synth.NAME, "in", "metric_00", "metric_02")
        req = json.dumps(synth.pushdown(filt, segs, "sum", [nd.STATUS]))
        with pytest.raises(LakesideError) as e:   # shard: path i on rank i -- the INT64 file is rank 1's alone
            eng.eval_pushdown_dist(req, paths, None, 2)
        assert e.value.code == LK_ERR_UNSUPPORTED, str(e.value)
        assert "numeric groupBy" in str(e.value) and "distributed" in str(e.value)
        with open(os.path.join(out_dir, f"message_{rank}.txt"), "w") as f:
            f.write(str(e.value))
        req = json.dumps(synth.pushdown(filt, segs, "sum", [nd.SVC]))
        res = eng.eval_pushdown_dist(req, paths, None, 2)
        if rank == 0:
            assert_rows_equal(res.rows(), dx.evaluate_merged(dx.parse_pushdown(req), paths, 2), "sum", "dist by service")
        else:
            assert len(res) == 0
        dist.barrier()
    finally:
        eng.close()
        dist.destroy_process_group()


def test_dist_numeric_group_by_refused_on_every_rank(tmp_path):
    import torch.multiprocessing as mp

    from tests import numgroup_data as nd
    paths = [nd.write_file(tmp_path / "text.parquet", "V", seed=41, rows=1500),
             nd.write_file(tmp_path / "int64.parquet", "A", seed=42, rows=1500)]
    ctx = mp.spawn(_worker, args=(2, _free_port(), paths, str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + LIMIT_S
    while not ctx.join(timeout=2):   # raises when a rank failed (and ends the other)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"a rank was still running after {LIMIT_S} s")
    msgs = [open(tmp_path / f"message_{r}.txt").read() for r in range(2)]
    assert msgs[0] == msgs[1] and msgs[0]
