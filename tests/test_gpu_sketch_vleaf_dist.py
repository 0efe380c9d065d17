"""`p<NN>` and `ces` charts with numeric comparison leaves on the value column through the distributed path (host
transport, world 2; files: tests/vleaf_data.py): rank 0's merged rows equal the single-GPU call's, and a shape that stays
refused fails on both ranks -- before the first collective (a mixed conjunct: the gate reads the request alone), or after
the glob agreement (a groupBy the files store as a number) -- without a hang."""
import os

import pytest

from tests import vleaf_data as vd

pytestmark = pytest.mark.gpu

KINDS = ["lean", "int64", "nulls", "names70"]


def _keyed(res, agg):
    """Rows by (timestamp, tags) -- their order within a timestamp is not part of the contract: value bits, sketch."""
    import numpy as np
    bits = np.asarray(res.values).view(np.uint64).tolist()
    rows = {(int(res.ts[r]), tuple(sorted(res.tags[r].items()))): (bits[r], res.sketch(r) if agg[0] == "p" else None)
            for r in range(len(res))}
    assert len(rows) == len(res)
    return rows


def _worker(rank, world, port, paths):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    from lakeside_amd import LK_MERGED, _lib, synth
    from lakeside_amd.evaluator import Engine
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = Engine(0)
    try:
        eng.comm_init_host(world, rank)
        leaf = vd.and_all([vd.name_filter("dense")] + vd.VALUE_FILTERS["between"])
        for agg, gbs in (("p50", [vd.SVC]), ("ces", [vd.SVC])):
            req = vd.request(leaf, agg, gbs, len(paths))
            try:
                res = eng.eval_pushdown_dist(req, paths, None, vd.GLOB)
            except Exception as e:   # both ranks' failures in the log (spawn reports only one)
                print(f"rank {rank}: {agg} failed: {e}", flush=True)
                raise
            if rank == 0:
                one = eng.eval_pushdown(req, paths, vd.GLOB, LK_MERGED)
                assert res.stats["filter"]["vleaf"] == 1, res.stats
                assert len(res) == len(one) >= 12 and _keyed(res, agg) == _keyed(one, agg), agg
            else:
                assert len(res) == 0
        mixed = vd.and_all([vd.name_filter("sparse"), {"op": "or", "q1": vd.num("gt", "1"),
                                                       "q2": synth.leaf(vd.SVC, "eq", "svc-1")}])
        for filt, gbs in ((mixed, []), (leaf, [vd.NUMCOL])):
            for agg in ("p50", "ces"):
                with pytest.raises(_lib.LakesideError) as ei:
                    eng.eval_pushdown_dist(vd.request(filt, agg, gbs, len(paths)), paths, None, vd.GLOB)
                assert ei.value.code == _lib.LK_ERR_UNSUPPORTED, (rank, agg, ei.value)
                assert "numeric comparison leaves in sketch queries" in str(ei.value), (rank, agg, ei.value)
        dist.barrier()
    finally:
        eng.close()
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_dist_sketch_value_leaves_world2(tmp_path):
    import torch.multiprocessing as mp

    from tests.test_gpu_dist import _free_port
    files = vd.write_files(tmp_path)
    mp.spawn(_worker, args=(2, _free_port(), [files[k] for k in KINDS]), nprocs=2, join=True)
