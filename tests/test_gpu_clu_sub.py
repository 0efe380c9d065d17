"""scan_clu's split tiles merged from the clustered copy's sub-block aggregates (`sagg` / `csub`, clu.hpp; built by
clu_build with clu_reduce_pinned) on the MI355X: a split tile's 4,096-row sub-blocks that hold no bucket boundary hand
on their stored (code, sub-block) aggregates, only the sub-blocks that hold one are streamed.

Every case is evaluated three ways, per glob and merged, each against the oracle (tests/parity.py):
  * as it stands;
  * with LK_NO_CLU_SUB=1 (split tiles stream their ranges whole, the path before the sub-block area);
  * with LK_NO_CLUSTER=1 (scan_lean / scan_tiles).
MIN, MAX and sums of integral values are the same rows BIT FOR BIT in the three modes; sums of real values hold the
suite's SUM bar (1 ulp of the correctly rounded value) in each mode -- the double-double partials combine in another
order, so they are not promised bit-equal.

Plan bytes (LK_PLAN_BYTES) are the evidence of the path.  A streamed range of n elements counts the 128-B lines of its
8 n value bytes and 2 n row-index bytes: between 10 n and 10 n + 2 * 254 B.  With the sub-block area a passing code of
a split tile counts the lines of its csub entries (at most 2: up to 68 B), of its sagg entries (nsub * 32 B from a 128-B
aligned start) and of its straddling sub-blocks' elements, so per split tile and passing code with n elements of which
m lie in s straddling sub-blocks:
    plan_bytes  <=  plan_bytes(LK_NO_CLU_SUB=1) - 10 n + 10 m + 508 s + 128 * (2 + ceil(nsub / 4))
(everything else -- descriptors, the boundary search -- is counted alike in both modes)."""
import io
import json

import numpy as np
import pytest

from tests import nonfinite_data as nf
from tests.parity import assert_rows_equal
from tests.test_gpu_clustered import ALL16, NAME, _bits, _cells, _Env, _one, _with, odd_file  # noqa: F401

pytestmark = pytest.mark.gpu

HOUR = 3_600_000
TILE = 1 << 16
SUB = 4096
MODES = (("sub", {}), ("nosub", {"LK_NO_CLU_SUB": 1}), ("off", {"LK_NO_CLUSTER": 1}))


def _three(engine, keys, blobs, segs, filt, agg, gbs=(), glob_size=10, integral=True, label=""):
    """{mode: (per-glob result, merged result)} after the oracle and the cross-mode comparisons."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS, LK_PLAN_BYTES, synth
    from oracle import dataexpr as dx
    req = json.dumps(synth.pushdown(filt, segs, agg, list(gbs)))
    ck = (tuple(keys), json.dumps(filt, sort_keys=True), tuple(gbs), json.dumps(segs, sort_keys=True), glob_size)
    pr = dx.parse_pushdown(req)
    if ck not in _cells:
        _cells[ck] = dx.evaluate_glob_cells(dx.parse_pushdown(req), glob_size, keys, sources=blobs)
    cells = _cells[ck]
    want_pg = [[(c.ts, c.agg_value(agg), c.tags) for c in cs] for cs in cells]
    want_mg = dx.merge_glob_cells(pr, cells)
    out = {}
    for mode, env in MODES:
        with _Env(**env):
            pg = engine.eval_pushdown(req, keys, glob_size, LK_PER_GLOB_ROWS | LK_PLAN_BYTES)
            mg = engine.eval_pushdown(req, keys, glob_size, LK_MERGED | LK_PLAN_BYTES)
        for gi, (g, w) in enumerate(zip(pg.per_glob(len(want_pg)), want_pg)):
            assert_rows_equal(g, w, agg, f"{label} {mode} glob {gi}")
        assert_rows_equal(mg.rows(), want_mg, agg, f"{label} {mode} merged")
        for r in (pg, mg):
            if mode == "off":
                assert r.stats["clustered"] == 0 and r.stats["clustered_tiles"] == 0, r.stats
            else:
                assert r.stats["clustered"] == 1 and r.stats["clustered_tiles"] > 0, (label, mode, r.stats)
        out[mode] = (pg, mg)
    for a, b, c in zip(out["sub"], out["nosub"], out["off"]):
        assert a.ts.tolist() == b.ts.tolist() == c.ts.tolist() and a.tags == b.tags == c.tags, label
        if agg != "sum" or integral:
            assert _bits(a.values) == _bits(b.values), f"{label}: LK_NO_CLU_SUB rows differ"
            assert _bits(a.values) == _bits(c.values), f"{label}: LK_NO_CLUSTER rows differ"
    return out


def _pb(out):
    """Plan bytes of the merged evaluation: (sub-block aggregates, LK_NO_CLU_SUB=1)."""
    return out["sub"][1].stats["plan_bytes"], out["nosub"][1].stats["plan_bytes"]


def _sub_counts(blob):
    """{name: [rows of the name in sub-block j]} of a one-tile file, read back from the Parquet."""
    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    names = np.asarray(pq.read_table(io.BytesIO(blob), columns=[dx.NAME]).column(dx.NAME).to_pylist(), dtype=object)
    nsub = (len(names) + SUB - 1) // SUB
    return {str(p): [int(np.sum(names[j * SUB:(j + 1) * SUB] == p)) for j in range(nsub)] for p in set(names.tolist())}


def _assert_plan_bound(out, counts, passing, straddling, agg, label):
    """The module docstring's bound for an all-split call over one tile whose sub-blocks `straddling` hold a boundary
    (MIN also reads the line of each passing code's NaN bits)."""
    a, b = _pb(out)
    bound = b
    for p in passing:
        per = counts[p]
        m = [per[j] for j in straddling if per[j]]
        bound += -10 * sum(per) + 10 * sum(m) + 508 * len(m) + 128 * (2 + (len(per) + 3) // 4) + (128 if agg == "min" else 0)
    assert a <= bound and a < b, (label, passing, a, b, bound)


FILTERS = [("eq", lambda s: s.leaf(NAME, "eq", "metric_07"), ()),
           ("in3", lambda s: s.leaf(NAME, "in", "metric_03", "metric_07", "metric_11"), (NAME,)),
           ("all16", lambda s: s.leaf(NAME, "in", *ALL16), (NAME,))]


@pytest.mark.parametrize("step", [600_000, 300_000])
@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_split_tiles_integral(engine, agg, step):
    """2^19 rows in 65,536-row pages: tiles of up to 7.5 min and 16 sub-blocks; a 10 min step gives one boundary in a
    split tile, a 5 min step one or two.  Split and pinned tiles share the call; the split ones read fewer bytes."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    for name, filt, gbs in FILTERS:
        out = _three(engine, keys, blobs, _with(segs, step), filt(synth), agg, gbs, label=f"int {name} {agg} {step}")
        st = out["sub"][1].stats
        assert st["clustered_tiles"] == st["tiles"] >= 8, st
        a, b = _pb(out)
        assert 0 < b - a, (name, agg, step, a, b)


@pytest.mark.parametrize("step", [600_000, 300_000])
def test_split_tiles_real_and_compensated_integers(engine, step):
    """value_mode=1 (lognormal reals: every add compensated), then the integral data under LK_NO_EXACT_SUM=1 (the
    compensated form of the same sums: exact, so still bit for bit)."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 2, rows=1 << 19, value_mode=1, page_rows=TILE)
    for agg in ("sum", "min", "max"):
        for name, filt, gbs in FILTERS:
            out = _three(engine, keys, blobs, _with(segs, step), filt(synth), agg, gbs, integral=False,
                         label=f"real {name} {agg} {step}")
            assert out["sub"][1].stats["exact_sum"] == 0
            a, b = _pb(out)
            assert 0 < b - a
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    with _Env(LK_NO_EXACT_SUM=1):
        for name, filt, gbs in FILTERS:
            out = _three(engine, keys, blobs, _with(segs, step), filt(synth), "sum", gbs, label=f"no exact sum {name} {step}")
            assert out["sub"][1].stats["exact_sum"] == 0
            a, b = _pb(out)
            assert 0 < b - a


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_window_cuts_first_and_last_tile(engine, agg):
    """The window cut 7 s / 11 s inside the hour: the end tiles' rows outside it (classes 0 and nsb) are dropped, from
    whole sub-blocks as well as from streamed ones -- at a 10 min step, and at 1 h, where the end tiles are the only
    split ones and nearly all their sub-blocks are whole."""
    from lakeside_amd import synth
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    for step in (600_000, HOUR):
        full = _three(engine, keys, blobs, _with(segs, step), synth.leaf(NAME, "in", "metric_07", "metric_08"), agg, [NAME],
                      label=f"whole window {agg} {step}")
        out = _three(engine, keys, blobs, _with(segs, step, (7000, 11000)), synth.leaf(NAME, "in", "metric_07", "metric_08"),
                     agg, [NAME], label=f"cut window {agg} {step}")
        a, b = _pb(out)
        assert 0 < b - a
        if agg == "sum":   # the cut did drop rows of the end tiles
            assert _bits(full["sub"][1].values) != _bits(out["sub"][1].values)


def test_all_pinned_and_no_copy_are_unchanged(engine):
    """A call whose tiles are all pinned (1 h step on the hour) counts the same bytes with and without the switch; on a
    segment loaded with {"cluster_values": false} the switch changes nothing."""
    from lakeside_amd import LK_MERGED, LK_PLAN_BYTES, synth
    from lakeside_amd.evaluator import Engine
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    out = _three(engine, keys, blobs, _with(segs, HOUR), synth.leaf(NAME, "in", "metric_02", "metric_07"), "sum", [NAME],
                 label="all pinned")
    a, b = _pb(out)
    assert a == b
    req = json.dumps(synth.pushdown(synth.leaf(NAME, "in", "metric_02", "metric_07"), _with(segs, 600_000), "sum", [NAME]))
    on = engine.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES)
    eng = Engine(0, cluster_values=False)
    try:
        eng.put_segment(keys[0], blobs[0])
        assert eng.stats["clu_bytes"] == 0 and eng.stats["clu_sub_bytes"] == 0
        res = []
        for env in ({}, {"LK_NO_CLU_SUB": 1}):
            with _Env(**env):
                res.append(eng.eval_pushdown(req, keys, 10, LK_MERGED | LK_PLAN_BYTES))
        for off in res:
            assert off.stats["clustered"] == 0 and off.stats["clustered_tiles"] == 0
            assert off.ts.tolist() == on.ts.tolist() and off.tags == on.tags and _bits(off.values) == _bits(on.values)
        assert res[0].stats["plan_bytes"] == res[1].stats["plan_bytes"]
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------
# Crafted one-tile files (pyarrow: one row group, one page)
# ---------------------------------------------------------------------------------------------------------------
CRAFT_ROWS = 3 * SUB + 37
CRAFT_STEP = 600_000
CRAFT_CUT = 10_000   # the second boundary's row: the middle of the third sub-block


def _write_one_tile(path, ts, names, val):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    t = pa.table({dx.TIMESTAMP: pa.array(ts, pa.int64()), dx.VALUE: pa.array(val, pa.float64()),
                  dx.NAME: pa.array(list(names), pa.string())})
    pq.write_table(t, path, compression="NONE", use_dictionary=[dx.NAME], row_group_size=len(ts), data_page_size=1 << 22,
                   column_encoding={dx.TIMESTAMP: "PLAIN", dx.VALUE: "PLAIN"})
    with open(path, "rb") as f:
        return f.read()


def _crafted_ts(rng, n, cuts):
    """Sorted timestamps of one tile shorter than two steps that meets three buckets: rows [0, cuts[0]) in the last 10 s
    of bucket 0, rows [cuts[0], cuts[1]) over bucket 1, the rest in the first 5 s of bucket 2."""
    from lakeside_amd import synth
    a = np.sort(rng.integers(CRAFT_STEP - 10_000, CRAFT_STEP, cuts[0]))
    b = np.sort(rng.integers(CRAFT_STEP, 2 * CRAFT_STEP, cuts[1] - cuts[0]))
    b[0] = CRAFT_STEP
    c = np.sort(rng.integers(2 * CRAFT_STEP, 2 * CRAFT_STEP + 5_000, n - cuts[1]))
    return synth.T0 + np.concatenate([a, b, c])


@pytest.fixture(scope="module")
def crafted(engine, tmp_path_factory):
    """3 x 4,096 + 37 rows in one tile: a bucket boundary exactly on row 4,096 (the second sub-block stays whole),
    another on row 10,000 in the middle of the third, `gap` absent from the second sub-block, which `fill` fills alone,
    and a short last sub-block of 37 rows.  {"int" | "real": (path, blob, names)}."""
    root = tmp_path_factory.mktemp("clu_sub")
    out = {}
    for kind in ("int", "real"):
        rng = np.random.default_rng(4096 + len(kind))
        ts = _crafted_ts(rng, CRAFT_ROWS, (SUB, CRAFT_CUT))
        names = rng.choice(["a", "b", "gap"], CRAFT_ROWS).astype(object)
        names[rng.choice(SUB, 40, replace=False)] = "fill"
        names[SUB:2 * SUB] = "fill"
        val = rng.integers(-500, 500, CRAFT_ROWS).astype(np.float64) if kind == "int" else rng.lognormal(0.0, 2.0, CRAFT_ROWS)
        path = str(root / f"crafted_{kind}.parquet")
        blob = _write_one_tile(path, ts, names, val)
        engine.load_segment(path)
        out[kind] = (path, blob, names)
    return out


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_crafted_tile(engine, crafted, agg, kind):
    from lakeside_amd import synth
    path, blob, names = crafted[kind]
    segs = [synth.segment_request(0, step=CRAFT_STEP, hour=0)]
    for passing in (["gap"], ["fill"], ["a", "gap", "fill"], ["a", "b", "gap", "fill"]):
        out = _three(engine, [path], [blob], segs, synth.leaf(NAME, "in", *passing), agg, [NAME], integral=kind == "int",
                     label=f"crafted {kind} {passing} {agg}")
        st = out["sub"][1].stats
        assert st["tiles"] == st["clustered_tiles"] == 1, st
        assert len({r[0] for r in out["sub"][1].rows()}) == (2 if passing == ["fill"] else 3)   # `fill` ends in bucket 1
        # the docstring's bound: one split tile, four sub-blocks, the third one straddling
        _assert_plan_bound(out, _sub_counts(blob), passing, [2], agg, f"crafted {kind}")


NF_SUBS = 4


@pytest.fixture(scope="module")
def nonfinite_tile(engine, tmp_path_factory):
    """tests/nonfinite_data.py's kinds of values over four sub-blocks of one split tile (sub-block j holds file j % 3's
    rows): one bucket boundary on row 4,096 and one in the middle of the third sub-block, so every kind lies in whole
    sub-blocks and in the straddler.  `naninf` keeps its NaNs in the last sub-block only (a whole one, bit 3 of the
    code's stored mask): elsewhere they are +inf, so no streamed element and no stored extreme is a NaN."""
    kinds, vals = [], []
    for j in range(NF_SUBS):
        _, kind, val, _, _, _ = nf._columns(j % nf.NFILES, np.random.default_rng(7100 + j), False)
        if j != NF_SUBS - 1:
            val = np.where((kind == "naninf") & np.isnan(val), np.inf, val)
        # `zmix` with one sign, as every cell of nonfinite_data's own files has: +0.0 == -0.0, so which of the two a
        # cell's MIN / MAX returns is not defined (`negz` keeps the -0.0 case)
        val = np.where(kind == "zmix", 0.0, val)
        kinds.append(kind)
        vals.append(val)
    names, val = np.concatenate(kinds), np.concatenate(vals)
    ts = _crafted_ts(np.random.default_rng(7099), len(val), (SUB, CRAFT_CUT))
    path = str(tmp_path_factory.mktemp("clu_sub_nf") / "nf_tile.parquet")
    blob = _write_one_tile(path, ts, names, val)
    engine.load_segment(path)
    return path, blob, names, val


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_nonfinite_over_sub_blocks(engine, nonfinite_tile, agg):
    from lakeside_amd import synth
    path, blob, names, val = nonfinite_tile
    last = (NF_SUBS - 1) * SUB
    assert np.isnan(val[last:][names[last:] == "naninf"]).any() and not np.isnan(val[:last]).any()
    segs = [synth.segment_request(0, step=CRAFT_STEP, hour=0)]
    out = _three(engine, [path], [blob], segs, nf.all_names(), agg, [NAME], integral=False, label=f"nonfinite sub {agg}")
    st = out["sub"][1].stats
    assert st["tiles"] == st["clustered_tiles"] == 1, st
    _assert_plan_bound(out, _sub_counts(blob), sorted(nf.KINDS), [2], agg, "nonfinite tile")
    # A merged MIN that met a NaN is evaluated again with its cells kept per glob (stats `redo` = 2).  Here the only
    # NaNs lie in a whole sub-block, beside finite values of the same code, so nothing but the stored per-code mask
    # (bit 3) can raise the flag on the sub-block path; LK_NO_CLU_SUB=1 streams them and sees them itself.
    for mode in ("sub", "nosub"):
        assert out[mode][1].stats.get("redo", 0) == (2 if agg == "min" else 0), (mode, out[mode][1].stats)

    def classes(rows):
        zero = ("-0", "+0")
        return sorted((t, tags.get("name"), "0" if agg == "sum" and nf.value_class(v) in zero else nf.value_class(v))
                      for t, v, tags in rows)
    want = classes(out["off"][1].rows())
    for mode in ("sub", "nosub"):
        assert classes(out[mode][1].rows()) == want, mode
    rows = {(tags.get("name"), t): v for t, v, tags in out["sub"][1].rows()}
    end = max(t for _, t in rows)
    if agg in ("min", "max"):
        # the oracle's rows (checked in _three): NaN is the greatest value, so MIN skips the last bucket's NaNs and MAX
        # returns them
        assert (rows[("naninf", end)] != rows[("naninf", end)]) == (agg == "max")
        assert _bits([v for _, v in sorted(rows.items())]) == _bits([v for _, v in sorted(
            {(tags.get("name"), t): v for t, v, tags in out["nosub"][1].rows()}.items())])


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_odd_file_minute_step(engine, odd_file, agg):
    """tests/test_gpu_clustered.py's odd file at the 1 m step: short tiles (one sub-block each), single-code tiles, a
    name present in one tile only."""
    from lakeside_amd import synth
    path, blob = odd_file
    segs = [synth.segment_request(0, step=60_000, hour=0)]
    for names in (["rare"], ["solo"], ["rare", "solo", "a", "b"]):
        out = _three(engine, [path], [blob], segs, synth.leaf(NAME, "in", *names), agg, [NAME], label=f"odd {names} {agg}")
        assert out["sub"][1].stats["tiles"] >= 8
        a, b = _pb(out)
        assert a <= b + 128 * 3 * len(names) * out["sub"][1].stats["tiles"]   # one-sub-block tiles stream what they streamed


def test_engine_clu_sub_bytes(tmp_path_factory):
    """A file of tests/nonfinite_data.py is one tile with a 12-name dictionary: its sub-block area is one stride of
    clu_sub_bytes(12) (the layout of csrc/clu.hpp in Python integers, as tests/test_clu_sub_cpu.py pins the function);
    `clu_bytes` is what it was and `segment_bytes` covers both."""
    from lakeside_amd.evaluator import Engine

    def align(x, a):
        return (x + a - 1) // a * a
    paths, blobs = nf.write_files(tmp_path_factory.mktemp("clu_sub_size"), "clean")
    d = len(nf.KINDS)
    sub = align(d * 16 * 32 + d * 17 * 4 + d * 2, 128)
    blk = align(1 * 16, 128) + align(288 + 32 * d + 10 * nf.ROWS, 128)
    eng = Engine(0)
    try:
        for i, p in enumerate(paths):
            eng.load_segment(p)
            assert eng.stats["clu_sub_bytes"] == (i + 1) * sub and eng.stats["clu_bytes"] == (i + 1) * blk, (i, eng.stats)
        with_copy = eng.segment_bytes
        assert with_copy >= eng.stats["clu_bytes"] + eng.stats["clu_sub_bytes"] + sum(len(b) for b in blobs)
    finally:
        eng.close()
    # the same files without the copy weigh their streams and tables alone: the difference is both areas, exactly
    eng = Engine(0, cluster_values=False)
    try:
        for p in paths:
            eng.load_segment(p)
        assert eng.stats["clu_bytes"] == 0 and eng.stats["clu_sub_bytes"] == 0
        assert with_copy - eng.segment_bytes == len(paths) * (blk + sub), (with_copy, eng.segment_bytes, blk, sub)
    finally:
        eng.close()


@pytest.mark.timeout(120)
def test_distributed_world1_loopback(engine):
    from lakeside_amd import synth
    from lakeside_amd.evaluator import Engine
    from oracle import dataexpr as dx
    keys, blobs, segs = _one(engine, 0, rows=1 << 19, page_rows=TILE)
    segs = _with(segs, 600_000)
    req = json.dumps(synth.pushdown(synth.leaf(NAME, "in", "metric_07", "metric_09"), segs, "sum", [NAME]))
    pr = dx.parse_pushdown(req)
    want = dx.merge_glob_cells(pr, dx.evaluate_glob_cells(pr, 10, keys, sources=blobs))
    with _Env(LK_COMM_LOOPBACK=1):
        eng = Engine(0)
        try:
            eng.comm_init(Engine.unique_id(), 1, 0)
            eng.put_segment(keys[0], blobs[0])
            res = eng.eval_pushdown_dist(req, keys, None, 10)
            with _Env(LK_NO_CLU_SUB=1):
                ref = eng.eval_pushdown_dist(req, keys, None, 10)
            for r in (res, ref):
                assert r.stats["clustered"] == 1, r.stats
                assert_rows_equal(r.rows(), want, "sum", "dist loopback")
            assert res.ts.tolist() == ref.ts.tolist() and res.tags == ref.tags and _bits(res.values) == _bits(ref.values)
        finally:
            eng.close()
