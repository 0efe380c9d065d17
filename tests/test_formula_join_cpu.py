"""What lk_eval_formula decides without a segment or a device (lakeside_amd/csrc/formula_join.cpp), through
lk_formula_gate_sim and lk_formula_union_sim of liblakeside_text.so: the gate over the request alone (every refusal by
code and named rule, the leaf numbering, the evaluation order, the chart transformer), the union group ids of the table
path and of the identity path, the cell space, and the collapse ranks against the reference's rule -- rows of one
operand that share a key collapse to the row with the smallest sorted (tag name, value) list (tests/formula_ref.py,
`expected`).  The rank property is drawn over ASCII texts only: C++ compares bytes, Python code points."""
import ctypes
import json
import os
import random
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
ARG, UNSUPPORTED = -1, -2
STEP = 60_000
FX_MAXLEAF, FX_MAXCOL = 8, 8                                    # formula_cell.hpp
RANK_ABSENT, NONAME_FIRST, NONAME_LAST = 0xffffffff, 1, 0xfffffffc


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB)
    L.lk_formula_gate_sim.restype = ctypes.c_int
    L.lk_formula_gate_sim.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.lk_formula_union_sim.restype = ctypes.c_int
    L.lk_formula_union_sim.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    return L


def _result(rc, out):
    return (0, json.loads(out.value)) if rc == 0 else (rc, out.value.decode())


def gate(lib, formula, exprs, dist=0, world=1):
    """(0, the gate's outcome) or (status code, message)."""
    call = {"expressions": exprs}
    if formula is not None:
        call["formula"] = formula
    out = ctypes.create_string_buffer(1 << 16)
    return _result(lib.lk_formula_gate_sim(json.dumps(call).encode(), dist, world, out, len(out)), out)


def union(lib, spec):
    out = ctypes.create_string_buffer(1 << 16)
    return _result(lib.lk_formula_union_sim(json.dumps(spec).encode(), out, len(out)), out)


# ---- requests, shaped as tests/test_gpu_formula.py shapes them ----
def all_names():
    from lakeside_amd import synth
    return synth.leaf(synth.NAME, "regex", "^metric_")


def be(filt, agg, gbs=(), chart_type="count", dataset="logs", metric_type=None, field=None):
    e = {"id": "x", "dataset": dataset, "filter": filt,
         "chart": {"aggregation": agg, "groupBys": list(gbs), "type": chart_type}}
    if metric_type is not None:
        e["metricType"] = metric_type
    if field is not None:
        e["chart"]["fieldName"], e["chart"]["fieldType"] = field
    return e


def expressions(bes, dataset="logs"):
    from lakeside_amd import synth
    segs = [synth.segment_request(i, step=STEP, hour=0, dataset=dataset) for i in (0, 1)]
    return {k: {"pushDown": {"baseExpr": bes[k], "segmentRequests": segs, "reverseSort": False, "isTagQuery": False},
                "paths": ["fx/0", "fx/1"]} for k in bes}


@pytest.fixture(scope="module")
def ex():
    from lakeside_amd import synth
    return expressions({"a": be(all_names(), "count", [synth.SERVICE]), "b": be(all_names(), "sum", [synth.SERVICE]),
                        "c": be(all_names(), "sum", [synth.NAMESPACE])})


def refused(lib, formula, exprs, code, word, **kw):
    rc, msg = gate(lib, formula, exprs, **kw)
    assert rc == code, (rc, msg)
    assert word in msg, msg


def test_gate_refusals_of_test_refusals(lib, ex):
    """The request-only cases of tests/test_gpu_formula.py::test_refusals, by code and named rule."""
    from lakeside_amd import synth
    refused(lib, "a / c", ex, UNSUPPORTED, "groupBy")
    exemplar = json.loads(json.dumps(ex))
    del exemplar["b"]["pushDown"]["baseExpr"]["chart"]
    refused(lib, "a / b", exemplar, UNSUPPORTED, "chart")
    tagq = json.loads(json.dumps(exemplar))
    tagq["b"]["pushDown"]["isTagQuery"] = True
    tagq["b"]["pushDown"]["tagDataType"] = {"tagName": synth.SERVICE, "dataType": "string"}
    refused(lib, "a / b", tagq, UNSUPPORTED, "tag query")
    steps = json.loads(json.dumps(ex))
    for s in steps["b"]["pushDown"]["segmentRequests"]:
        s["stepInMillis"] = 10_000
    refused(lib, "a / b", steps, ARG, "step")
    refused(lib, "a ^ 2", ex, UNSUPPORTED, "'^'")
    refused(lib, "a / total", ex, ARG, "total")
    # an unreferenced expression is not read: b's other step, and a b that is no request at all
    rc, got = gate(lib, "a + 0", steps)
    assert rc == 0 and [o["var"] for o in got["operands"]] == ["a"]
    rc, got = gate(lib, "a + 0", dict(ex, b={"pushDown": 7}))
    assert rc == 0 and [o["var"] for o in got["operands"]] == ["a"]
    rc, got = gate(lib, "5 + 3", ex)
    assert rc == 0 and got["operands"] == [] and got["order"] == []


def test_gate_refusals_no_gpu_test_reaches(lib, ex):
    from lakeside_amd import synth
    rc, msg = gate(lib, None, ex)
    assert rc == ARG and '"formula"' in msg
    out = ctypes.create_string_buffer(4096)
    rc = lib.lk_formula_gate_sim(json.dumps({"formula": "a + 0"}).encode(), 0, 1, out, len(out))
    assert rc == ARG and '"expressions"' in out.value.decode()
    refused(lib, "a + 0", dict(ex, a={"paths": ["fx/0", "fx/1"]}), ARG, "pushDown")
    short = json.loads(json.dumps(ex))
    short["a"]["paths"] = ["fx/0"]
    refused(lib, "a + 0", short, ARG, "paths must match")
    for key in ("extract", "compute"):
        x = json.loads(json.dumps(ex))
        x["a"]["pushDown"]["baseExpr"][key] = {"regex": "x"}
        refused(lib, "a + 0", x, UNSUPPORTED, "extract / compute")
    pct = expressions({"a": be(all_names(), "p95", [synth.SERVICE], dataset="metrics")}, dataset="metrics")
    refused(lib, "a + 0", pct, UNSUPPORTED, "metrics percentiles")
    rc, got = gate(lib, "a + 0", expressions({"a": be(all_names(), "p95", field=("lat", "number"), dataset="metrics")},
                                             dataset="metrics"))
    assert rc == 0 and got["operands"][0]["uploaded"] is True   # a field chart's percentile: evaluated, then uploaded
    for bad in (0, -STEP):
        x = json.loads(json.dumps(ex))
        x["a"]["pushDown"]["segmentRequests"][1]["stepInMillis"] = bad
        refused(lib, "a + 0", x, ARG, "stepInMillis must be positive")
    names = "abcdefghi"
    many = expressions({v: be(all_names(), "sum") for v in names})
    refused(lib, " + ".join(names), many, UNSUPPORTED, f"more than {FX_MAXLEAF} expressions")
    assert gate(lib, " + ".join(names[:FX_MAXLEAF]), many)[0] == 0
    cols = [f"g{i}" for i in range(FX_MAXCOL + 1)]
    refused(lib, "a + 0", expressions({"a": be(all_names(), "sum", cols)}), UNSUPPORTED, f"more than {FX_MAXCOL} groupBy")
    assert gate(lib, "a + 0", expressions({"a": be(all_names(), "sum", cols[:FX_MAXCOL])}))[0] == 0
    refused(lib, "a + 0", expressions({"a": be(all_names(), "sum", chart_type="gauge")}), ARG, "unknown chart type gauge")
    refused(lib, "a + 0", expressions({"a": be(all_names(), "sum", metric_type="timer")}), ARG, "unknown metric type timer")


def test_gate_shard(lib, ex):
    """The shard check of a distributed call; a local call does not read the key."""
    def with_shard(sh):
        x = json.loads(json.dumps(ex))
        x["a"]["shard"] = sh
        return x
    refused(lib, "a / b", with_shard([0, 1, 2]), ARG, "one rank per path", dist=1, world=3)
    refused(lib, "a / b", with_shard([0]), ARG, "one rank per path", dist=1, world=3)
    refused(lib, "a / b", with_shard([0, 3]), ARG, "shard rank 3 outside", dist=1, world=3)
    refused(lib, "a / b", with_shard([-1, 0]), ARG, "shard rank -1 outside", dist=1, world=3)
    refused(lib, "a / b", with_shard([0, 1]), ARG, "shard rank 1 outside", dist=1, world=1)
    rc, got = gate(lib, "a / b", with_shard(None), dist=1, world=3)
    assert rc == 0 and got["operands"][0]["shard"] == []
    rc, got = gate(lib, "a / b", with_shard([2, 0]), dist=1, world=3)
    assert rc == 0 and [o["shard"] for o in got["operands"]] == [[2, 0], []]
    for sh in ([0, 3], [0], "x"):
        rc, got = gate(lib, "a / b", with_shard(sh), dist=0, world=1)
        assert rc == 0 and got["operands"][0]["shard"] == []


def test_gate_outcome(lib):
    """Leaf numbers follow `expressions`, the evaluation order the names' bytes; key columns, step, paths."""
    from lakeside_amd import synth
    bes = {"b": be(all_names(), "sum", [synth.SERVICE, synth.NAMESPACE, synth.SERVICE]),
           "a": be(all_names(), "ces", [synth.NAMESPACE, synth.SERVICE]),
           "unused": be(all_names(), "sum")}
    rc, got = gate(lib, "a / b", expressions(bes))
    assert rc == 0
    assert got["program"].split() == ["$1", "$0", "/"]
    assert [o["var"] for o in got["operands"]] == ["b", "a"] and got["order"] == ["a", "b"]
    assert [o["uploaded"] for o in got["operands"]] == [False, True]
    assert got["key_cols"] == sorted([synth.NAMESPACE, synth.SERVICE])
    assert got["step"] == STEP and got["secs"] == 60
    assert all(o["paths"] == ["fx/0", "fx/1"] for o in got["operands"])
    rc, got = gate(lib, "Z + a", expressions({"a": bes["unused"], "Z": bes["unused"]}))
    assert rc == 0 and got["order"] == ["Z", "a"] and got["program"].split() == ["$1", "$0", "+"]


def test_gate_transformer(lib):
    def xform(**kw):
        ds = kw.get("dataset", "logs")
        rc, got = gate(lib, "a + 0", expressions({"a": be(all_names(), "sum", **kw)}, dataset=ds))
        assert rc == 0, got
        return got["operands"][0]["xform"]
    assert xform(chart_type="rate") == "div"
    assert xform(chart_type=" Rate ") == "div"
    assert xform(chart_type="count") == "none"
    assert xform(chart_type="rate", metric_type="rate") == "div"                 # logs: the chart type alone
    assert xform(dataset="metrics", chart_type="count", metric_type="rate") == "mul"
    assert xform(dataset="metrics", chart_type="rate", metric_type="counter") == "div"
    assert xform(dataset="metrics", chart_type="rate", metric_type="count") == "div"   # "count" reads as counter
    for ct, mt in (("count", "counter"), ("count", "gauge"), ("count", None), ("rate", "rate"), ("rate", "gauge"),
                   ("rate", "histogram"), ("rate", None)):
        assert xform(dataset="metrics", chart_type=ct, metric_type=mt) == "none", (ct, mt)


# ---- union group space ----
def dim(tag, dims):
    return {"tag": tag, "dims": dims}


NO_NAME = dim("name", [])


def test_union_ids_table_path(lib):
    k1 = [["x", None, "", "y"], ["y", "z", None]]
    k2 = [["p", "q"], ["q", None, "r", "only-1"]]
    qt = [[["k1", "y"], ["k2", "qt-only"], ["zone", "w"]], [["zone", "w"]]]
    spec = {"key_cols": ["k1", "k2"],
            "operands": [{"name": NO_NAME, "keys": [dim("k1", k1[k]), dim("k2", k2[k])], "query_tags": qt[k]}
                         for k in range(2)]}
    rc, got = union(lib, spec)
    assert rc == 0, got
    sizes = []
    for j, col in enumerate((k1, k2)):
        ids = {}
        for k in range(2):
            m = got["operands"][k]["maps"][j]
            assert len(m) == len(col[k])
            for text, u in zip(col[k], m):
                if not text:
                    assert u == 0                                 # null and "" are absent
                else:
                    assert u >= 1 and ids.setdefault(text, u) == u   # equal texts, equal ids across operands
        for k in range(2):
            v = dict(map(tuple, qt[k])).get(spec["key_cols"][j], "")
            u = got["operands"][k]["qt_ids"][j]
            assert (u == 0) if not v else (ids.setdefault(v, u) == u)
        assert len(set(ids.values())) == len(ids)                # distinct texts, distinct ids
        assert sorted(ids.values()) == list(range(1, len(ids) + 1))
        sizes.append(len(ids) + 1)
    assert sizes == [4, 6]                               # x y z | p q r only-1 qt-only; + absent
    assert got["ustride"] == [6, 1] and got["U"] == 24
    for o in got["operands"]:
        assert o["qt_u"] == sum(u * s for u, s in zip(o["qt_ids"], got["ustride"]))
    assert got["operands"][0]["qt_u"] != 0 and got["operands"][1]["qt_u"] == 0
    # an expression without rows is absent everywhere and is not read
    rc, got2 = union(lib, dict(spec, operands=[None] + spec["operands"]))
    assert rc == 0 and got2["operands"][1:] == got["operands"] and got2["U"] == got["U"]
    assert got2["operands"][0]["name_rank"] == [] and got2["operands"][0]["qt_u"] == 0


NDIM = 4_000_000_000


def test_union_ids_identity_path(lib):
    """A column every operand reads through one dictionary is not walked, however large: the hook fails a call that asks
    for one of its texts, and the call returns at once."""
    words = {f"v{i}": 7 * i for i in range(9)}
    words["last"] = NDIM - 1                                      # the dictionary's id of dim_null: not a dim of its own
    big = {"tag": "c", "ndim": NDIM}
    qts = ["v3", "new1", "v8", "new2", "new1", "last", ""]
    spec = {"key_cols": ["c"], "ident": [{"ndim": NDIM, "dict": words}],
            "operands": [{"name": NO_NAME, "keys": [big], "query_tags": [["c", v]] if v else []} for v in qts]}
    t0 = time.perf_counter()
    rc, got = union(lib, spec)
    took = time.perf_counter() - t0
    assert rc == 0, got
    assert took < 1.0
    assert [o["qt_ids"][0] for o in got["operands"]] == [7 * 3 + 1, NDIM + 1, 7 * 8 + 1, NDIM + 2, NDIM + 1, NDIM + 3, 0]
    assert all(o["maps"] == [[]] for o in got["operands"])
    assert got["U"] == NDIM + 1 + 3 and got["ustride"] == [1]
    # a column of this kind that is no identity column is walked: the proof above is not vacuous
    small = {"key_cols": ["c"], "operands": [{"name": NO_NAME, "keys": [{"tag": "c", "ndim": 5}], "query_tags": []}]}
    rc, msg = union(lib, small)
    assert rc != 0 and "walked" in msg
    three = {"key_cols": ["c", "d", "e"], "ident": [{"ndim": NDIM, "dict": {}}] * 3,
             "operands": [{"name": NO_NAME, "keys": [dict(big, tag=t) for t in "cde"], "query_tags": []}] * 2}
    rc, msg = union(lib, three)
    assert rc == UNSUPPORTED and "64 bits" in msg


def test_cell_space(lib):
    one = {"key_cols": ["k"], "operands": [{"name": NO_NAME, "keys": [dim("k", ["x", "y"])], "query_tags": []}]}
    for base, last, step in ((0, 0, STEP), (1_700_000_000_000, 1_700_000_000_000 + 10 * STEP, STEP), (5, 5 + 7 * 13, 13)):
        rc, got = union(lib, dict(one, cells={"base": base, "last": last, "step": step}))
        assert rc == 0 and got["nbuckets"] == (last - base) // step + 1 and got["nkeys"] == got["nbuckets"] * got["U"]
    rc, got = union(lib, dict(one, cells={"base": 0, "last": ((1 << 26) - 1) * STEP, "step": STEP}))
    assert rc == 0 and got["nbuckets"] == 1 << 26
    rc, msg = union(lib, dict(one, cells={"base": 0, "last": (1 << 26) * STEP, "step": STEP}))
    assert rc == UNSUPPORTED and "2^26 buckets" in msg
    big = {"key_cols": ["c", "d"], "ident": [{"ndim": NDIM, "dict": {}}] * 2,
           "operands": [{"name": NO_NAME, "keys": [{"tag": "c", "ndim": NDIM}, {"tag": "d", "ndim": NDIM}], "query_tags": []}]}
    rc, got = union(lib, dict(big, cells={"base": 0, "last": 0, "step": STEP}))
    assert rc == 0 and got["U"] == (NDIM + 1) ** 2 and got["nkeys"] == got["U"]
    rc, msg = union(lib, dict(big, cells={"base": 0, "last": STEP, "step": STEP}))   # 2 x 1.6e19 > 2^64
    assert rc == UNSUPPORTED and "cell key" in msg


# ---- collapse ranks ----
def rows_under_query_tags(lib, name_tag, key_tags, texts, qt):
    """The rows of one operand that can meet under the queryTags' key, as (sorted tag list, rank the join gives)."""
    spec = {"key_cols": key_tags,
            "operands": [{"name": dim(name_tag, texts + [None]), "keys": [dim(t, []) for t in key_tags],
                          "query_tags": [list(kv) for kv in qt]}]}
    rc, got = union(lib, spec)
    assert rc == 0, got
    o = got["operands"][0]
    assert o["name_rank"][-1] == RANK_ABSENT
    assert o["after_name"] == sum(1 << j for j, t in enumerate(key_tags) if t > name_tag)
    rest = [(t, dict(qt)[t]) for t in key_tags if t in dict(qt)]
    rows = [(sorted(rest + [(name_tag, text)]), o["name_rank"][d]) for d, text in enumerate(texts)]
    if rest:   # the row without a name tag, ranked as fx_scatter ranks it
        rows.append((sorted(rest), NONAME_LAST if any(t > name_tag for t, _ in rest) else NONAME_FIRST))
    rows.append((sorted(qt), o["qt_rank"]))   # the all-absent row carries the whole queryTags
    return rows, o


def assert_ranks_follow_lists(rows, what):
    for i, (l1, r1) in enumerate(rows):
        for l2, r2 in rows[i + 1:]:
            if l1 != l2:
                assert (r1 < r2) == (l1 < l2), (what, l1, r1, l2, r2)


def test_collapse_ranks_follow_the_sorted_tag_lists(lib):
    rng = random.Random(20240611)
    tags = ["a", "k1", "k2", "m", "name", "z", "zz"]
    values = ["A", "b", "svc", "x", "z"]
    for case in range(2000):
        name_tag = rng.choice(["a", "m", "name", "zz"])
        others = [t for t in tags if t != name_tag]
        key_tags = sorted(rng.sample(others, rng.randint(0, 2)))
        qt = [(t, rng.choice(values)) for t in rng.sample(others, rng.randint(0, 3))]
        texts = rng.sample(values, rng.randint(0, 4))
        rows, _ = rows_under_query_tags(lib, name_tag, key_tags, texts, qt)
        assert_ranks_follow_lists(rows, (case, name_tag, key_tags, texts, qt))


def test_collapse_rank_edges(lib):
    """The all-absent row before the key's row without a name tag (rank 0), and behind it when that row ranks last."""
    rows, o = rows_under_query_tags(lib, "name", ["k1"], ["b", "A"], [("k1", "svc"), ("a", "x")])
    assert o["qt_rank"] == 0 and o["name_rank"] == [6, 4, RANK_ABSENT]
    assert_ranks_follow_lists(rows, "first")
    rows, o = rows_under_query_tags(lib, "a", ["k1"], ["b", "A"], [("z", "x"), ("k1", "svc")])
    assert o["qt_rank"] == NONAME_LAST + 1
    assert_ranks_follow_lists(rows, "last")
    rows, o = rows_under_query_tags(lib, "name", ["k1"], ["b", "A"], [])
    assert o["qt_rank"] == 3 and o["qt_u"] == 0                   # no queryTags: the empty list sorts first
