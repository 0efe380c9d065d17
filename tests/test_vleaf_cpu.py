"""Numeric comparison leaves on a chart's value column (lakeside_amd/csrc/vleaf.hpp: vleaf_pass, the rule scan_tiles
applies per passing row in COUNT / p<NN> / ces calls) without a GPU, through lk_vleaf_sim of liblakeside_text.so: the real
shape_leaves, sketch gate, plan_filter and plan_truth, then vleaf_pass over QParams::vl / vtab as setup_scan fills them.

Reference: the oracle's filter evaluation (oracle.dataexpr._eval_filter: Kleene logic over the leaves of BaseExpr.scala:
488-498) of the whole tree on a one-row glob holding the same value, whose string columns make every string conjunct
TRUE -- the whole filter is then TRUE iff the value-leaf conjuncts are.

Trees: seed 23, 40 per leaf count 1..5 (`and` / `or` / `not`; decimal, scientific and duration literals; zero to two
string conjuncts beside them), under `p50`, `ces` and `sum`.  Probes: NULL, NaN, +-0.0, +-inf, the smallest subnormal,
every literal of the tree with its two neighbouring doubles.  Refusals: a mixed conjunct, six value leaves, a leaf on
another column, LK_NO_VLEAF=1, metrics `ces` -- vleaf is 0 and, under `p50` and `ces`, the gate answers its unchanged
text."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import dataexpr as dx
from tests import filter_trees as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
LK_ERR_UNSUPPORTED = -2
REFUSAL = "numeric comparison leaves in sketch queries"
SEED = 23
ROW_NAME, ROW_SVC = "metric_01", "svc-2"     # the probed row's string columns
# (literal, dataType): decimal, scientific, duration (QuantityParser: ns) -- negative, zero, tiny and huge among them
LITERALS = [("250", "number"), ("0.5", "number"), ("-3.25", "number"), ("0", "number"), ("1e3", "number"),
            ("2.5e-3", "number"), ("-1E2", "number"), ("1e300", "number"), ("4.9e-324", "number"),
            ("1.5ms", "duration"), ("250ms", "duration"), ("2s", "duration"), ("750ns", "duration")]
# string conjuncts that are TRUE for the probed row
STRING_TRUE = [ft.and_chain([{"k": ft.NAME, "v": [ROW_NAME], "op": "eq", "extracted": False, "computed": False, "dataType": "string"}]),
               {"not": {"k": ft.SVC, "v": ["svc-0", "svc-9"], "op": "in", "extracted": False, "computed": False, "dataType": "string"}},
               {"op": "or", "q1": {"k": ft.NAME, "v": ["nope"], "op": "eq", "extracted": False, "computed": False, "dataType": "string"},
                "q2": {"k": ft.SVC, "v": ["^svc-[12]$"], "op": "regex", "extracted": False, "computed": False, "dataType": "string"}}]


def value_leaf(rng, col=ft.VALUE):
    lit, dt = LITERALS[int(rng.integers(0, len(LITERALS)))]
    return {"k": col, "v": [lit], "op": ["gt", "ge", "lt", "le"][int(rng.integers(0, 4))], "extracted": False,
            "computed": False, "dataType": dt}


def request(filt, agg, gbs=(), dataset="logs"):
    from lakeside_amd import synth
    d = synth.pushdown(filt, [], "count" if agg == "ces_rollup" else agg, list(gbs), dataset=dataset)
    if agg[0] == "p":
        d["baseExpr"]["chart"]["rollup"] = agg
    if agg == "ces_rollup":
        d["baseExpr"]["chart"]["rollup"] = "ces"
    return json.dumps(d)


def sim(req, valid, vals):
    """(0, vleaf, pass bits) or (error code, message, None)."""
    L = ctypes.CDLL(LIB)
    L.lk_vleaf_sim.restype = ctypes.c_int
    L.lk_vleaf_sim.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    valid = np.ascontiguousarray(valid, np.uint8)
    vals = np.ascontiguousarray(vals, np.float64)
    out = np.full(len(vals), 7, np.uint8)
    vleaf = ctypes.c_int(-1)
    msg = ctypes.create_string_buffer(1024)
    rc = L.lk_vleaf_sim(req.encode(), valid.ctypes.data, vals.ctypes.data, len(vals), ctypes.byref(vleaf), out.ctypes.data,
                        msg, len(msg))
    return (0, vleaf.value, out) if rc == 0 else (rc, msg.value.decode(), None)


def probes(tree):
    """(valid, values): the fixed probes, then every literal of the tree's numeric leaves with its two neighbours."""
    vals = [0.0, float("nan"), 0.0, -0.0, float("inf"), float("-inf"), 5e-324, -5e-324]
    valid = [0] + [1] * (len(vals) - 1)
    for l in ft.leaves_of(tree):
        if l["op"] in dx.NUMERIC_OPS:
            c = dx.normalized_value(dx.handle_filter(l))
            vals += [float(np.nextafter(c, -np.inf)), c, float(np.nextafter(c, np.inf))]
            valid += [1, 1, 1]
    return np.array(valid, np.uint8), np.array(vals, np.float64)


def oracle_pass(req, valid, vals):
    """The whole filter's TRUE mask over one-row-per-probe columns whose strings make every string conjunct TRUE."""
    pr = dx.parse_pushdown(req)
    n = len(vals)
    cols = {ft.NAME: dx._Col(np.zeros(n, np.int64), [ROW_NAME]), ft.SVC: dx._Col(np.zeros(n, np.int64), [ROW_SVC]),
            ft.VALUE: dx._NumCol([float(v) if ok else None for ok, v in zip(valid, vals)], "float")}
    t, _ = dx._eval_filter(pr.baseExpr.filter, cols, set(), n)
    return t


def value_tree(rng, n_val, n_str):
    val = ft._tree(rng, n_val, lambda: value_leaf(rng), 0.3)
    parts, room = [], 6 - n_val          # TT_MAX_LEAVES leaves in all
    for i in rng.permutation(len(STRING_TRUE))[:n_str]:
        if len(ft.leaves_of(STRING_TRUE[int(i)])) <= room:
            parts.append(STRING_TRUE[int(i)])
            room -= len(ft.leaves_of(STRING_TRUE[int(i)]))
    parts.append(val)
    order = rng.permutation(len(parts))
    return ft.and_chain([parts[int(i)] for i in order])


@pytest.mark.parametrize("n_val", [1, 2, 3, 4, 5])
def test_pass_bits_equal_the_oracle(n_val):
    seen = {"pass": 0, "fail": 0, "not": 0, "or": 0, "duration": 0, "sci": 0}
    for i in range(40):
        rng = np.random.default_rng([SEED, n_val, i])
        tree = value_tree(rng, n_val, int(rng.integers(0, 3)))
        text = json.dumps(tree)
        valid, vals = probes(tree)
        for agg in ("p50", "ces", "ces_rollup", "sum"):
            req = request(tree, agg, [ft.SVC] if i % 2 else [])
            rc, vleaf, got = sim(req, valid, vals)
            assert rc == 0 and vleaf == 1, (agg, vleaf, text)
            want = oracle_pass(req, valid, vals)
            assert np.array_equal(got.astype(bool), want), (agg, text, vals[got.astype(bool) != want].tolist())
            assert got[0] == 0                       # NULL: every value leaf UNKNOWN, the conjunct never TRUE
        seen["pass"] += int(got.sum())
        seen["fail"] += int((got == 0).sum())
        seen["not"] += '"not"' in text
        seen["or"] += '"or"' in text
        seen["duration"] += '"duration"' in text
        seen["sci"] += "e" in "".join(l["v"][0].lower() for l in ft.leaves_of(tree) if l["dataType"] == "number")
    assert seen["pass"] > 40 and seen["fail"] > 40 and seen["duration"] >= 5 and seen["sci"] >= 5, seen
    assert seen["not"] >= 5 and (n_val == 1 or seen["or"] >= 5), seen


def test_nan_and_infinities_by_operator():
    """NaN is DuckDB's greatest value: gt / ge keep it, lt / le drop it; +-inf compare as numbers."""
    valid = np.ones(3, np.uint8)
    vals = np.array([float("nan"), float("inf"), float("-inf")])
    for op, want in (("gt", [1, 1, 0]), ("ge", [1, 1, 0]), ("lt", [0, 0, 1]), ("le", [0, 0, 1])):
        leaf = {"k": ft.VALUE, "v": ["1e300"], "op": op, "extracted": False, "computed": False, "dataType": "number"}
        rc, vleaf, got = sim(request(leaf, "p99"), valid, vals)
        assert (rc, vleaf, got.tolist()) == (0, 1, want), op
        rc, vleaf, got = sim(request({"not": leaf}, "p99"), valid, vals)
        assert (rc, vleaf, got.tolist()) == (0, 1, [1 - w for w in want]), op


def _refused_shapes():
    rng = np.random.default_rng([SEED, 99])
    name = STRING_TRUE[0]
    v = lambda: value_leaf(rng)   # noqa: E731
    return {
        "mixed conjunct": ft.and_chain([name, {"op": "or", "q1": v(), "q2": STRING_TRUE[1]}]),
        "six value leaves": ft.and_chain([v() for _ in range(6)]),
        "seven leaves in all": ft.and_chain([name, STRING_TRUE[1], STRING_TRUE[2], v(), v(), v()]),
        "another column": ft.and_chain([name, value_leaf(rng, ft.DUR)]),
        "value and another column": ft.and_chain([name, v(), value_leaf(rng, ft.RATIO)]),
    }


@pytest.mark.parametrize("shape", list(_refused_shapes()))
def test_refused_shapes(shape):
    tree = _refused_shapes()[shape]
    valid, vals = probes(tree)
    for agg in ("p50", "ces", "ces_rollup"):
        rc, msg, _ = sim(request(tree, agg), valid, vals)
        assert rc == LK_ERR_UNSUPPORTED and msg == REFUSAL, (shape, agg, rc, msg)
    rc, vleaf, got = sim(request(tree, "sum"), valid, vals)   # other aggregations plan it (the row scan takes it)
    assert rc == 0 and vleaf == 0 and not got.any(), (shape, rc, vleaf)


def test_refused_by_switch_and_dataset(monkeypatch):
    tree = ft.and_chain([STRING_TRUE[0], {"k": ft.VALUE, "v": ["250"], "op": "gt", "extracted": False, "computed": False,
                                          "dataType": "number"}])
    valid, vals = probes(tree)
    assert sim(request(tree, "p50"), valid, vals)[:2] == (0, 1)
    # metrics `ces` binds no value column (BaseExpr.scala:385-388): refused, whatever the leaf's column
    rc, msg, _ = sim(request(tree, "ces", dataset="metrics"), valid, vals)
    assert rc == LK_ERR_UNSUPPORTED and msg == REFUSAL, (rc, msg)
    monkeypatch.setenv("LK_NO_VLEAF", "1")
    for agg in ("p50", "ces"):
        rc, msg, _ = sim(request(tree, agg), valid, vals)
        assert rc == LK_ERR_UNSUPPORTED and msg == REFUSAL, (agg, rc, msg)
    assert sim(request(tree, "sum"), valid, vals)[:2] == (0, 0)


def test_leaf_free_requests_pass_the_gate():
    for agg in ("p50", "ces", "sum"):
        rc, vleaf, got = sim(request(STRING_TRUE[0], agg), np.ones(2, np.uint8), np.array([1.0, 2.0]))
        assert rc == 0 and vleaf == 0 and not got.any(), agg
