"""The host filter planning (lakeside_amd/csrc/filter_plan.cpp: leaf numbering, the postfix Kleene program, the truth
tables of plan_truth, the early / late split, the value-leaf table, the device column order) without a GPU, through
lk_filter_plan_sim of liblakeside_text.so, against a recursive Kleene evaluator over {T, F, U} written here.

Trees: tests/filter_trees.py, seed 17.  Tables: 6 strata x 50 trees + 60 split-reason trees = 360 trees of <= 6 leaves,
every assignment of {T, F, U} to their leaves (exists leaves never U).  Programs: 48 trees of 7..32 leaves + 6 right-deep
chains, 200 sampled assignments each.  Refusals: 6 cases."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import filter_trees as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
NUMERIC_OPS = ("gt", "ge", "lt", "le")
OP_AND, OP_OR, OP_NOT, OP_TRUE = 0x80, 0x81, 0x82, 0x83   # layout.hpp
MAXPROG = 96
LK_ERR_UNSUPPORTED = -2
GBS = [[], [ft.SVC], [ft.NAME, ft.NS]]
TRUE = {"op": "true"}   # the empty conjunction


def plan(filt, gbs=(), numeric_gbs=()):
    """(0, plan dict) or (error code, message)."""
    from lakeside_amd import synth
    L = ctypes.CDLL(LIB)
    L.lk_filter_plan_sim.restype = ctypes.c_int
    L.lk_filter_plan_sim.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_char_p,
                                     ctypes.c_size_t]
    req = json.dumps(synth.pushdown(filt, [], "sum", list(gbs))).encode()
    arr = (ctypes.c_char_p * max(1, len(numeric_gbs)))(*[g.encode() for g in numeric_gbs])
    out = ctypes.create_string_buffer(1 << 16)
    rc = L.lk_filter_plan_sim(req, arr, len(numeric_gbs), out, len(out))
    return (0, json.loads(out.value)) if rc == 0 else (rc, out.value.decode())


# ---- the reference: Kleene logic over (is_true, is_false) arrays, one entry per assignment ----
def kleene(q, val):
    if q is TRUE:
        n = len(next(iter(val.values()))[0])
        return np.ones(n, bool), np.zeros(n, bool)
    if "not" in q:
        t, f = kleene(q["not"], val)
        return f, t
    if "k" in q:
        return val[id(q)]
    (t1, f1), (t2, f2) = kleene(q["q1"], val), kleene(q["q2"], val)
    return (t1 & t2, f1 | f2) if q["op"] == "and" else (t1 | t2, f1 & f2)


def conjuncts(q):
    if "not" not in q and "k" not in q and q["op"] == "and":
        return conjuncts(q["q1"]) + conjuncts(q["q2"])
    return [q]


def conj_of(parts):
    return ft.and_chain(parts) if parts else TRUE


def is_num(l):
    return l["op"] in NUMERIC_OPS


def numbering(tree, gbs):
    """The documented leaf numbering: string columns = name, then leaf keys in tree order, then groupBys; string leaves
    column by column in tree order, then the numeric leaves in tree order.  -> (cols, [leaf dict by index])"""
    ls = ft.leaves_of(tree)
    cols = [ft.NAME]
    for c in [l["k"] for l in ls if not is_num(l)] + list(gbs):
        if c not in cols:
            cols.append(c)
    order = [l for c in cols for l in ls if not is_num(l) and l["k"] == c] + [l for l in ls if is_num(l)]
    return cols, order


def bits(words, L):
    w = np.array([int(x, 16) for x in words], dtype="<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)[:max(32, 1 << (2 * L))]


def assignments(order, rng=None, samples=None):
    """A[n, L] in {0: T, 1: F, 2: U}: every assignment (or `samples` random ones); exists leaves never U."""
    L = len(order)
    if samples is None:
        A = np.stack(np.meshgrid(*[np.arange(3)] * L, indexing="ij"), -1).reshape(-1, L) if L else np.zeros((1, 0), int)
    else:
        A = rng.integers(0, 3, (samples, L))
    for j, l in enumerate(order):
        if l["op"] == "exists":
            A = A[A[:, j] != 2] if samples is None else np.where(A[:, [j]] == 2, rng.integers(0, 2, (len(A), 1)), A)
    return A


def index_of(A):
    L = A.shape[1]
    sh = np.arange(L)
    return ((A == 0).astype(np.int64) << sh).sum(1) | (((A == 1).astype(np.int64) << sh).sum(1) << L)


def leaf_values(order, A):
    return {id(l): (A[:, j] == 0, A[:, j] == 1) for j, l in enumerate(order)}


def check_tables(tree, gbs, label, numeric_gbs=()):
    rc, p = plan(tree, gbs, numeric_gbs)
    assert rc == 0, f"{label}: {p}"
    cols, order = numbering(tree, [g for g in gbs if g not in numeric_gbs])
    L = len(order)
    assert p["cols"] == cols, label
    assert [(l["k"], l["op"], l["index"]) for l in p["leaves"]] == [(l["k"], l["op"], j) for j, l in enumerate(order)], label
    assert [l["col"] for l in p["leaves"]] == [-1 if is_num(l) else cols.index(l["k"]) for l in order], label
    nnum = sum(is_num(l) for l in order)
    assert [n["leaf"] for n in p["nleaves"]] == list(range(L - nnum, L)), label
    A = assignments(order)
    val = leaf_values(order, A)
    ix = index_of(A)
    conj = conjuncts(tree)
    # ---- 3.1.a ----
    whole = kleene(tree, val)[0]
    truth = bits(p["truth"], L)
    if p["vleaf"]:
        pure_val = [c for c in conj if all(is_num(l) for l in ft.leaves_of(c))]
        strs = [c for c in conj if c not in pure_val]
        assert all(l["k"] == ft.VALUE for l in order if is_num(l)) and pure_val, label
        assert all(not is_num(l) for c in strs for l in ft.leaves_of(c)), label
        assert np.array_equal(truth[ix], kleene(conj_of(strs), val)[0]), f"{label}: truth (string conjuncts)"
        assert np.array_equal(bits(p["truth_x"], L)[ix], whole), f"{label}: truth_x"
        # ---- 3.1.c ----
        numeric_known = np.all(A[:, L - nnum:] != 2, axis=1)
        m = ((A[:, L - nnum:] == 0).astype(np.int64) << np.arange(nnum)).sum(1)
        vt = (p["vtab"] >> m) & 1
        assert np.array_equal((truth[ix] & (vt == 1))[numeric_known], whole[numeric_known]), f"{label}: vtab"
        conj = strs
    else:
        assert p["truth_x"] == [] and p["vtab"] == 0, label
        assert np.array_equal(truth[ix], whole), f"{label}: truth"
    # ---- the split ----
    ncol = len(cols)
    dev_of = p["dev_of"]
    assert sorted(dev_of) == list(range(ncol)) and dev_of[p["lead"]] == 0, label
    colsets = [{"#" if is_num(l) else l["k"] for l in ft.leaves_of(c)} for c in conj]
    single = [next(iter(s)) for s in colsets if len(s) == 1 and "#" not in s]
    if p["late_mask"]:
        # ---- 3.1.b ----
        e = p["early"]
        assert 0 <= e < ncol and cols[e] in single, label
        te, tl = bits(p["truth_early"], L), bits(p["truth_late"], L)
        assert np.array_equal(te[ix] & tl[ix], truth[ix]), f"{label}: early & late"
        early_leaf = np.array([(not is_num(l)) and l["k"] == cols[e] for l in order], bool)
        assert np.array_equal(te[index_of(np.where(early_leaf, A, 2))], te[ix]), f"{label}: early reads late leaves"
        assert np.array_equal(tl[index_of(np.where(early_leaf, 2, A))], tl[ix]), f"{label}: late reads early leaves"
        assert p["late_mask"] == sum(1 << dev_of[s] for s in range(ncol) if s != e), f"{label}: late_mask {p}"
        if e > 0 and ncol <= 3 and not os.environ.get("LK_NO_EARLY_FIRST"):
            assert dev_of[e] == 0 and dev_of[0] == e, label
        else:
            assert dev_of == list(range(ncol)), label
        reasons = []
    else:
        assert p["truth_early"] == [] and p["truth_late"] == [] and dev_of == list(range(ncol)), label
        # ---- 3.1.d: why there is no late pass ----
        reasons = []
        if ncol < 2:
            reasons.append("one string column")
        if nnum and not p["vleaf"]:
            reasons.append("a numeric leaf outside vleaf")
        if not single:
            reasons.append("no single-column conjunct")
        elif any(len(s) > 1 and cols[p["early"]] in s for s in colsets if 0 <= p["early"] < ncol):
            reasons.append("a mixed conjunct")
        assert reasons, f"{label}: late_mask == 0 without a documented reason: {p}"
    # and the other way round: a filter with none of the reasons must split
    if ncol >= 2 and single and not (nnum and not p["vleaf"]) and all(len(s) == 1 for s in colsets):
        assert p["late_mask"], f"{label}: single-column conjuncts only, and no late pass: {p}"
    return p, reasons


TABLE_STRATA = ["one_column", "early_late", "mixed", "wide", "value_leaves", "numeric"]
N_TABLE = 50


@pytest.mark.parametrize("stratum", TABLE_STRATA)
def test_truth_tables(stratum):
    """3.1.a-c over 50 trees per stratum (<= 6 leaves; the numeric stratum's larger trees go to test_programs)."""
    seen = {"late": 0, "swap": 0, "vleaf": 0, "n": 0}
    for i, tree in ft.trees(stratum, 2 * N_TABLE if stratum == "numeric" else N_TABLE):
        if len(ft.leaves_of(tree)) > 6:
            continue
        gbs = ft.wide_group_bys(i, tree) if stratum == "wide" else GBS[i % 3]
        p, _ = check_tables(tree, gbs, ft.describe(stratum, i, tree))
        seen["n"] += 1
        seen["late"] += p["late_mask"] != 0
        seen["swap"] += p["dev_of"] != sorted(p["dev_of"])
        seen["vleaf"] += p["vleaf"]
    assert seen["n"] >= N_TABLE, seen
    if stratum == "early_late":
        assert seen["late"] == seen["n"] and seen["swap"] >= 5, seen   # every conjunct tree over >= 2 columns splits
    if stratum == "mixed":
        assert seen["late"] == 0, seen
    if stratum == "wide":
        assert seen["swap"] == 0, seen
    if stratum == "value_leaves":
        assert seen["vleaf"] == seen["n"], seen


def test_split_reasons():
    """3.1.d: conjunct trees over >= 2 columns that must not split, 20 per documented reason."""
    for i in range(20):
        rng = np.random.default_rng([ft.SEED, 100, i])
        cols = [[ft.NAME, ft.SVC], [ft.SVC, ft.NS], [ft.NAME, ft.SVC, ft.NS]][i % 3]
        base = ft.conjunct_tree(rng, cols, 3 if i % 2 else len(cols))
        # a numeric leaf outside vleaf: a conjunct on attr.dur
        t = ft.and_chain([base, ft.numeric_leaf(rng, ft.DUR)])
        _, why = check_tables(t, GBS[i % 3], ft.describe("reason:numeric", i, t))
        assert "a numeric leaf outside vleaf" in why, (i, why)
        # no single-column conjunct: every conjunct an `or` over two columns
        t = ft.and_chain([{"op": "or", "q1": ft.string_leaf(rng, ft.NAME), "q2": ft.string_leaf(rng, ft.SVC)},
                          {"not": {"op": "and", "q1": ft.string_leaf(rng, ft.NS), "q2": ft.string_leaf(rng, ft.SVC)}}])
        _, why = check_tables(t, GBS[i % 3], ft.describe("reason:none-single", i, t))
        assert why == ["no single-column conjunct"], (i, why)
        # a conjunct that mixes the early column with another
        t = ft.and_chain([base, {"op": "or", "q1": ft.string_leaf(rng, ft.NAME), "q2": ft.string_leaf(rng, ft.SVC)},
                          {"not": ft.string_leaf(rng, ft.NAME)}])
        p, why = check_tables(t, GBS[i % 3], ft.describe("reason:mixed", i, t))
        assert why == ["a mixed conjunct"], (i, why)
        assert p["late_mask"] == 0, (i, p)


def run_prog(prog, A):
    """The postfix program on (is_true, is_false) arrays: a stack machine of its own."""
    st = []
    for op in prog:
        if op < 0x80:
            st.append((A[:, op] == 0, A[:, op] == 1))
        elif op == OP_NOT:
            t, f = st.pop()
            st.append((f, t))
        elif op == OP_TRUE:
            st.append((np.ones(len(A), bool), np.zeros(len(A), bool)))
        else:
            (t2, f2), (t1, f1) = st.pop(), st.pop()
            st.append((t1 & t2, f1 | f2) if op == OP_AND else (t1 | t2, f1 & f2))
    assert len(st) == 1
    return st[0], max(1, sum(1 for op in prog if op < 0x80))


def check_program(tree, gbs, label):
    rc, p = plan(tree, gbs)
    assert rc == 0, f"{label}: {p}"
    cols, order = numbering(tree, gbs)
    assert [(l["k"], l["op"]) for l in p["leaves"]] == [(l["k"], l["op"]) for l in order], label
    assert len(p["prog"]) <= MAXPROG and p["truth"] == [] and p["late_mask"] == 0 and p["vleaf"] == 0, label
    A = assignments(order, np.random.default_rng([ft.SEED, 7, len(order)]), 200)
    (t, f), _ = run_prog(p["prog"], A)
    wt, wf = kleene(tree, leaf_values(order, A))
    assert np.array_equal(t, wt) and np.array_equal(f, wf), f"{label}: prog {p['prog']}"


def test_programs():
    """3.2: 48 program-stratum trees and the numeric stratum's 7..12-leaf trees through the returned program."""
    n = 0
    for i, tree in ft.trees("program", 48):
        check_program(tree, GBS[i % 3] if len(ft._leaf_count(tree)) <= 5 else [], ft.describe("program", i, tree))
        n += 1
    for i, tree in ft.trees("numeric", 48):
        if len(ft.leaves_of(tree)) > 6:
            check_program(tree, GBS[i % 3], ft.describe("numeric", i, tree))
            n += 1
    assert n >= 60


def test_right_deep_and_maxprog():
    """Right-deep chains of 32 leaves (stack depth 32); NOTs that push the program past MAXPROG are refused."""
    for i in range(6):
        rng = np.random.default_rng([ft.SEED, 200, i])
        tree = ft.right_deep(rng, 32, ft.STRINGS[:4 + i % 3])
        check_program(tree, [], ft.describe("right_deep", i, tree))
        rc, p = plan(tree)
        assert len(p["prog"]) == 63
        # 33 NOTs fit exactly (96); 34 do not
        t33 = tree
        for _ in range(33):
            t33 = {"not": t33}
        t34 = {"not": t33}
        rc, p = plan(t33)
        assert rc == 0 and len(p["prog"]) == MAXPROG, p
        check_program(t33, [], "33 NOTs")
        rc, msg = plan(t34)
        assert rc == LK_ERR_UNSUPPORTED and "too large" in msg, (rc, msg)


def test_refusals():
    rng = np.random.default_rng([ft.SEED, 300])
    leaf = lambda c: ft.string_leaf(rng, c)   # noqa: E731
    # 8 string columns are planned, 9 refused
    eight = ft.and_chain([leaf(c) for c in ft.STRINGS[:5]])
    assert plan(eight, ft.STRINGS[5:])[0] == 0
    rc, msg = plan(eight, ft.STRINGS[5:] + ["attr.ninth"])
    assert rc == LK_ERR_UNSUPPORTED and "too many string columns" in msg, (rc, msg)
    # 32 leaves are planned, 33 refused
    assert plan(ft.right_deep(rng, 32, ft.STRINGS[:4]))[0] == 0
    rc, msg = plan(ft.right_deep(rng, 33, ft.STRINGS[:5]))
    assert rc == LK_ERR_UNSUPPORTED and "too many filter leaves" in msg, (rc, msg)
    # 8 leaves on one column are planned, 9 refused (LEAF_BITS)
    assert plan(ft.right_deep(rng, 8, [ft.SVC]))[0] == 0
    rc, msg = plan(ft.right_deep(rng, 9, [ft.SVC]))
    assert rc == LK_ERR_UNSUPPORTED and "too many leaves on one column" in msg, (rc, msg)
    # a column used both as text and as a number
    both = {"op": "and", "q1": {**leaf(ft.SVC), "k": ft.DUR}, "q2": ft.numeric_leaf(rng, ft.DUR)}
    rc, msg = plan(both)
    assert rc == LK_ERR_UNSUPPORTED and "both as a string and as a number" in msg, (rc, msg)


def test_numeric_group_by_leaves_no_string_column():
    """A numeric groupBy is a numeric query column: no string column, no late pass (the row scan takes the call)."""
    for i, tree in ft.trees("mixed", 10):
        p, why = check_tables(tree, [ft.CODE], ft.describe("mixed+code", i, tree), numeric_gbs=[ft.CODE])
        assert ft.CODE not in p["cols"] and p["nums"] == [ft.CODE] and p["late_mask"] == 0, p
