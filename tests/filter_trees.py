"""Seeded random filter trees and the small Parquet files they run over: shared by the CPU plan test
(test_filter_plan_cpu.py), the oracle cross-check (test_oracle_cpu.py) and the GPU fuzz (test_gpu_filter_trees.py).
No test in here.

Files (make_files): six profiles that steer the scan kernels' per-tile branches --
  a  NULL-free, 4 names                       b  NULL-free, 40 names (code mask `fast`, not `emask32`), one ~20k-row group
  c  NULL-free, 100 names (no code mask)      d  NULLs only in the service column (a late column)
  e  NULLs in the name and namespace columns  f  as (a), the attr.msg column absent
Besides the name / service / namespace / attr.msg tags every file carries four more small tag columns (attr.zone,
attr.tier, attr.env, attr.pod: functions of the service and namespace) so a query can reach the 8-string-column limit
with real columns.

Trees (random_tree, conjunct_tree, value_leaf_tree): JSON filters as query-api sends them.  Everything is seeded;
describe() is the text a failing assertion carries (seed, index, tree)."""
import json

import numpy as np

NAME = "_cardinalhq.name"
VALUE = "_cardinalhq.value"
TIMESTAMP = "_cardinalhq.timestamp"
SVC = "resource.service.name"
NS = "resource.k8s.namespace.name"
MSG = "attr.msg"
DUR = "attr.dur"
RATIO = "attr.ratio"
CODE = "attr.code"
EXTRA = ["attr.zone", "attr.tier", "attr.env", "attr.pod"]
STRINGS = [NAME, SVC, NS, MSG] + EXTRA
SEED = 17

T0 = 1704067200000   # lakeside_amd.synth.T0
HOUR = 3_600_000

# profile -> (rows, names, row_group_size); rows odd and no multiple of 64
PROFILES = {"a": (5003, 4, 2500), "b": (20011, 40, 1 << 20), "c": (6007, 100, 2500), "d": (6501, 4, 2500),
            "e": (6999, 4, 2500), "f": (5701, 4, 2500)}
_CARD = {SVC: ("svc-", 5), NS: ("ns-", 3), MSG: ("m", 9), "attr.zone": ("z", 4), "attr.tier": ("t", 3),
         "attr.env": ("e", 2), "attr.pod": ("p", 7)}


def make_files(dirpath, value_nulls):
    """Writes the six files; returns (paths, blobs, ts) -- ts: every file's timestamps (for window row counts)."""
    import os

    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(SEED + (1 if value_nulls else 0))
    paths, blobs, tss = [], [], []
    for prof, (n, names, rg) in PROFILES.items():
        ts = np.sort(T0 + rng.integers(0, HOUR, n))
        val = rng.lognormal(0, 2, n)
        vmask = None
        if value_nulls:
            val[rng.random(n) < 0.02] = np.nan
            vmask = rng.random(n) < 0.05
        none = np.zeros(n, bool)
        cols = {TIMESTAMP: pa.array(ts, pa.int64()), VALUE: pa.array(val, pa.float64(), mask=vmask),
                NAME: pa.array([f"metric_{k:02d}" for k in rng.integers(0, names, n)], pa.string(),
                               mask=(rng.random(n) < 0.07) if prof == "e" else none)}
        ix = {c: rng.integers(0, card, n) for c, (_, card) in _CARD.items() if c not in EXTRA}
        # the four extra tags follow the service and the namespace, so eight groupBys do not make one group per row
        ix.update({"attr.zone": ix[SVC] % 4, "attr.tier": ix[NS], "attr.env": ix[SVC] % 2,
                   "attr.pod": (3 * ix[SVC] + ix[NS]) % 7})
        for c, (pre, card) in _CARD.items():
            nulls = (prof == "d" and c == SVC) or (prof == "e" and c == NS)
            if prof == "f" and c == MSG:
                continue
            cols[c] = pa.array([f"{pre}{k}" for k in ix[c]], pa.string(), mask=(rng.random(n) < 0.1) if nulls else none)
        cols["_cardinalhq.message"] = pa.array([f"line {k}" for k in ix[MSG]], pa.string())   # (exemplar rows project it)
        cols[DUR] = pa.array(rng.integers(0, 5_000_000, n), pa.int64(), mask=rng.random(n) < 0.1)
        cols[RATIO] = pa.array(rng.random(n).astype(np.float32), pa.float32())
        cols[CODE] = pa.array((rng.integers(0, 6, n) * 100 + 200).astype(np.int32), pa.int32())
        t = pa.table(cols)
        strings = [c for c in t.column_names if t.schema.field(c).type == pa.string()]
        path = os.path.join(str(dirpath), f"ft_{'n' if value_nulls else 'c'}_{prof}.parquet")
        pq.write_table(t, path, compression="NONE", use_dictionary=strings, row_group_size=rg,
                       column_encoding={c: "PLAIN" for c in t.column_names if c not in strings})
        paths.append(path)
        with open(path, "rb") as f:
            blobs.append(f.read())
        tss.append(ts)
    return paths, blobs, tss


# ---- leaves ----
# literals: the last one of every list is a value no file holds (drawn for one leaf literal in eight)
_LIT = {NAME: ["metric_00", "metric_01", "metric_02", "metric_03", "metric_17", "nope"],
        SVC: ["svc-0", "svc-1", "svc-2", "svc-3", "svc-4", "svc-9"], NS: ["ns-0", "ns-1", "ns-2", "ns-x"],
        MSG: [f"m{k}" for k in range(9)] + ["mx"], "attr.zone": ["z0", "z1", "z2", "z3", "zz"],
        "attr.tier": ["t0", "t1", "t2", "tt"], "attr.env": ["e0", "e1", "ee"],
        "attr.pod": [f"p{k}" for k in range(7)] + ["pp"]}
_RE = {NAME: ["^metric_0[0-2]$", "metric_.[13]", "_1", "^METRIC_03"], SVC: ["^svc-[0-2]", "[34]$"], NS: ["ns-[01]", "2|x"],
       MSG: ["^m[0-4]$", "m[2468]"], "attr.zone": ["z[12]"], "attr.tier": ["t[^0]"], "attr.env": ["e1"],
       "attr.pod": ["p[0-3]"]}
_SUB = {NAME: ["c_0", "7", "_02"], SVC: ["-3", "vc"], NS: ["-1", "s-"], MSG: ["m", "5"], "attr.zone": ["1"],
        "attr.tier": ["2"], "attr.env": ["0"], "attr.pod": ["6"]}
STRING_OPS = ["eq", "!=", "in", "not_in", "regex", "contains", "exists"]
_OP_P = [0.2, 0.15, 0.2, 0.15, 0.12, 0.1, 0.08]
_NUM_LIT = {VALUE: ["0.5", "1", "2.5", "1e1", "40"], DUR: ["2500000", "2.5e6", "400000", "4.6e6"],
            RATIO: ["0.25", "0.5", "0.75", "0.9"]}


def string_leaf(rng, col):
    op = STRING_OPS[int(rng.choice(len(STRING_OPS), p=_OP_P))]
    lit = _LIT[col]

    def one():
        return lit[-1] if rng.random() < 0.125 else lit[int(rng.integers(0, len(lit) - 1))]
    if op in ("eq", "!="):
        v = [one()]
    elif op in ("in", "not_in"):
        v = sorted({one() for _ in range(int(rng.integers(1, 4)))})
    elif op == "regex":
        v = [_RE[col][int(rng.integers(0, len(_RE[col])))]]
    elif op == "contains":
        v = [_SUB[col][int(rng.integers(0, len(_SUB[col])))]]
    else:
        v = []
    return {"k": col, "v": v, "op": op, "extracted": False, "computed": False, "dataType": "string"}


def numeric_leaf(rng, col):
    op = ["gt", "ge", "lt", "le"][int(rng.integers(0, 4))]
    lit = _NUM_LIT[col]
    return {"k": col, "v": [lit[int(rng.integers(0, len(lit)))]], "op": op, "extracted": False, "computed": False,
            "dataType": "number"}


def _tree(rng, n_leaves, leaf_fn, p_not, p_and=0.5):
    def node(n):
        if n == 1:
            q = leaf_fn()
        else:
            k = int(rng.integers(1, n))
            q = {"op": "and" if rng.random() < p_and else "or", "q1": node(k), "q2": node(n - k)}
        return {"not": q} if rng.random() < p_not else q
    return node(n_leaves)


def random_tree(rng, n_leaves, string_cols, numeric=(), p_not=0.25, p_and=0.5):
    """A random binary tree of exactly n_leaves leaves over string_cols (string operators) and the `numeric` columns
    (gt/ge/lt/le); every node is wrapped in {"not": ..} with probability p_not."""
    def leaf():
        if numeric and (not string_cols or rng.random() < 0.5):
            return numeric_leaf(rng, numeric[int(rng.integers(0, len(numeric)))])
        return string_leaf(rng, string_cols[int(rng.integers(0, len(string_cols)))])
    return _tree(rng, n_leaves, leaf, p_not, p_and)


def and_chain(parts):
    q = parts[-1]
    for p in reversed(parts[:-1]):
        q = {"op": "and", "q1": p, "q2": q}
    return q


def conjunct_tree(rng, cols, n_leaves, p_not=0.25):
    """A top-level `and` chain whose every conjunct is a random subtree over one column of `cols` (each column gets a
    conjunct, in shuffled order): the shape plan_truth splits into early and late."""
    assert n_leaves >= len(cols)
    share = [1] * len(cols)
    for _ in range(n_leaves - len(cols)):
        share[int(rng.integers(0, len(cols)))] += 1
    # (inside a conjunct `or` is the likelier node: an `and` over one small column mostly contradicts itself)
    parts = [random_tree(rng, share[i], [cols[i]], (), p_not, 0.25) for i in range(len(cols))]
    order = rng.permutation(len(parts))
    return and_chain([parts[int(i)] for i in order])


def value_leaf_tree(rng, cols, n_str, n_val, p_not=0.25):
    """String conjuncts `and` one subtree of n_val leaves on the value column."""
    parts = ([conjunct_tree(rng, cols, n_str, p_not)] if n_str else []) + [random_tree(rng, n_val, [], (VALUE,), p_not)]
    if rng.random() < 0.5:
        parts.reverse()
    return and_chain(parts)


def right_deep(rng, n_leaves, cols):
    """leaf op (leaf op (leaf ...)): the interpreter's stack grows to n_leaves."""
    q = string_leaf(rng, cols[(n_leaves - 1) % len(cols)])
    for i in range(n_leaves - 2, -1, -1):
        q = {"op": "and" if rng.random() < 0.5 else "or", "q1": string_leaf(rng, cols[i % len(cols)]), "q2": q}
    return q


# ---- strata: name -> tree of index i (own rng) ----
def _one_column(rng, i):
    return random_tree(rng, 1 + i % 6, [NAME])


def _early_late(rng, i):
    cols = [[NAME, SVC], [SVC, NS], [NAME, SVC, NS], [NS, NAME], [SVC, MSG]][i % 5]
    return conjunct_tree(rng, cols, max(len(cols), 2 + i % 5))


def _mixed(rng, i):
    """One top-level conjunct over two or more columns (an `or` or a `not` at the root): nothing to split."""
    cols = [[NAME, SVC], [NAME, SVC, NS], [SVC, NS], [NAME, MSG, NS]][i % 4]
    while True:
        q = random_tree(rng, 2 + i % 5, cols, (), 0.3)
        if q.get("op") == "and":
            q["op"] = "or"
        if len(_leaf_count(q)) >= 2:
            return {"not": q} if i % 3 == 0 and "op" in q else q   # (a negated `or`: the selective end)


def _wide(rng, i):
    """<= 6 leaves over 2-4 of the string columns; wide_group_bys() brings the query to 4 + i % 5 string columns."""
    k = 2 + i % 3
    cols = [STRINGS[int(c)] for c in rng.choice(len(STRINGS), k, replace=False)]
    return random_tree(rng, min(6, k + i % 4), cols, (), 0.2)


def wide_group_bys(i, tree):
    have = {NAME} | set(_leaf_count(tree))
    gbs = []
    for c in [SVC, NS] + EXTRA + [MSG]:   # (attr.msg last: it multiplies the groups by nine)
        if len(have) + len(gbs) >= max(4, min(8, 4 + i % 5)):
            break
        if c not in have:
            gbs.append(c)
    return gbs


def _program(rng, i):
    """7..32 leaves over 1-5 columns, at most 8 on any one column."""
    n = [7, 8, 12, 16, 24, 32, 9, 20][i % 8]
    ncols = max(1 + i % 5, -(-n // 8))
    pool = [STRINGS[c % ncols] for c in range(n)]
    rng.shuffle(pool)
    return _tree(rng, n, lambda: string_leaf(rng, pool.pop()), 0.15)


def _value_leaves(rng, i):
    n_val = 1 + i % 5
    cols = [[NAME], [NAME, SVC], [NAME, SVC, NS], [SVC], [NAME, NS]][(i // 5) % 5]
    n_str = 0 if i % 11 == 10 else min(6 - n_val, len(cols) + i % 2)
    return value_leaf_tree(rng, cols[:n_str], n_str, n_val)


def _numeric(rng, i):
    n = 1 + i % 12
    while True:   # (at least one numeric leaf)
        q = random_tree(rng, n, [NAME, SVC, NS][:1 + i % 3] if n > 1 else [], (DUR, RATIO), 0.2)
        if any(l["op"] in ("gt", "ge", "lt", "le") for l in leaves_of(q)):
            return q


STRATA = {"one_column": _one_column, "early_late": _early_late, "mixed": _mixed, "wide": _wide, "program": _program,
          "value_leaves": _value_leaves, "numeric": _numeric}


def _leaf_count(q, out=None):
    out = {} if out is None else out
    if "not" in q:
        return _leaf_count(q["not"], out)
    if "k" in q:
        out[q["k"]] = out.get(q["k"], 0) + 1
        return out
    _leaf_count(q["q1"], out)
    return _leaf_count(q["q2"], out)


def leaves_of(q):
    if "not" in q:
        return leaves_of(q["not"])
    if "k" in q:
        return [q]
    return leaves_of(q["q1"]) + leaves_of(q["q2"])


def trees(stratum, count, seed=SEED):
    """[(index, tree)] of a stratum: tree i comes from its own generator, so a longer list extends a shorter one."""
    sid = sorted(STRATA).index(stratum)
    return [(i, STRATA[stratum](np.random.default_rng([seed, sid, i]), i)) for i in range(count)]


def describe(stratum, index, tree, seed=SEED):
    return f"stratum {stratum} seed {seed} index {index} tree {json.dumps(tree, sort_keys=True)}"
