"""Expectation of a formula over DataExprs, independent of the code under test (lk_eval_formula, the C parser, the
cell function): every variable goes through queryapi.evaluate_base_expr (already checked against the oracle), then
QueryEngineV2.evaluateFormula's second pass is restated here over those payloads per timestamp:

  * each payload becomes {sum: value} and BaseExpr.eval runs again (QueryEngineV2.scala:344-371): the chart transformer
    is applied a second time and rows collapse per group key (idempotent);
  * Formula.eval / ASTUtils.eval (Formula.scala:32-69, ASTUtils.scala:42-69) join the sides per key.

Keys are the tuple of group values (absent read as ""), () without groupBys.  A value whose tags come from a constant
under groupBys carries the candidate tag maps instead (any row of that key and timestamp)."""
import math
import re
import struct

import numpy as np

from lakeside_amd import queryapi as qa

_TOKEN = re.compile(r"\s*(?:(\d+(?:\.\d+)?(?:[eE][+-]?\d+)?)|([A-Za-z_][A-Za-z0-9_]*)|(.))")


def parse(formula):
    """AST: ("var", name) | ("const", float) | (op, e1, e2) with op in + - * /; precedence climbing."""
    toks = []
    pos = 0
    while pos < len(formula) and formula[pos:].strip():
        m = _TOKEN.match(formula, pos)
        num, ident, ch = m.groups()
        toks.append(("const", float(num)) if num else ("var", ident) if ident else ch)
        pos = m.end()
    i = [0]

    def atom():
        t = toks[i[0]]
        i[0] += 1
        if t == "(":
            e = expr()
            assert toks[i[0]] == ")"
            i[0] += 1
            return e
        assert isinstance(t, tuple), t
        return t

    def term():
        e = atom()
        while i[0] < len(toks) and toks[i[0]] in ("*", "/"):
            op = toks[i[0]]
            i[0] += 1
            e = (op, e, atom())
        return e

    def expr():
        e = term()
        while i[0] < len(toks) and toks[i[0]] in ("+", "-"):
            op = toks[i[0]]
            i[0] += 1
            e = (op, e, term())
        return e

    e = expr()
    assert i[0] == len(toks)
    return e


def variables(ast):
    if ast[0] == "var":
        return [ast[1]]
    if ast[0] == "const":
        return []
    out = []
    for v in variables(ast[1]) + variables(ast[2]):
        if v not in out:
            out.append(v)
    return out


def _java_double(x):
    """Java's Double.toString for the plain-notation range the tests use (1e-3 <= |x| < 1e7, or 0)."""
    assert x == 0 or 1e-3 <= abs(x) < 1e7
    return repr(float(x))


def label(ast, base_expressions, tags):
    if ast[0] == "var":
        return qa.label(base_expressions[ast[1]], tags)
    if ast[0] == "const":
        return _java_double(ast[1])
    return f"{label(ast[1], base_expressions, tags)} {ast[0]} {label(ast[2], base_expressions, tags)}"


class Side:
    """One EvalResult: value, tags -- or, for a constant under groupBys, the candidate tag maps."""

    def __init__(self, value, tags=None, cands=None):
        self.value, self.tags, self.cands = value, tags, cands


def _eval(ast, leaves, group_bys, all_rows):
    """ASTUtils.eval for one timestamp: {key: Side}."""
    if ast[0] == "var":
        return leaves.get(ast[1], {})
    if ast[0] == "const":
        if not group_bys:
            return {(): Side(ast[1], tags={})}
        out = {}
        for key, tags in all_rows:
            out.setdefault(key, Side(ast[1], cands=[])).cands.append(tags)
        return out
    op = ast[0]
    m1, m2 = _eval(ast[1], leaves, group_bys, all_rows), _eval(ast[2], leaves, group_bys, all_rows)
    out = {}
    for key in list(m1) + [k for k in m2 if k not in m1]:
        e1, e2 = m1.get(key), m2.get(key)
        if e1 is None or e2 is None:
            if op != "+":
                continue
            if e1 is None:
                e1 = Side(0.0, e2.tags, e2.cands)
            else:
                e2 = Side(0.0, e1.tags, e1.cands)
        with np.errstate(all="ignore"):
            a, b = np.float64(e1.value), np.float64(e2.value)
            if op == "+":
                v = a + b
            elif op == "-":
                v = a - b
            elif op == "*":
                v = a * b
            else:
                if not (b != 0):
                    continue
                v = a / b
        out[key] = Side(float(v), e1.tags, e1.cands)
    return out


def expected(engine, base_expressions, formula, segs_by_id, paths_by_id, step_ms, glob_size, now_ms):
    """{timestamp: {key: Side}} of the formula, and the AST."""
    ast = parse(formula)
    used = variables(ast)
    gb_sets = [sorted(set((base_expressions[v].get("chart") or {}).get("groupBys") or [])) for v in used]
    group_bys = gb_sets[0] if gb_sets else []
    assert all(g == group_bys for g in gb_sets)
    per_ts = {}
    for v in used:
        be = base_expressions[v]
        payloads = qa.evaluate_base_expr(engine, be, segs_by_id[v], paths_by_id[v], step_ms, glob_size, now_ms)
        tf = qa.transformer(be, step_ms)
        for p in payloads:
            m = p["message"]
            key = tuple(str(m["tags"].get(g, "")) for g in group_bys)
            value = float(tf(np.array([m["value"]]))[0])   # the second BaseExpr.eval
            slot = per_ts.setdefault(m["timestamp"], {}).setdefault(v, {})
            rank = sorted(m["tags"].items())
            if key not in slot or rank < slot[key][0]:
                slot[key] = (rank, Side(value, tags=dict(m["tags"])))
    out = {}
    for ts, leaves in per_ts.items():
        leaves = {v: {k: s for k, (_, s) in rows.items()} for v, rows in leaves.items()}
        all_rows = [(k, s.tags) for v in used for k, s in leaves.get(v, {}).items()]
        cells = _eval(ast, leaves, group_bys, all_rows)
        if cells:
            out[ts] = cells
    return out, ast, group_bys


def bits(x):
    return struct.pack("<d", x)


def same_value(a, b):
    return bits(a) == bits(b) or (math.isnan(a) and math.isnan(b))


def assert_rows(got_rows, want, group_bys, what=""):
    """got_rows: [(ts, value, tags)] ascending in ts; want: expected()'s map.  Per timestamp the rows are a set keyed
    by the group-value tuple; values bit for bit (NaN = NaN); tags equal, or among a constant's candidates."""
    ts_seq = [r[0] for r in got_rows]
    assert ts_seq == sorted(ts_seq), f"{what}: timestamps not ascending"
    got = {}
    for ts, v, tags in got_rows:
        key = tuple(str(tags.get(g, "")) for g in group_bys)
        assert key not in got.setdefault(ts, {}), f"{what}: key {key} twice at {ts}"
        got[ts][key] = (v, tags)
    assert sorted(got) == sorted(want), f"{what}: timestamps differ ({len(got)} vs {len(want)})"
    n = 0
    for ts, cells in want.items():
        assert sorted(got[ts]) == sorted(cells), f"{what}: keys differ at {ts}"
        for key, side in cells.items():
            v, tags = got[ts][key]
            assert same_value(v, side.value), f"{what}: {ts} {key}: {v!r} != {side.value!r}"
            if side.cands is not None:
                assert tags in side.cands, f"{what}: {ts} {key}: tags {tags} not among the candidates"
            else:
                assert tags == side.tags, f"{what}: {ts} {key}: tags {tags} != {side.tags}"
            n += 1
    return n


def expected_payloads(want, ast, formula, base_expressions):
    out = []
    for ts in sorted(want):
        for key in sorted(want[ts]):
            s = want[ts][key]
            tags = s.tags if s.cands is None else None
            out.append({"id": formula, "type": "timeseries",
                        "message": {"timestamp": ts, "tags": tags, "value": s.value,
                                    "label": None if tags is None else label(ast, base_expressions, tags)}})
    return out
