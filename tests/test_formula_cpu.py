"""Formulas over DataExprs, the parts that need no GPU (liblakeside_text.so only): the formula parser
(lk_formula_plan, lakeside_amd/csrc/formula.cpp), the cell function the GPU kernels compile (lk_formula_eval_cell,
formula_cell.hpp) against the Python restatement of Formula.eval (tests/formula_ref.py), and the labels."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

from tests import formula_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lakeside_amd", "liblakeside_text.so")
ARG, UNSUPPORTED = -1, -2


def _lib():
    L = ctypes.CDLL(LIB)
    L.lk_formula_plan.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_char_p,
                                  ctypes.c_size_t]
    L.lk_formula_plan.restype = ctypes.c_int
    L.lk_formula_eval_cell.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_size_t,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]
    L.lk_formula_eval_cell.restype = ctypes.c_int
    return L


def _names(names):
    return (ctypes.c_char_p * len(names))(*[n.encode() for n in names])


def plan(formula, names=("a", "b", "c")):
    out = ctypes.create_string_buffer(4096)
    rc = _lib().lk_formula_plan(formula.encode(), _names(names), len(names), out, len(out))
    return rc, out.value.decode()


def test_precedence_and_associativity():
    assert plan("a+b*c") == (0, "$0 $1 $2 * +")          # a + (b * c)
    assert plan("a*b+c") == (0, "$0 $1 * $2 +")
    assert plan("a-b-c") == (0, "$0 $1 - $2 -")          # (a - b) - c
    assert plan("a/b/c") == (0, "$0 $1 / $2 /")          # (a / b) / c
    assert plan("a-b+c") == (0, "$0 $1 - $2 +")
    assert plan("a/b*c") == (0, "$0 $1 / $2 *")
    assert plan("a / b * 100") == (0, "$0 $1 / 100.0 *")


def test_parentheses_blanks_and_numbers():
    assert plan("(a+b)*c") == (0, "$0 $1 + $2 *")
    assert plan("a/(b-c)") == (0, "$0 $1 $2 - /")
    assert plan("((a)) + (b)") == (0, "$0 $1 +")
    assert plan("  a \t+\n b  ") == (0, "$0 $1 +")
    assert plan("a*1e3") == (0, "$0 1000.0 *")
    assert plan("a * 2.5E-2") == (0, "$0 0.025 *")
    assert plan("a*1.0e-4") == (0, "$0 1.0E-4 *")        # constants print as Java's Double.toString
    assert plan("a + 12345678.5") == (0, "$0 1.23456785E7 +")
    assert plan("5 + 3") == (0, "5.0 3.0 +")
    assert plan("x_1 + _y", names=("x_1", "_y")) == (0, "$0 $1 +")


@pytest.mark.parametrize("formula", ["a + d", "(a", "a", "(a)", "7", "a + b)", "a +", "", "a b", "2a", "1. + a", "a + .5",
                                     "a $ b", "a + 1e", "(a + b"])
def test_malformed_is_arg(formula):
    rc, msg = plan(formula)
    assert rc == ARG, (formula, rc, msg)
    assert msg.startswith("formula:")


@pytest.mark.parametrize("formula,token", [("a^b", "^"), ("a>b", ">"), ("a >= b", ">="), ("a<b", "<"), ("a == b", "=="),
                                           ("a != b", "!="), ("-a", "-"), ("a*-b", "-"), ("+a + b", "+"),
                                           ("(a + b) ^ 2", "^"), ("a - -1", "-")])
def test_unrestated_productions_are_unsupported(formula, token):
    rc, msg = plan(formula)
    assert rc == UNSUPPORTED, (formula, rc, msg)
    assert f"'{token}'" in msg, msg      # the token is named


def test_unknown_variable_names_it():
    rc, msg = plan("a / total")
    assert rc == ARG and "total" in msg


PROGRAMS = ["a + b", "a - b", "a * b", "a / b", "a / b * 100", "a / (a + b)", "(a - b) / (a + b) * 100", "100 * a",
            "a + 0", "a / (b - b)", "a / ((0 - b) * 0)", "a + b + c", "a * b - c / a", "(a + b) * (c + 1.5) / (b + c)",
            "5 + a - b", "a + (b * c) + (2 / c)"]
SPECIAL = [0.0, -0.0, math.nan, math.inf, -math.inf, 1e308, -1e308, 5e-324]


def _python_cell(ast, present, value, names):
    """Formula.eval for one cell through tests/formula_ref.py: leaves present / absent under the key ()."""
    leaves = {n: ({(): fr.Side(value[i], tags={"leaf": i})} if present[i] else {}) for i, n in enumerate(names)}
    cell = fr._eval(ast, leaves, [], []).get(())
    if cell is None:
        return False, 0.0, -1
    return True, cell.value, (cell.tags["leaf"] if cell.tags else -1)


def test_cell_function_matches_the_restatement():
    L = _lib()
    rng = np.random.default_rng(20240611)
    names = ("a", "b", "c")
    ncells = 1000
    total = 0
    for formula in PROGRAMS:
        ast = fr.parse(formula)
        present = (rng.random((ncells, 3)) < 0.7).astype(np.uint8)
        value = rng.normal(0, 1e3, (ncells, 3))
        pick = rng.random((ncells, 3)) < 0.35
        value[pick] = rng.choice(SPECIAL, int(pick.sum()))
        value[rng.random((ncells, 3)) < 0.1] = 7.0          # equal operands: a - b = 0 exactly
        src = np.tile(np.arange(3, dtype=np.int32), (ncells, 1))
        op = np.zeros(ncells, np.uint8)
        ov = np.zeros(ncells, np.float64)
        os_ = np.zeros(ncells, np.int32)
        rc = L.lk_formula_eval_cell(formula.encode(), _names(names), 3, ncells, present.ctypes.data, value.ctypes.data,
                                    src.ctypes.data, op.ctypes.data, ov.ctypes.data, os_.ctypes.data)
        assert rc == 0, formula
        for i in range(ncells):
            wp, wv, ws = _python_cell(ast, present[i], value[i].tolist(), names)
            assert bool(op[i]) == wp, (formula, i, present[i], value[i])
            if wp:
                assert struct.pack("<d", ov[i]) == struct.pack("<d", wv) or (math.isnan(ov[i]) and math.isnan(wv)), \
                    (formula, i, present[i], value[i], ov[i], wv)
                assert int(os_[i]) == ws, (formula, i, present[i], value[i], int(os_[i]), ws)
        total += ncells
    assert total >= 10_000 and len(PROGRAMS) >= 12


def test_cell_rules_by_hand():
    """The presence rules of Formula.scala:41-63, one by one."""
    names = ("a", "b")

    def run(formula, pa, va, pb, vb):
        ast = fr.parse(formula)
        present = np.array([[pa, pb]], np.uint8)
        value = np.array([[va, vb]], np.float64)
        src = np.array([[0, 1]], np.int32)
        op, ov, os_ = np.zeros(1, np.uint8), np.zeros(1), np.zeros(1, np.int32)
        assert _lib().lk_formula_eval_cell(formula.encode(), _names(names), 2, 1, present.ctypes.data, value.ctypes.data,
                                           src.ctypes.data, op.ctypes.data, ov.ctypes.data, os_.ctypes.data) == 0
        want = _python_cell(ast, [pa, pb], [va, vb], names)
        got = (bool(op[0]), float(ov[0]), int(os_[0])) if op[0] else (False, 0.0, -1)
        assert got[0] == want[0] and got[2] == want[2] and (fr.same_value(got[1], want[1]))
        return got

    assert run("a + b", 1, 2.0, 0, 0.0) == (True, 2.0, 0)            # b filled with 0, a's tags
    assert run("a + b", 0, 0.0, 1, 3.0) == (True, 3.0, 1)            # a filled: b's tags
    assert run("a - b", 1, 2.0, 0, 0.0)[0] is False                  # every other operator drops the key
    assert run("a * b", 0, 2.0, 1, 1.0)[0] is False
    assert run("a / b", 1, 2.0, 1, 0.0)[0] is False                  # division by +0.0 and -0.0: no row
    assert run("a / b", 1, 2.0, 1, -0.0)[0] is False
    got = run("a / b", 1, 2.0, 1, math.nan)                          # NaN != 0: flows through
    assert got[0] and math.isnan(got[1])
    assert run("100 * a", 1, 2.0, 0, 0.0) == (True, 200.0, -1)       # tags of e1, a constant
    assert run("a * 100", 1, 2.0, 0, 0.0) == (True, 200.0, 0)
    assert run("5 + a", 0, 0.0, 1, 0.0) == (True, 5.0, -1)           # a constant is present wherever the cell exists
    assert run("a + b", 0, 0.0, 0, 0.0)[0] is False
    assert fr.bits(run("a + b", 0, 0.0, 1, -0.0)[1]) == fr.bits(0.0)  # 0 + -0.0 = +0.0


def test_labels():
    """Formula.label (Formula.scala:71-80) over BaseExpr.label; a constant prints as Java's Double.toString."""
    from lakeside_amd import queryapi as qa
    svc = "resource.service.name"
    filt = {"k": "_cardinalhq.name", "v": ["m1"], "op": "eq"}
    a = {"id": "a", "dataset": "logs", "filter": filt, "chart": {"aggregation": "count", "groupBys": [svc]}}
    b = dict(a, id="b")
    exprs = {"a": a, "b": b}
    tags = {svc: "svc-003", "name": "m1"}
    want = "(resource.service.name = svc-003) / (resource.service.name = svc-003) * 100.0"
    assert qa.formula_label("a / b * 100", exprs, tags) == want
    assert fr.label(fr.parse("a / b * 100"), exprs, tags) == want
    a0 = dict(a, chart={"aggregation": "count", "groupBys": []})
    assert qa.formula_label("a / b * 100", {"a": a0, "b": a0}, {}) == \
        "(_cardinalhq.name = m1) / (_cardinalhq.name = m1) * 100.0"
    assert qa.formula_label("a * 0.0001", exprs, tags) == "(resource.service.name = svc-003) * 1.0E-4"
    assert qa.formula_label("(a - b) / (a + b)", exprs, {}) == "() - () / () + ()"     # labels carry no parentheses
    assert qa.formula_label("1e7 + a", {"a": a0}, {}) == "1.0E7 + (_cardinalhq.name = m1)"
    with pytest.raises(ValueError):
        qa.formula_label("a ^ 2", exprs, tags)
