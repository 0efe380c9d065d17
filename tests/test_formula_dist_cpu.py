"""lk_eval_formula_dist, the parts that need no GPU: the header declares it, the library exports it, bad arguments are
status codes, and the Python layers carry it (Engine.eval_formula_dist, queryapi.evaluate_formula's distributed /
shard_by_id)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lakeside_gpu.h")


def test_header_declares_the_entry():
    text = open(HEADER).read()
    m = re.search(r"int\s+lk_eval_formula_dist\s*\(([^)]*)\)\s*;", text)
    assert m, "include/lakeside_gpu.h does not declare lk_eval_formula_dist"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["lk_engine* e", "const char* formula_json", "int glob_size", "lk_result** out"]
    # the comment cites the Scala it replaces, as the other entries do
    head = text[:m.start()]
    comment = head[head.rindex("/*"):]
    assert "QueryEngineV2.scala:310-389" in comment and "Formula.scala" in comment


def test_library_exports_and_binds_it():
    from lakeside_amd import _lib
    assert hasattr(_lib.lib(), "lk_eval_formula_dist")
    assert "lk_eval_formula_dist" in {name for name, _, _ in _lib.SIGNATURES}


def test_bad_arguments_are_status_codes():
    from lakeside_amd import _lib
    assert _lib.lib().lk_eval_formula_dist(None, b"{}", 10, None) == _lib.LK_ERR_ARG


def test_python_layers_carry_it():
    from lakeside_amd import queryapi
    from lakeside_amd.evaluator import Engine
    assert list(inspect.signature(Engine.eval_formula_dist).parameters) == ["self", "formula", "expressions", "glob_size"]
    p = inspect.signature(queryapi.evaluate_formula).parameters
    assert p["distributed"].default is False and p["shard_by_id"].default is None
