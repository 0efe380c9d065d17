"""query-api side of an aggregate DataExpr over the HIP evaluator.

Mirrors, for one chart DataExpr over one SegmentGroup:
  QueryEngineV2.evaluateBaseExpr      query-api/src/main/scala/com/cardinal/queryapi/engine/QueryEngineV2.scala:271-308
  (fan-out + K-way mergeSortedSource  QueryEngineV2.scala:76-97, SegmentSequencer.scala:53-160)
  TimeGroupedSketchAggregator         core/src/main/scala/com/cardinal/eval/TimeGroupedSketchAggregator.scala:57-258
  BaseExpr.eval / getFromSketch       core/src/main/scala/com/cardinal/utils/ast/BaseExpr.scala:665-695, 86-93
  ASTUtils.getTransformerFunc / toGroupByKey / QueryClause.toString
                                      core/src/main/scala/com/cardinal/utils/ast/ASTUtils.scala:190-219, 87-89, 102-122
  BaseExpr.label                      BaseExpr.scala:697-716
  toGenericSSEPayload                 QueryEngineV2.scala:400-417

MI355X design: the worker fan-out, the K-way stream merge and the time-grouped sketch merge collapse into the
engine's merged table (LK_MERGED: one cell per (bucket, tags), globs and GPUs folded on the device, emitted in
ascending time).  AVG, which the reference runs as two pushdowns (SUM and COUNT) merged per (timestamp, tags)
into a {sum, count} map, is one scan: the table carries both and the merged value is Σsum / Σcount.  What is
left for the host is O(output rows): the future-timestamp drop, the chart transformer (vectorised), the
group-key collapse of BaseExpr.eval and the payload.
"""
import ctypes
import json
import os
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from ._lib import LK_MERGED

SUM, COUNT, MIN, MAX, AVG = "sum", "count", "min", "max", "avg"


def clause_string(q: dict) -> str:
    """QueryClause.toString (ASTUtils.scala:102-122) of a filter JSON node (parsed as ASTUtils.handleFilter,
    ASTUtils.scala:379-417: `not`, leaf, or a binary node whose non-text members fold left)."""
    if q.get("not") is not None:
        return f"not({clause_string(q['not'])})"
    if q.get("k") is not None:
        k, v, op = q["k"], list(q.get("v") or []), q.get("op")
        if op in ("eq", "gt", "ge", "lt", "le"):
            sym = {"eq": "=", "gt": ">", "ge": ">=", "lt": "<", "le": "<="}[op]
            return f"{k} {sym} {v[0]}"
        if op == "regex":
            return f"regexMatches({k}, {v[0]})"
        if op == "contains":
            return f"{k} contains {v[0]}"
        if op == "in":
            return f"{k} in ({', '.join(v)})"
        return ""
    children = [c for c in q.values() if not isinstance(c, str)]
    s = clause_string(children[0])
    for c in children[1:]:
        s = f"({s} {q['op']} {clause_string(c)})"
    return s


def label(base_expr: dict, tags: Dict[str, str]) -> str:
    """BaseExpr.label (BaseExpr.scala:697-716)."""
    gbs = sorted(set((base_expr.get("chart") or {}).get("groupBys") or []))
    if gbs:
        inner = ", ".join(f"{k} = {tags[k]}" for k in gbs if k in tags)
    else:
        inner = clause_string(base_expr["filter"])
    return f"({inner})"


def group_by_key(group_bys: Sequence[str], tags: Dict[str, str]) -> str:
    """ASTUtils.toGroupByKey (ASTUtils.scala:87-89); "default" without groupBys (BaseExpr.scala:689-690)."""
    gbs = sorted(set(group_bys))
    if not gbs:
        return "default"
    return ":".join(str(tags.get(k, "")) for k in gbs)


def _chart_type(s: Optional[str]) -> str:
    """ChartType.fromStr (core/.../model/query/common/ChartType.scala:41-47); default "count"
    (ASTUtils.scala:350)."""
    t = (s if s is not None else "count").lower().strip()
    if t not in ("count", "rate"):
        raise ValueError(f"Unknown chart type {s}!")
    return t


def _metric_type(s: Optional[str]) -> str:
    """MetricType.fromStr (core/.../model/query/common/MetricType.scala:65-73; METRIC_TYPE_* at
    core/.../utils/Commons.scala:49-52); default gauge (ASTUtils.scala:298-303)."""
    t = (s if s is not None else "gauge").lower().strip()
    if t == "rate":
        return "rate"
    if t in ("count", "counter"):
        return "counter"
    if t in ("gauge", "histogram"):
        return t
    raise ValueError(f"Unknown metric type {s}!")


def transformer(base_expr: dict, step_ms: int) -> Callable[[np.ndarray], np.ndarray]:
    """ASTUtils.getTransformerFunc (ASTUtils.scala:190-219), vectorised.  The step in seconds is the Long
    quotient stepInMillis / 1000; IEEE division (x / 0 = ±inf / NaN) as on the JVM."""
    chart = base_expr.get("chart") or {}
    ct = _chart_type(chart.get("type"))
    mt = _metric_type(base_expr.get("metricType"))
    secs = np.float64(int(step_ms) // 1000)

    def div(v):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.asarray(v, np.float64) / secs

    if base_expr.get("dataset", "metrics") == "metrics":
        if ct == "count" and mt == "rate":
            return lambda v: np.asarray(v, np.float64) * secs
        if ct == "rate" and mt == "counter":
            return div
        return lambda v: np.asarray(v, np.float64)
    if ct == "rate":
        return div
    return lambda v: np.asarray(v, np.float64)


def eval_merged_rows(base_expr: dict, ts: np.ndarray, values: np.ndarray, tags: Sequence[Dict[str, str]],
                     step_ms: int, now_ms: Optional[int] = None) -> List[dict]:
    """Merged (timestamp, value, tags) rows, ascending in time (one per time-grouped sketch merger cell) ->
    the `timeseries` payloads query-api streams to the client.

      * TimeGroupedSketchAggregator.onPush (TimeGroupedSketchAggregator.scala:200-222): a timestamp later than
        now is dropped ("future"); with ascending input the "old" drop never fires;
      * BaseExpr.eval (BaseExpr.scala:665-695): value = transformer(getFromSketch(map, aggregation)); results of
        one timestamp are keyed by toGroupByKey (sorted groupBy values joined with ":") or "default", a later
        row overwriting an earlier one under the same key.  The reference's order among rows of one
        timestamp is the iteration order of a hash map; here the row with the smallest sorted tag list wins
        (deterministic), and payloads of one timestamp come out in key order.
    """
    now = int(time.time() * 1000) if now_ms is None else int(now_ms)
    gbs = (base_expr.get("chart") or {}).get("groupBys") or []
    expr_id = base_expr.get("id", "_")
    vals = transformer(base_expr, step_ms)(values)
    out: List[dict] = []
    n = len(ts)
    i = 0
    while i < n:
        t = int(ts[i])
        j = i
        while j < n and int(ts[j]) == t:
            j += 1
        if t <= now:
            best: Dict[str, tuple] = {}
            for r in range(i, j):
                key = group_by_key(gbs, tags[r])
                rank = sorted(tags[r].items())
                if key not in best or rank < best[key][0]:
                    best[key] = (rank, r)
            for key in sorted(best):
                r = best[key][1]
                out.append({"id": expr_id, "type": "timeseries",
                            "message": {"timestamp": t, "tags": dict(tags[r]), "value": float(vals[r]),
                                        "label": label(base_expr, tags[r])}})
        i = j
    return out


def evaluate_base_expr(engine, base_expr: dict, segment_requests: Sequence[dict], paths: Sequence[str],
                       step_ms: int, glob_size: int = 10, now_ms: Optional[int] = None,
                       shard: Optional[Sequence[int]] = None, distributed: bool = False) -> List[dict]:
    """QueryEngineV2.evaluateBaseExpr (QueryEngineV2.scala:271-308) for one SegmentGroup, then
    toGenericSSEPayload (400-417): one merged evaluation on the engine (lk_eval_pushdown LK_MERGED, or the
    sharded lk_eval_pushdown_dist whose rank 0 alone gets rows), then eval_merged_rows."""
    req = json.dumps({"baseExpr": base_expr, "segmentRequests": list(segment_requests), "reverseSort": False,
                      "isTagQuery": False})
    if distributed:
        res = engine.eval_pushdown_dist(req, list(paths), shard, glob_size)
    else:
        res = engine.eval_pushdown(req, list(paths), glob_size, LK_MERGED)
    return eval_merged_rows(base_expr, res.ts, res.values, res.tags, step_ms, now_ms)


_TEXT = None


def _text_lib():
    """liblakeside_text.so: the formula parser the engine links and Java's Double.toString (host only)."""
    global _TEXT
    if _TEXT is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "liblakeside_text.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `make`")
        L = ctypes.CDLL(path)
        L.lk_formula_plan.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_char_p,
                                      ctypes.c_size_t]
        L.lk_formula_plan.restype = ctypes.c_int
        _TEXT = L
    return _TEXT


def formula_plan(formula: str, names: Sequence[str]) -> List[str]:
    """The formula's postfix program over the variables `names` (lk_formula_plan): `$<i>`, a constant as Java prints
    it, `+ - * /`.  ValueError on a formula the engine refuses."""
    arr = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
    out = ctypes.create_string_buffer(8192)
    rc = _text_lib().lk_formula_plan(formula.encode(), arr, len(names), out, len(out))
    if rc != 0:
        raise ValueError(f"formula error {rc}: {out.value.decode()}")
    return out.value.decode().split(" ")


def formula_label(formula: str, base_expressions: Dict[str, dict], tags: Dict[str, str]) -> str:
    """Formula.label (Formula.scala:71-80): "<e1Label> <op> <e2Label>" with + - * /, recursively and without
    parentheses; ConstantExpr.label is Java's Double.toString of the value; BaseExpr.label is `label`."""
    names = list(base_expressions)
    stack: List[str] = []
    for tok in formula_plan(formula, names):
        if tok in ("+", "-", "*", "/"):
            e2 = stack.pop()
            e1 = stack.pop()
            stack.append(f"{e1} {tok} {e2}")
        elif tok.startswith("$"):
            stack.append(label(base_expressions[names[int(tok[1:])]], tags))
        else:
            stack.append(tok)
    return stack[0]


def evaluate_formula(engine, base_expressions: Dict[str, dict], formula: str,
                     segment_requests_by_id: Dict[str, Sequence[dict]], paths_by_id: Dict[str, Sequence[str]],
                     step_ms: int, glob_size: int = 10, now_ms: Optional[int] = None, distributed: bool = False,
                     shard_by_id: Optional[Dict[str, Sequence[int]]] = None) -> List[dict]:
    """QueryEngineV2.evaluateFormula (QueryEngineV2.scala:310-389) for one SegmentGroup, then toGenericSSEPayload
    (400-417) with id = the formula text (387): one lk_eval_formula call -- the base expressions are evaluated and
    joined per (timestamp, group key) on the device, only the combined rows come back -- then the future-timestamp
    drop (TimeGroupedSketchAggregator.scala:200-222; the leaf and the formula pass both drop per timestamp, so
    dropping last is the same) and the payloads.  Payloads of one timestamp come out in key order.
    distributed: one lk_eval_formula_dist call, every rank of the engine's communicator making it with the same
    arguments; `shard_by_id[name]` gives the rank of every path of that expression (absent: i % world).  Rank 0 returns
    the payloads, every other rank []."""
    now = int(time.time() * 1000) if now_ms is None else int(now_ms)
    for be in base_expressions.values():   # the engine applies the leaves' transformers: same step, checked here
        transformer(be, step_ms)
    exprs = {}
    for name, be in base_expressions.items():
        exprs[name] = {"pushDown": {"baseExpr": be, "segmentRequests": list(segment_requests_by_id[name]),
                                    "reverseSort": False, "isTagQuery": False},
                       "paths": list(paths_by_id[name])}
        if distributed and shard_by_id and shard_by_id.get(name) is not None:
            exprs[name]["shard"] = list(shard_by_id[name])
    res = engine.eval_formula_dist(formula, exprs, glob_size) if distributed else engine.eval_formula(formula, exprs, glob_size)
    gbs = sorted({g for be in base_expressions.values() for g in ((be.get("chart") or {}).get("groupBys") or [])})
    rows = [(int(t), tuple(tg.get(g, "") for g in gbs), float(v), tg)
            for t, v, tg in zip(res.ts, res.values, res.tags) if int(t) <= now]
    rows.sort(key=lambda r: (r[0], r[1]))
    return [{"id": formula, "type": "timeseries",
             "message": {"timestamp": t, "tags": dict(tg), "value": v, "label": formula_label(formula, base_expressions, tg)}}
            for t, _, v, tg in rows]


def _filter_leaves(q: dict):
    """The leaves of a filter JSON node (ASTUtils.handleFilter's shapes: `not`, leaf, binary node)."""
    if q.get("not") is not None:
        yield from _filter_leaves(q["not"])
    elif q.get("k") is not None:
        yield q
    else:
        for c in q.values():
            if isinstance(c, dict):
                yield from _filter_leaves(c)


def is_tag_synthetic(base_expr: dict, tag_name: str) -> bool:
    """BaseExpr.isTagSynthetic (BaseExpr.scala:146-157): the tag is an extracted or computed field of the filter."""
    return any(f["k"] == tag_name and (f.get("extracted") or f.get("computed"))
               for f in _filter_leaves(base_expr["filter"]))


def evaluate_tag_query(engine, base_expr: dict, segment_requests: Sequence[dict], paths: Sequence[str],
                       tag_data_type: Optional[dict] = None, limit: int = 1000, glob_size: int = 10) -> List[dict]:
    """QueryEngineV2.evaluateTagQuery (QueryEngineV2.scala:419-491) for one SegmentGroup: with a tagDataType
    ({"tagName", "dataType"}) whose tag is not synthetic the filter is ANDed with `exists` on the tag; the chart is
    dropped; the pushdown carries isTagQuery and processor.tagNameCompressionEnabled.  Yields each row's tags map (the
    GenericSSEPayload message), at most `limit` of them (QueryApi's take(limit)).  Without a tagDataType this is the
    tag-name query: the engine returns every tag name once, on the first passing row that holds a value for it, rows of
    a glob in file order and globs in request order (include/lakeside_gpu.h)."""
    be = dict(base_expr)
    if tag_data_type is not None and not is_tag_synthetic(be, tag_data_type["tagName"]):
        be["filter"] = {"q1": be["filter"],
                        "q2": {"k": tag_data_type["tagName"], "v": [], "op": "exists",
                               "dataType": tag_data_type.get("dataType", "string"), "extracted": False, "computed": False},
                        "op": "and"}
    be.pop("chart", None)
    req = {"baseExpr": be, "segmentRequests": list(segment_requests), "reverseSort": False, "isTagQuery": True,
           "processor": {"tagNameCompressionEnabled": True}}
    if tag_data_type is not None:
        req["tagDataType"] = {"tagName": tag_data_type["tagName"], "dataType": tag_data_type.get("dataType", "string")}
    res = engine.eval_pushdown(json.dumps(req), list(paths), glob_size, LK_MERGED)
    return [{"message": dict(t)} for t in res.tags[:max(0, int(limit))]]


__all__ = ["clause_string", "label", "group_by_key", "transformer", "eval_merged_rows", "evaluate_base_expr",
           "formula_plan", "formula_label", "evaluate_formula", "is_tag_synthetic", "evaluate_tag_query"]
