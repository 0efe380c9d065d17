"""DDSketch bins on the MI355X at the index boundaries and the edges of the mapping's range, on every route a value takes
into a sketch (families, classes and files: tests/sketch_data.py, checked on the CPU in tests/test_sketch_cpu.py):

  tiles    logs `p50` by attr.case: scan_tiles bins every row (dd_bin), hash table, no general segment
  rows     the same grouped by attr.case and the INT64 column attr.n: every segment takes the general row scan (ex_scan,
           dd_bin again).  A numeric comparison leaf would do the same but is refused in sketch queries (asserted below),
           so the numeric groupBy is the request that reaches this statement of the mapping.
  metrics  the metrics twin: MAX(rollup) per (timestamp, name, case) on the device, dd::Sketch::accept on the host

Every decided value must sit alone in bin floor(x) of its sign, every crossing value in k - 1 or k, with x from `decimal`
(no tolerance; the oracle's side of an undecided boundary is not demanded).  An untrackable value (NaN, +-inf, a
magnitude beyond MAX_INDEXABLE) fails the call on every route when it passes the filter and the window, and only then."""
import collections
import json

import numpy as np
import pytest

from oracle import ddsketch as dd
from tests import sketch_data as sd
from tests.parity import assert_rows_equal

pytestmark = pytest.mark.gpu

ROUTES = ["tiles", "rows", "metrics"]
GLOB = 4
BROAD_FILES = 8


def _segs(n, route, start=None, end=None):
    from lakeside_amd import synth
    metrics = route == "metrics"
    segs = [synth.segment_request(i, step=sd.METRICS_STEP if metrics else sd.STEP, hour=0,
                                  dataset="metrics" if metrics else "logs") for i in range(n)]
    for s in segs:
        if start is not None:
            s["startTs"], s["endTs"] = start, end
    return segs


def _names(route, names):
    """The name filter: `probe` stands for the metrics twin's four probe names."""
    from lakeside_amd import synth
    out = []
    for n in names:
        out += sd.METRIC_NAMES if (n == sd.PROBE and route == "metrics") else [n]
    return synth.leaf(synth.NAME, "eq" if len(out) == 1 else "in", *out), set(out)


def _request(route, agg, filt, nsegs, start=None, end=None):
    from lakeside_amd import synth
    gbs = [sd.CASE, sd.NUM] if route == "rows" else [sd.CASE]
    d = synth.pushdown(filt, _segs(nsegs, route, start, end), agg, gbs, dataset="metrics" if route == "metrics" else "logs")
    if route != "metrics" and agg[0] == "p":
        d["baseExpr"]["chart"]["rollup"] = agg
    return json.dumps(d)


def _route_stats(route, st, nsegs, passing_rows=None):
    assert st["segments"] == nsegs, st
    if route == "tiles":
        assert st["general_segments"] == 0 and st["table"] == "hash", st
    elif route == "rows":
        assert st["general_segments"] == nsegs and st["table"] == "hash", st
    else:
        assert "metrics_pct_rows_in" in st and (passing_rows is None or st["metrics_pct_rows_in"] == passing_rows), st


def _case_of(route, tags):
    want = {sd.CASE, sd.NUM} if route == "rows" else {sd.CASE}
    assert set(tags) == want and (route != "rows" or tags[sd.NUM] == str(sd.NUM_VALUE)), tags
    return tags[sd.CASE]


@pytest.fixture(scope="module")
def files(engine, tmp_path_factory):
    """One boundary + edge + wide file and the broad family's files, as logs and as metrics twins, loaded once."""
    root = tmp_path_factory.mktemp("sketch_bins")
    out = {}
    probes = sd.wide_probes() + sd.boundary_probes() + sd.edge_probes()   # wide first: one timestamp, one bucket
    broad = sd.broad_probes()
    per = (len(broad) + BROAD_FILES - 1) // BROAD_FILES
    for kind, metrics in (("logs", False), ("metrics", True)):
        rows_of = sd.metrics_rows if metrics else sd.logs_rows
        rows = rows_of(probes)
        out[kind, "boundary"] = ([sd.write_file(root / f"{kind}_boundary.parquet", rows, metrics)], [rows])
        chunks = [broad] if metrics else [broad[i:i + per] for i in range(0, len(broad), per)]
        rws = [rows_of(c) for c in chunks]
        out[kind, "broad"] = ([sd.write_file(root / f"{kind}_broad{i}.parquet", r, metrics) for i, r in enumerate(rws)], rws)
    for paths, _ in out.values():
        for p in paths:
            engine.load_segment(p)
    return out


def _files(files, route, family):
    return files["metrics" if route == "metrics" else "logs", family]


def _sketch_rows(res, route, per_glob=False):
    """[(glob, ts, case, value, decoded sketch)] of a percentile result (glob 0 for merged rows)."""
    globs = np.asarray(res.globs).tolist() if per_glob else [0] * len(res)
    tags = res.tags
    return [(globs[r], int(res.ts[r]), _case_of(route, tags[r]), float(res.values[r]), dd.decode(res.sketch(r)))
            for r in range(len(res))]


def _expected(rows_per_file, names, route, glob_size, win=None):
    """Per glob {(sketch ts, case): [probe | None]}; the last entry is the merged map (sketches merge per (ts, tags))."""
    step = None if route == "metrics" else sd.STEP
    per_glob = []
    for g in range(0, len(rows_per_file), glob_size):
        rows = [r for f in rows_per_file[g:g + glob_size] for r in f]
        per_glob.append(sd.expected_sketches(rows, names, step, win))
    merged = collections.defaultdict(list)
    for e in per_glob:
        for k, v in e.items():
            merged[k] += v
    return per_glob, dict(merged)


def _check_rows(route, got, want, q, label, single):
    """`got`: [(ts, case, value, sketch)] of one glob or of the merged result; `want`: {(ts, case): [probe | None]}."""
    assert sorted((ts, case) for ts, case, _, _ in got) == sorted(want), f"{label}: row keys differ"
    filler_bin = sd.classify(sd.FILLER_VALUE)
    assert filler_bin.kind == "decided"
    for ts, case, val, sk in got:
        entries = want[(ts, case)]
        if case == sd.FILLER:
            assert all(e is None for e in entries)
            assert sk.bins() == ({filler_bin.index: float(len(entries))}, {}, 0.0), (label, ts, sk.bins())
            assert val == dd.value(filler_bin.index), (label, ts, val)
            continue
        sd.match_sketch(sk, entries, f"{label} {case}")
        if single and case != sd.WIDE_CASE:
            assert len(entries) == 1 and sk.count() == 1.0, (label, case)
        if sk.count() == 1.0:   # the count is 1: any q returns the bin's value
            pos, neg, zero = sk.bins()
            w = 0.0 if zero else (-dd.value(next(iter(neg))) if neg else dd.value(next(iter(pos))))
            assert sd.bits(val) == sd.bits(w), (label, case, val, w)
        else:
            assert sd.bits(val) == sd.bits(sk.quantile(q)), (label, case, val, sk.quantile(q))


@pytest.mark.parametrize("listing", ["sparse", "dense"])
@pytest.mark.parametrize("route", ROUTES)
def test_boundaries_and_edges(engine, files, route, listing):
    """Every boundary and edge probe alone in its sketch, per glob and merged, and the wide case's two bins.  `sparse`
    filters on the probe names (1 row in 16 passes in a logs tile), `dense` adds `filler` (every row passes): the two
    listings of the passing rows in scan_tiles' late stage.  (The metrics twin's rows never reach that stage: its two
    runs differ in the MAX rows handed to the host.)"""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    names = [sd.PROBE] if listing == "sparse" else [sd.PROBE, sd.FILLER]
    paths, rows = _files(files, route, "boundary")
    filt, nameset = _names(route, names)
    per_glob, merged = _expected(rows, nameset, route, GLOB)
    passing = sum(1 for r in rows[0] if r.name in nameset)
    req = _request(route, "p50", filt, len(paths))
    res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
    _route_stats(route, res.stats, len(paths), passing)
    got = _sketch_rows(res, route, per_glob=True)
    assert {r[0] for r in got} == {0}
    _check_rows(route, [r[1:] for r in got], per_glob[0], 0.5, f"{route} {listing} glob 0", single=True)
    mg = engine.eval_pushdown(req, paths, GLOB, LK_MERGED)
    _route_stats(route, mg.stats, len(paths), passing)
    mrows = [r[1:] for r in _sketch_rows(mg, route)]
    _check_rows(route, mrows, merged, 0.5, f"{route} {listing} merged", single=True)
    # the wide sketch: the first and the last index in one store of kmax - kmin + 1 packed doubles
    kmin, kmax = sd.index_range()
    wide = [r for r in range(len(mg)) if mrows[r][1] == sd.WIDE_CASE]
    assert len(wide) == 1
    assert mrows[wide[0]][3].bins() == ({kmin: 1.0, kmax: 1.0}, {}, 0.0)
    assert len(mg.sketch(wide[0])) > 8 * (kmax - kmin + 1)
    assert mrows[wide[0]][2] == dd.value(kmin)          # p50 of two values: rank 0.5, the first bin


@pytest.mark.parametrize("route", ROUTES)
def test_broad_family(engine, files, route):
    """4,000 decided magnitudes over the whole range under 16 case tags: every sketch decodes to exactly the `decimal`
    floor's bins and counts; p0 / p50 / p99.9 / p100 equal the oracle's quantile of those bins bit for bit."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS
    paths, rows = _files(files, route, "broad")
    filt, nameset = _names(route, [sd.PROBE, sd.FILLER] if route == "tiles" else [sd.PROBE])
    per_glob, merged = _expected(rows, nameset, route, GLOB)
    assert len({case for _, case in merged} - {sd.FILLER}) == 2 * sd.BROAD_BANDS
    for agg in ("p0", "p50", "p99.9", "p100"):
        q = float(agg[1:]) / 100.0
        req = _request(route, agg, filt, len(paths))
        if agg == "p50":
            res = engine.eval_pushdown(req, paths, GLOB, LK_PER_GLOB_ROWS)
            _route_stats(route, res.stats, len(paths))
            got = _sketch_rows(res, route, per_glob=True)
            for gi, want in enumerate(per_glob):
                _check_broad([r[1:] for r in got if r[0] == gi], want, q, f"{route} broad {agg} glob {gi}")
        mg = engine.eval_pushdown(req, paths, GLOB, LK_MERGED)
        _route_stats(route, mg.stats, len(paths))
        _check_broad([r[1:] for r in _sketch_rows(mg, route)], merged, q, f"{route} broad {agg} merged")


def _check_broad(got, want, q, label):
    assert sorted((ts, case) for ts, case, _, _ in got) == sorted(want), f"{label}: row keys differ"
    nvals = 0
    for ts, case, val, sk in got:
        entries = want[(ts, case)]
        if case == sd.FILLER:
            entries = [sd.Probe(sd.FILLER, sd.FILLER_VALUE, sd.classify(sd.FILLER_VALUE))] * len(entries)
        pos, neg, zero = sd.bins_of(entries)
        assert sk.bins() == (pos, neg, zero), (label, ts, case)
        o = dd.Sketch()
        o.pos, o.neg, o.zero = pos, neg, zero
        assert sd.bits(val) == sd.bits(o.quantile(q)), (label, ts, case, val, o.quantile(q))
        nvals += len(entries) if case != sd.FILLER else 0
    return nvals


# ---- untrackable values ----

@pytest.fixture(scope="module")
def bad_files(engine, tmp_path_factory):
    """Per untrackable value one small file: as logs, as the VARCHAR twin of attr.n the oracle reads for the `rows`
    route, and as a metrics twin."""
    root = tmp_path_factory.mktemp("sketch_untrackable")
    out = {}
    for tag, v in sd.UNTRACKABLE:
        logs = sd.untrackable_rows(v)
        met = sd.untrackable_rows(v, metrics=True)
        out[tag] = {"logs": sd.write_file(root / f"{tag}_logs.parquet", logs),
                    "twin": sd.write_file(root / f"{tag}_twin.parquet", logs, num_as_text=True),
                    "metrics": sd.write_file(root / f"{tag}_metrics.parquet", met, metrics=True)}
        engine.load_segment(out[tag]["logs"])
        engine.load_segment(out[tag]["metrics"])
    return out


def _pct_rows(res, route):
    return [(int(res.ts[r]), res.tags[r], float(res.values[r]), res.sketch(r)) for r in range(len(res))]


@pytest.mark.parametrize("tag", [t for t, _ in sd.UNTRACKABLE])
@pytest.mark.parametrize("route", ROUTES)
def test_untrackable(engine, bad_files, route, tag):
    """An untrackable row that passes the filter and the window fails the call (LK_ERR_ARG; the worker answers empty
    globs; the oracle raises); dropped by the filter or by the window it does not; sum / count never mind it."""
    from lakeside_amd import LK_MERGED, LK_PER_GLOB_ROWS, _lib, synth
    from lakeside_amd.evaluator import evaluate_push_down_request
    from oracle import dataexpr as dx
    from tests.test_gpu_features import _pct_rows_equal
    f = bad_files[tag]
    path = f["metrics" if route == "metrics" else "logs"]
    opath = {"tiles": f["logs"], "rows": f["twin"], "metrics": f["metrics"]}[route]
    both = synth.leaf(synth.NAME, "in", sd.GOOD, sd.BAD)
    good = synth.leaf(synth.NAME, "eq", sd.GOOD)

    # 1. the bad row passes
    req = _request(route, "p50", both, 1)
    for flags in (LK_PER_GLOB_ROWS, LK_MERGED):
        with pytest.raises(_lib.LakesideError) as ei:
            engine.eval_pushdown(req, [path], GLOB, flags)
        assert ei.value.code == _lib.LK_ERR_ARG and "trackable" in str(ei.value), ei.value
    assert evaluate_push_down_request(engine, "q", True, req, [path]) == [[]]
    with pytest.raises(ValueError):
        dx.evaluate_percentile_per_glob(dx.parse_pushdown(req), GLOB, [opath])

    # 2. the filter drops it; 3. the window ends at its timestamp
    for label, req in (("filter", _request(route, "p50", good, 1)),
                       ("window", _request(route, "p50", both, 1, synth.T0, synth.T0 + sd.BAD_TS_OFFSET))):
        pr = dx.parse_pushdown(req)
        want = dx.evaluate_percentile_per_glob(pr, GLOB, [opath])
        assert len(want) == 1 and len(want[0]) >= 4
        res = engine.eval_pushdown(req, [path], GLOB, LK_PER_GLOB_ROWS)
        _route_stats(route, res.stats, 1)
        _pct_rows_equal(_pct_rows(res, route), want[0], 0.5, f"{route} {tag} {label} glob 0")
        mg = engine.eval_pushdown(req, [path], GLOB, LK_MERGED)
        _pct_rows_equal(_pct_rows(mg, route), dx.merge_percentile(pr, want), 0.5, f"{route} {tag} {label} merged")

    # 4. the flag is a sketch matter only
    for agg in ("sum", "count"):
        req = _request(route, agg, both, 1)
        pr = dx.parse_pushdown(req)
        cells = dx.evaluate_glob_cells(pr, GLOB, [opath])
        res = engine.eval_pushdown(req, [path], GLOB, LK_PER_GLOB_ROWS)
        assert_rows_equal(res.per_glob(1)[0], [(c.ts, c.agg_value(agg), c.tags) for c in cells[0]], agg,
                          f"{route} {tag} {agg}")
        assert any(t.get(sd.CASE) == sd.BAD for t in res.tags)


def test_numeric_leaf_is_refused_in_sketch_queries(engine, files):
    """Why the `rows` route groups by a numeric column: a numeric comparison leaf is refused before any scan."""
    from lakeside_amd import LK_PER_GLOB_ROWS, _lib, synth
    paths, _ = _files(files, "tiles", "boundary")
    leaf = {"k": sd.NUM, "v": ["0"], "op": "ge", "extracted": False, "computed": False, "dataType": "number"}
    filt = {"op": "and", "q1": synth.leaf(synth.NAME, "eq", sd.PROBE), "q2": leaf}
    with pytest.raises(_lib.LakesideError) as ei:
        engine.eval_pushdown(_request("tiles", "p50", filt, 1), paths, GLOB, LK_PER_GLOB_ROWS)
    assert ei.value.code == _lib.LK_ERR_UNSUPPORTED and "numeric comparison leaves in sketch queries" in str(ei.value)


def test_sites_report(engine, files):
    """Prints, per site, at how many crossing values its index differs from floor(x), and where two sites differ from
    each other (a logs percentile and a metrics percentile over one value may then land one bin apart: allowed, but
    known).  Two pairs of sites run one statement over the same inputs and must agree: the two kernels (dd_bin), and the
    metrics route with dd::Sketch::accept called directly (lk_dd_sim)."""
    from lakeside_amd import LK_MERGED
    ps = {p.case: p for p in sd.boundary_probes() if p.cls.kind == "crossing"}
    sites = {}
    for route in ROUTES:
        paths, _ = _files(files, route, "boundary")
        filt, _ = _names(route, [sd.PROBE])
        mg = engine.eval_pushdown(_request(route, "p50", filt, len(paths)), paths, GLOB, LK_MERGED)
        found = {}
        for _, _, case, _, sk in _sketch_rows(mg, route):
            if case in ps:
                (i,) = list(sk.neg if ps[case].value < 0 else sk.pos)
                found[case] = i
        assert set(found) == set(ps)
        sites[route] = found
    vals = np.array([abs(p.value) for p in ps.values()])
    sites["oracle"] = dict(zip(ps, dd.index(vals).tolist()))
    sites["host"] = {c: next(iter(dd.decode(sd.host_sketch([abs(p.value)]).blob).pos)) for c, p in ps.items()}
    for site, found in sites.items():
        off = sorted(c for c, i in found.items() if i != ps[c].cls.floor)
        print(f"SITE {site}: {len(off)} of {len(ps)} crossing values off floor(x)")
    names = list(sites)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            diff = sorted(c for c in ps if sites[a][c] != sites[b][c])
            print(f"SITES {a} vs {b}: {len(diff)} differ {diff[:12]}")
    assert sites["tiles"] == sites["rows"] and sites["metrics"] == sites["host"]
