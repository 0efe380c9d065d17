"""The DDSketch index mapping and the host's dd::Sketch without a GPU.

The value families of tests/sketch_data.py satisfy their own definitions, recomputed here independently of their builder
(another precision, rational margins); the oracle's index and the host's accept (the real dd::Sketch, through lk_dd_sim
of liblakeside_text.so) put every decided value in floor(x) and every crossing value in k - 1 or k; add_bin, quantile,
serialize and merge of the host sketch equal the oracle's and, independently of it, the exact order statistics."""
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import ddsketch as dd
from tests import sketch_data as sd

QS = [0.0, 0.001, 0.5, 0.95, 0.999, 1.0]
_CTX = decimal.Context(prec=90)


def _x(a):
    """x(a) as a rational, from an evaluation independent of sketch_data.x_of (90 digits)."""
    return Fraction(_CTX.multiply(_CTX.ln(decimal.Decimal(a)), decimal.Decimal(dd.MULTIPLIER)))


def _m(k):
    return Fraction(3) * Fraction(2) ** (math.frexp(abs(k))[1] - 1 - 52)   # frexp: |k| = f * 2^e, f in [0.5, 1)


def _class(a):
    if a == 1.0:
        return ("decided", 0)
    x = _x(a)
    k = round(x)
    return ("decided", math.floor(x)) if abs(x - k) >= _m(k or 1) else ("crossing", k)


def _up(a):
    return math.nextafter(a, math.inf)


def _down(a):
    return math.nextafter(a, 0.0)


def _decode_one(blob):
    """(sign, index) of a sketch that holds one count; ("zero", None) for the zero bin."""
    sk = dd.decode(blob)
    pos, neg, zero = sk.bins()
    assert sum(pos.values()) + sum(neg.values()) + zero == 1.0, (pos, neg, zero)
    if zero:
        return ("zero", None)
    return ("neg", next(iter(neg))) if neg else ("pos", next(iter(pos)))


def _all_probes():
    return sd.boundary_probes() + sd.edge_probes() + sd.broad_probes()


# ---- 1. the families ----

def test_index_range_and_ks():
    kmin, kmax = sd.index_range()
    assert kmin == math.floor(_x(sd.FIRST)) and kmax == math.floor(_x(sd.LAST))
    assert (kmin, kmax) == (-35418, 35486)
    ks = sd.boundary_ks()
    assert len(ks) == len(set(ks)) == 50 and kmin + 1 in ks and kmax in ks and 0 not in ks
    assert set(range(-8, 9)) - {0} <= set(ks)
    for k in (50, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096, 8191, 8192, 16384, 32767, 32768, 35000):
        assert k in ks and -k in ks
    # the margin covers the 2.1 ulp(x) a conforming site may be off by: an x within M of k has at most ulp(|k|)
    for k in ks:
        assert _m(k) >= Fraction(21, 10) * Fraction(math.ulp(float(abs(k))))
        assert math.frexp(abs(k) + float(_m(k)))[1] == math.frexp(abs(k))[1]          # k + M stays in k's binade
        assert Fraction(sd.margin(k)) == _m(k)


def test_boundary_family_definitions():
    for k in sd.boundary_ks():
        lo, b, c, hi = sd.boundary(k)
        m = _m(k)
        assert sd.FIRST <= lo <= b < c <= hi <= sd.LAST, k
        assert _x(lo) < k - m <= _x(_up(lo)), k
        assert _x(b) < k <= _x(c) and c == _up(b), k
        assert _x(_down(hi)) < k + m <= _x(hi), k
        assert _class(lo) == ("decided", k - 1) and _class(hi) == ("decided", k), k
        for a in (b, c):
            assert _class(a) in (("crossing", k), ("decided", k - 1 if a == b else k)), (k, a)
    for p in sd.boundary_probes():
        assert (p.cls.kind, p.cls.index) == _class(abs(p.value)), p
        assert p.cls.floor == math.floor(_x(abs(p.value))), p
    assert len(sd.boundary_probes()) == 50 * 4 * 2
    assert len({p.case for p in sd.boundary_probes() + sd.edge_probes()}) == 400 + len(sd.edge_probes())
    # small |k|: the window is below one ulp of a, lo / hi are b / c and decided; large |k|: thousands of ulps
    lo, b, c, hi = sd.boundary(1)
    assert (lo, hi) == (b, c)
    lo, b, c, hi = sd.boundary(35000)
    assert 4000 <= sd.bits(hi) - sd.bits(lo) <= 2 * 7500


def test_broad_family_is_decided():
    ps = sd.broad_probes()
    assert len(ps) == sd.BROAD_N and len({p.case for p in ps}) == 2 * sd.BROAD_BANDS
    assert sum(_class(abs(p.value))[0] == "crossing" for p in ps) == 0          # the cap is 0
    assert all(sd.FIRST <= abs(p.value) <= sd.LAST for p in ps)
    idx = [p.cls.index for p in ps]
    kmin, kmax = sd.index_range()
    assert min(idx) < kmin + 200 and max(idx) > kmax - 200                      # the whole range


def test_edge_classes():
    by = {p.case: p for p in sd.edge_probes()}
    kmin, kmax = sd.index_range()
    for s in "pn":
        for tag in ("zero.0", "zero.denorm", "zero.dblmin", "zero.below", "zero.minidx"):
            assert by[f"{tag}.{s}"].cls.kind == "zero"
        assert by[f"first.{s}"].cls == sd.Class("decided", kmin, kmin)
        assert by[f"last.{s}"].cls == sd.Class("decided", kmax, kmax)
        assert by[f"one.{s}"].cls.index == 0 and by[f"one.after.{s}"].cls == sd.Class("decided", 0, 0)
        assert by[f"one.before.{s}"].cls == sd.Class("decided", -1, -1)
    assert by["zero.null"].value is None and math.copysign(1.0, by["zero.0.n"].value) == -1.0
    assert all(p.cls.kind == "decided" for p in sd.wide_probes())


def test_oracle_index():
    ps = [p for p in _all_probes() if p.cls.kind != "zero"]
    got = dd.index(np.array([abs(p.value) for p in ps]))
    for p, i in zip(ps, got.tolist()):
        assert i in sd.allowed(p.cls), (p, i)
    crossing = [(p, i) for p, i in zip(ps, got.tolist()) if p.cls.kind == "crossing"]
    assert len(crossing) >= 100   # the tolerance is used: the family does hold undecided values
    print(f"oracle: {sum(i != p.cls.floor for p, i in crossing)} of {len(crossing)} crossing values off floor(x)")


# ---- 2. the host's accept ----

def test_host_constants():
    c = sd.host_sketch().consts
    want = [dd.GAMMA, dd.MULTIPLIER, dd.REL_ACC, dd.MIN_INDEXABLE, dd.MAX_INDEXABLE, sd.DD_BIAS, sd.DD_HALF, sd.DD_NBINS]
    assert [sd.bits(x) for x in c] == [sd.bits(float(x)) for x in want]
    kmin, kmax = sd.index_range()
    assert -sd.DD_BIAS <= kmin and kmax < sd.DD_BIAS


def test_host_accept_bins():
    off = n = 0
    for p in _all_probes():
        if p.value is None:
            continue
        h = sd.host_sketch([p.value])
        assert h.rejected is None and h.total == 1.0, p
        sign, i = _decode_one(h.blob)
        if p.cls.kind == "zero":
            assert sign == "zero", p
            continue
        assert sign == ("neg" if p.value < 0 else "pos") and i in sd.allowed(p.cls), (p, sign, i)
        if p.cls.kind == "crossing":
            n += 1
            off += i != p.cls.floor
    print(f"host accept: {off} of {n} crossing values off floor(x)")


def test_host_accept_equals_oracle_on_crossings():
    """Host and oracle both call glibc's log: the same side of every undecided boundary."""
    ps = [p for p in sd.boundary_probes() if p.cls.kind == "crossing"]
    want = dd.index(np.array([abs(p.value) for p in ps])).tolist()
    assert [_decode_one(sd.host_sketch([p.value]).blob)[1] for p in ps] == want


@pytest.mark.parametrize("tag,bad", sd.UNTRACKABLE)
def test_host_rejects_untrackable(tag, bad):
    h = sd.host_sketch([1.0, -2.0, 0.0, bad, 3.0])
    assert h.rejected == 3 and h.total == 3.0          # nothing before it is rejected, nothing after it is fed
    assert dd.decode(h.blob).bins() == dd.Sketch().accept_all(np.array([1.0, -2.0, 0.0])).bins()
    assert sd.host_sketch([1.0], merge_vals=[2.0, bad]).rejected == 2
    with pytest.raises(ValueError):
        dd.Sketch().accept_all(np.array([1.0, bad]))


# ---- 3. add_bin ----

def test_add_bin_equals_accept():
    seen = {}
    for p in _all_probes() + sd.wide_probes():
        if p.cls.kind == "decided":
            seen.setdefault((p.value < 0, p.cls.index), p.value)
    kmin, kmax = sd.index_range()
    assert (False, kmin) in seen and (True, kmax) in seen and (False, 0) in seen and (True, -1) in seen
    for (neg, i), v in seen.items():
        assert sd.host_sketch(bins=[(sd.kernel_bin(i, neg), 1.0)]).blob == sd.host_sketch([v]).blob, (neg, i, v)
    assert sd.host_sketch(bins=[(0, 1.0)]).blob == sd.host_sketch([0.0]).blob


def test_add_bin_id_range():
    B, H, N = sd.DD_BIAS, sd.DD_HALF, sd.DD_NBINS
    for bid, want in [(0, ({}, {}, 3.0)), (1, ({-B: 3.0}, {}, 0.0)), (H, ({B - 1: 3.0}, {}, 0.0)),
                      (H + 1, ({}, {-B: 3.0}, 0.0)), (N - 1, ({}, {B - 1: 3.0}, 0.0))]:
        assert dd.decode(sd.host_sketch(bins=[(bid, 3.0)]).blob).bins() == want, bid
    with pytest.raises(ValueError):
        sd.host_sketch(bins=[(N, 1.0)])


# ---- 4. quantile ----

def _exact(v, q):
    s = np.sort(v)
    return s[int(np.floor(q * (len(s) - 1)))]


def _quantile_cases():
    rng = np.random.default_rng(12)
    mixed = np.concatenate([rng.lognormal(0, 3, 3000), -rng.lognormal(1, 2, 1000), np.zeros(100), [sd.FIRST, -sd.LAST]])
    return {"one": np.array([42.5]), "negatives": -rng.lognormal(0, 2, 500), "zeros": np.zeros(7), "mixed": mixed,
            "empty": np.array([])}


@pytest.mark.parametrize("name", ["one", "negatives", "zeros", "mixed", "empty"])
def test_quantiles_of_accepted_values(name):
    v = _quantile_cases()[name]
    h = sd.host_sketch(v, qs=QS)
    o = dd.Sketch().accept_all(v)
    assert h.total == float(len(v)) and dd.decode(h.blob).bins() == o.bins()
    assert [sd.bits(x) for x in h.quantiles] == [sd.bits(o.quantile(q)) for q in QS]
    for q, got in zip(QS, h.quantiles):
        if len(v):
            e = _exact(v, q)
            assert abs(got - e) <= 0.01 * abs(e), (name, q, got, e)
        else:
            assert got == 0.0


def test_quantiles_of_large_counts():
    """Bins with counts up to 2^40, as add_bin takes them from the kernels' (cell, bin) counts."""
    bins = [(False, -300, 2.0 ** 40), (False, 12, 3.0), (True, 40, 2.0 ** 33), (True, -7, 1.0), (False, 900, 2.0 ** 40 - 1)]
    h = sd.host_sketch(bins=[(sd.kernel_bin(i, neg), c) for neg, i, c in bins] + [(0, 2.0 ** 20)], qs=QS)
    o = dd.Sketch()
    for neg, i, c in bins:
        (o.neg if neg else o.pos)[i] = c
    o.zero = 2.0 ** 20
    assert dd.decode(h.blob).bins() == o.bins() and h.total == o.count()
    assert [sd.bits(x) for x in h.quantiles] == [sd.bits(o.quantile(q)) for q in QS]
    # the exact order statistic of the bins' representative values, by integer rank
    ladder = sorted([(-dd.value(i) if neg else dd.value(i), int(c)) for neg, i, c in bins] + [(0.0, 2 ** 20)])
    total = sum(c for _, c in ladder)
    for q, got in zip(QS, h.quantiles):
        rank = q * (total - 1.0)            # the sketch's rank rule, on the double the sketch computes
        run = 0
        for val, c in ladder:
            run += c
            if run > rank:
                break
        assert got == val, (q, got, val)


# ---- 5. serialize ----

def test_serialize_round_trips():
    kmin, kmax = sd.index_range()
    assert dd.decode(sd.host_sketch().blob).bins() == ({}, {}, 0.0)
    assert dd.decode(sd.host_sketch([0.0, -0.0, 1e-310]).blob).bins() == ({}, {}, 3.0)
    h = sd.host_sketch([1.0, 1.0, 1.03])            # lowest index 0: no offset field
    assert dd.decode(h.blob).bins() == ({0: 2.0, 1: 1.0}, {}, 0.0)
    store = h.blob[11:]                              # after mapping{gamma}: 0x0a 0x09 0x09 <8 bytes>
    assert store[:4] == bytes([0x12, 18, 0x12, 16]) and store[20:] == bytes([0x1a, 0])   # two packed doubles, nothing else
    h = sd.host_sketch([0.5, -0.25, 3.0])           # negative lowest index: zigzag
    o = dd.Sketch().accept_all(np.array([0.5, -0.25, 3.0]))
    assert dd.decode(h.blob).bins() == o.bins() and min(o.pos) < 0 and min(o.neg) < 0
    h = sd.host_sketch([sd.FIRST, sd.LAST, -sd.FIRST, -sd.LAST])   # the full range, both stores
    assert dd.decode(h.blob).bins() == ({kmin: 1.0, kmax: 1.0}, {kmin: 1.0, kmax: 1.0}, 0.0)
    assert len(h.blob) > 2 * 8 * (kmax - kmin + 1)


# ---- 6. merge ----

def test_merge_is_concatenation():
    rng = np.random.default_rng(8)
    a = np.concatenate([rng.lognormal(0, 3, 2000), -rng.lognormal(0, 3, 500), np.zeros(9)])
    b = np.concatenate([rng.lognormal(2, 1, 700), -rng.lognormal(-3, 2, 900), np.zeros(2), [sd.LAST]])
    m = sd.host_sketch(a, merge_vals=b, qs=QS)
    u = sd.host_sketch(np.concatenate([a, b]), qs=QS)
    assert m.blob == u.blob and m.quantiles == u.quantiles and m.total == float(len(a) + len(b))
    extra = [(sd.kernel_bin(5, False), 4.0), (sd.kernel_bin(-9, True), 2.0), (0, 1.0)]
    m2 = sd.host_sketch(a, bins=extra, merge_vals=b, merge_bins=extra)
    want = dd.Sketch().accept_all(np.concatenate([a, b]))
    want.pos[5] = want.pos.get(5, 0.0) + 8.0
    want.neg[-9] = want.neg.get(-9, 0.0) + 4.0
    want.zero += 2.0
    assert dd.decode(m2.blob).bins() == want.bins()
    assert sd.host_sketch(merge_vals=a).blob == sd.host_sketch(a).blob      # into an empty sketch


# ---- 7. the files, through the oracle ----

@pytest.mark.parametrize("route", ["tiles", "rows", "metrics"])
def test_files_and_expectations_through_the_oracle(tmp_path, route):
    """The writers, expected_sketches and match_sketch as the GPU tests use them, with the oracle's evaluator in the
    engine's place: the boundary file's sketches per (timestamp, case) hold what the `decimal` floor says."""
    from oracle import dataexpr as dx
    from tests import test_gpu_sketch_bins as g
    probes = sd.wide_probes() + sd.boundary_probes() + sd.edge_probes()
    metrics = route == "metrics"
    rows = (sd.metrics_rows if metrics else sd.logs_rows)(probes)
    assert len(rows) <= sd.TILE_ROWS
    if metrics:   # MAX(rollup) per (timestamp, name, case) is the value itself
        assert len({(r.ts, r.name, r.case) for r in rows}) == len(rows)
    path = sd.write_file(tmp_path / "b.parquet", rows, metrics, num_as_text=route == "rows")
    filt, nameset = g._names(route, [sd.PROBE, sd.FILLER])
    req = g._request(route, "p50", filt, 1)
    pr = dx.parse_pushdown(req)
    got = dx.evaluate_percentile_per_glob(pr, g.GLOB, [path])
    per_glob, merged = g._expected([rows], nameset, route, g.GLOB)
    assert per_glob[0] == merged and len(got) == 1
    out = [(ts, g._case_of(route, tags), sk.quantile(0.5), sk) for ts, tags, sk in got[0]]
    g._check_rows(route, out, per_glob[0], 0.5, f"oracle {route}", single=True)
    kmin, kmax = sd.index_range()
    assert [sk.bins() for _, case, _, sk in out if case == sd.WIDE_CASE] == [({kmin: 1.0, kmax: 1.0}, {}, 0.0)]
    # an untrackable row: the oracle raises when it passes, and answers when the filter or the window drops it
    from lakeside_amd import synth
    bad = sd.write_file(tmp_path / "u.parquet", sd.untrackable_rows(math.inf, metrics), metrics, num_as_text=route == "rows")
    both, good = synth.leaf(synth.NAME, "in", sd.GOOD, sd.BAD), synth.leaf(synth.NAME, "eq", sd.GOOD)
    with pytest.raises(ValueError):
        dx.evaluate_percentile_per_glob(dx.parse_pushdown(g._request(route, "p50", both, 1)), g.GLOB, [bad])
    for req in (g._request(route, "p50", good, 1), g._request(route, "p50", both, 1, synth.T0, synth.T0 + sd.BAD_TS_OFFSET)):
        want = dx.evaluate_percentile_per_glob(dx.parse_pushdown(req), g.GLOB, [bad])
        assert sum(sk.count() for _, _, sk in want[0]) == 60.0 and len(want[0]) >= 4
