"""Infinite and overflowing values through the checkers themselves (CPU only): the row comparators, the Python
oracle's exact_sum, the C++ restatement's double-double cells, and the fixture of tests/test_gpu_nonfinite.py
(tests/nonfinite_data.py), whose row classes are asserted here on the oracle's rows and with exact rationals."""
import itertools
import json
import math
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import nonfinite_data as nf
from tests.parity import assert_rows_equal

INF, NAN = math.inf, math.nan
DBL_MAX = sys.float_info.max
AGGS = ["sum", "avg", "min", "max", "count"]


# ---------------------------------------------------------------------------------------------------------------
# 1. the comparators
# ---------------------------------------------------------------------------------------------------------------
REJECTED = [(1.0, INF), (-INF, INF), (NAN, INF), (INF, NAN), (1e308, INF), (INF, -INF), (-1e308, -INF), (INF, 1e308)]
ACCEPTED = [(INF, INF), (-INF, -INF), (NAN, NAN), (1.0, 1.0), (1.0 + 2 ** -52, 1.0)]


def _rows(v):
    return [(0, 5.0, {"name": "a"}), (600_000, v, {"name": "a"})]


def _cols(v):
    return (np.array([0, 600_000], np.int64), np.array([5.0, v]), np.array([b"name\x1ea", b"name\x1ea"], dtype=object))


@pytest.mark.parametrize("agg", ["sum", "avg"])
@pytest.mark.parametrize("got,want", REJECTED, ids=[f"{g!r}_vs_{w!r}" for g, w in REJECTED])
def test_comparators_reject(agg, got, want):
    from oracle import cpu
    with pytest.raises(AssertionError):
        assert_rows_equal(_rows(got), _rows(want), agg, "rows")
    with pytest.raises(AssertionError):
        cpu.assert_columns_equal(_cols(got), _cols(want), agg, "columns")


@pytest.mark.parametrize("agg", ["sum", "avg"])
@pytest.mark.parametrize("got,want", ACCEPTED, ids=[f"{g!r}_vs_{w!r}" for g, w in ACCEPTED])
def test_comparators_accept(agg, got, want):
    from oracle import cpu
    assert_rows_equal(_rows(got), _rows(want), agg, "rows")
    cpu.assert_columns_equal(_cols(got), _cols(want), agg, "columns")


def test_dd_value():
    """hi alone when it is not finite, else the rounded hi + lo; scalars and arrays alike."""
    from oracle import cpu
    pairs = [(INF, NAN, INF), (-INF, NAN, -INF), (NAN, NAN, NAN), (INF, 1.0, INF), (1.0, 2.0 ** -53, 1.0),
             (1.0, 2.0 ** -52, 1.0 + 2.0 ** -52), (0.0, 0.0, 0.0), (DBL_MAX, -1.0, DBL_MAX)]
    for hi, lo, want in pairs:
        got = cpu.dd_value(hi, lo)
        assert isinstance(got, float) and (got == want or (got != got and want != want)), (hi, lo, got)
    got = cpu.dd_value(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    want = np.array([p[2] for p in pairs])
    assert np.array_equal(got, want, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------
# 2. exact_sum against exact rationals
# ---------------------------------------------------------------------------------------------------------------
OVERFLOW = Fraction(2) ** 1024 - Fraction(2) ** 970   # halfway between DBL_MAX and 2^1024: rounds to even = 2^1024


def _round_fraction(s):
    """The double nearest to the rational s, ties to even, +-inf at or beyond the overflow threshold."""
    if s == 0:
        return 0.0
    if abs(s) >= OVERFLOW:
        return INF if s > 0 else -INF
    sign, a = (1.0 if s > 0 else -1.0), abs(s)
    k = a.numerator.bit_length() - a.denominator.bit_length()
    if a < Fraction(2) ** k:
        k -= 1                      # 2^k <= a < 2^(k+1)
    e = max(k - 52, -1074)          # the ulp of a's binade, or the subnormal spacing
    q = a / Fraction(2) ** e
    n, r = divmod(q.numerator, q.denominator)
    twice = 2 * r
    if twice > q.denominator or (twice == q.denominator and n & 1):
        n += 1
    return sign * math.ldexp(float(n), e)


ATOMS = [0.0, 5e-324, 1.0, 2.0 ** 53, 1e308, 1.7976931348623157e308]
VALUES = [s * a for a in ATOMS for s in (1.0, -1.0)]


def _exact_sum_cases():
    cases = [list(c) for n in (1, 2, 3) for c in itertools.combinations_with_replacement(VALUES, n)]
    rng = np.random.default_rng(3)
    cases += [rng.choice(VALUES, int(n)).tolist() for n in rng.integers(4, 12, 200)]
    cases += [[1.5e308, 1.5e308], [-1.5e308, -1.5e308], [1.7e307] * 10, [-1.7e307] * 10, [DBL_MAX, 2.0 ** 970],
              [DBL_MAX, 2.0 ** 969], [DBL_MAX, 2.0 ** 970, -5e-324], [1e308] * 40, [-1e308] * 40,
              [1.5e308, 1.5e308, -1.5e308], [DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, 1.0]]
    return cases


def test_exact_sum_finite_against_fractions():
    from oracle import dataexpr as dx
    n_inf = n_fallback = 0
    for vals in _exact_sum_cases():
        got = dx.exact_sum(np.array(vals, np.float64))
        want = _round_fraction(sum(map(Fraction, vals)))
        assert got == want, f"exact_sum({vals!r}) = {got!r}, exact rounding gives {want!r}"
        n_inf += math.isinf(want)
        try:
            math.fsum(vals)
        except OverflowError:
            n_fallback += 1
    assert n_inf > 20 and n_fallback > n_inf   # overflowing totals, and finite totals past an intermediate overflow
    assert dx.exact_sum(np.array([1.5e308, 1.5e308])) == INF
    assert dx.exact_sum(np.array([-1.5e308, -1.5e308])) == -INF
    assert dx.exact_sum(np.array([1.7e307] * 10)) == _round_fraction(10 * Fraction(1.7e307)) < INF
    assert dx.exact_sum(np.array([DBL_MAX, 2.0 ** 970])) == INF          # the threshold itself: ties to even
    assert dx.exact_sum(np.array([DBL_MAX, 2.0 ** 969])) == DBL_MAX


def test_round_fraction_is_float_rounding():
    """The reference rounding above against Python's own correctly rounded int / int division."""
    rng = np.random.default_rng(4)
    for _ in range(300):
        vals = rng.choice(VALUES[:10], 5).tolist() + rng.lognormal(0, 30, 3).tolist()
        s = sum(map(Fraction, vals))
        if abs(s) < OVERFLOW:
            assert _round_fraction(s) == s.numerator / s.denominator


@pytest.mark.parametrize("vals,want", [([1.0, INF], INF), ([-INF, 2.0], -INF), ([INF, -INF], NAN), ([INF, NAN], NAN),
                                        ([NAN], NAN), ([-INF, NAN, 1.0], NAN), ([INF, INF, 1e308], INF),
                                        ([1e308, 1e308, INF], INF), ([-1e308, -1e308, -INF], -INF)])
def test_exact_sum_nonfinite_follows_ieee(vals, want):
    from oracle import dataexpr as dx
    got = dx.exact_sum(np.array(vals, np.float64))
    assert got == want or (got != got and want != want)


# ---------------------------------------------------------------------------------------------------------------
# 3. / 4. the fixture: the oracle against the C++ restatement, and the row classes
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    root = tmp_path_factory.mktemp("nonfinite")
    return {label: nf.write_files(root, label) for label in ("clean", "mixed")}


def _request(agg, gbs=("name",)):
    from lakeside_amd import synth
    gbs = [synth.NAME if g == "name" else g for g in gbs]
    return json.dumps(synth.pushdown(nf.all_names(), nf.segments(), agg, gbs))


@pytest.fixture(scope="module")
def oracle_cells(sets):
    """Per-glob oracle cells of `:by name` (with their raw values: one evaluation serves every aggregate)."""
    from oracle import dataexpr as dx
    return {label: dx.evaluate_glob_cells(dx.parse_pushdown(_request("sum")), nf.GLOB, paths, sources=blobs)
            for label, (paths, blobs) in sets.items()}


@pytest.mark.parametrize("label", ["clean", "mixed"])
@pytest.mark.parametrize("agg", AGGS)
def test_oracle_against_restatement(sets, oracle_cells, label, agg):
    from oracle import cpu, dataexpr as dx
    paths, blobs = sets[label]
    pr = dx.parse_pushdown(_request(agg))
    cells = oracle_cells[label]
    got = cpu.evaluate_per_glob(pr, blobs, nf.GLOB, threads=4)
    assert len(got) == len(cells) == 2
    for gi, (g, cs) in enumerate(zip(got, cells)):
        assert_rows_equal(g, [(c.ts, c.agg_value(agg), c.tags) for c in cs], agg, f"{label} {agg} glob {gi}")
        nf.assert_classes(g, agg, gi, f"restatement {label} {agg} glob {gi}")
    want = dx.merge_glob_cells(pr, cells)
    merged = cpu.evaluate_merged(pr, blobs, nf.GLOB, threads=3)
    assert_rows_equal(merged, want, agg, f"{label} {agg} merged")
    nf.assert_classes(merged, agg, "merged", f"restatement {label} {agg} merged")
    # the columnar form (the bench's validator)
    table = cpu.evaluate_cell_table(pr, nf.GLOB, blobs, 4)
    wcols = (np.array([r[0] for r in want], np.int64), np.array([r[1] for r in want]),
             np.array([cpu.tag_key(r[2]) for r in want], dtype=object))
    cpu.assert_columns_equal(cpu.merge_cell_table(table, agg, True), wcols, agg, f"{label} {agg} merged columns")


@pytest.mark.parametrize("label", ["clean", "mixed"])
@pytest.mark.parametrize("agg", AGGS)
def test_fixture_classes(oracle_cells, label, agg):
    from oracle import dataexpr as dx
    pr = dx.parse_pushdown(_request(agg))
    cells = oracle_cells[label]
    for gi, cs in enumerate(cells):
        nf.assert_classes([(c.ts, c.agg_value(agg), c.tags) for c in cs], agg, gi, f"oracle {label} {agg} glob {gi}")
    nf.assert_classes(dx.merge_glob_cells(pr, cells), agg, "merged", f"oracle {label} {agg} merged")


@pytest.mark.parametrize("label", ["clean", "mixed"])
def test_fixture_guard(sets, oracle_cells, label):
    """The classes hold in every order of summation: the overflowing kinds are single-signed, every ovfp / ovfn cell's
    exact total is at least 2 * DBL_MAX, an ovfm glob cell stays below 0.8 * DBL_MAX and the merged ovfm cell is at
    least 1.2 * DBL_MAX, bigfin stays below DBL_MAX / 2 merged; at least 8 values per (file, bucket) and name; f1 of
    `mixed` alone holds NULLs."""
    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    big = Fraction(DBL_MAX)
    merged = {}
    for gi, cs in enumerate(oracle_cells[label]):
        assert len(cs) == nf.NBUCKETS * len(nf.KINDS)
        for c in cs:
            k, v = c.tags["name"], c.values
            merged.setdefault((k, c.ts), []).append(v)
            assert c.count >= 8 * (2 if gi == 0 else 1)
            if k in ("ovfp", "ovfm", "bigfin"):
                assert np.all(v > 0)
            if k == "ovfn":
                assert np.all(v < 0)
            if k in ("ovfp", "ovfn"):
                assert abs(nf.exact_fraction(v)) >= 2 * big
            if k == "ovfm":
                assert c.count == (16 if gi == 0 else 8)
                assert big / 2 < nf.exact_fraction(v) < big * 8 / 10
            if k in ("fin", "bigfin"):
                assert np.all(np.isfinite(v))
            if k in ("pinf", "ninf", "both", "naninf"):
                nfiles = 2 if gi == 0 else 1
                assert np.sum(v == np.inf) == (0 if k == "ninf" else 2 * nfiles)
                assert np.sum(v == -np.inf) == (2 * nfiles if k in ("ninf", "both") else 0)
                assert np.sum(np.isnan(v)) == (2 * nfiles if k == "naninf" else 0)
            if k == "intinf":
                assert np.sum(~np.isfinite(v)) == gi and np.sum(v == np.inf) == gi
                assert np.all(v[np.isfinite(v)] == np.trunc(v[np.isfinite(v)]))
            if k in ("negz", "zmix"):
                assert np.all(v == 0.0) and np.all(np.signbit(v) == (k == "negz" or gi == 1))
    for (k, ts), vs in merged.items():
        assert len(vs) == 2
        total = nf.exact_fraction(np.concatenate(vs)) if k in ("ovfm", "bigfin") else None
        if k == "ovfm":
            assert total >= big * 12 / 10
        if k == "bigfin":
            assert total < big / 2
    paths, _ = sets[label]
    for i, p in enumerate(paths):
        md = pq.ParquetFile(p).metadata
        assert md.num_rows == nf.ROWS and md.num_row_groups == 1
        t = pq.read_table(p)
        assert t.column(dx.VALUE).null_count == (int(nf.ROWS * nf.NULL_FRAC) if (label == "mixed" and i == 1) else 0)
        ts = t.column(dx.TIMESTAMP).to_numpy()
        assert np.all(np.diff(ts) >= 0) and len(np.unique(ts // nf.STEP)) == nf.NBUCKETS
        assert len(set(t.column(nf.SVC).to_pylist())) == 512
        assert t.column(nf.ATTR).to_numpy().min() >= 0
