"""Data of the non-finite value tests (tests/test_oracle_nonfinite.py on the CPU, tests/test_gpu_nonfinite.py on the
MI355X): three files of 4096 rows (one row group, one page: one tile each), timestamps sorted within hour 0, a 600 s
step (6 buckets), glob size 2 (globs [f0, f1] and [f2]).  Every name is one kind of value column, present in every
(file, bucket) with at least 8 rows, so every request `:by name` has 6 rows per name and glob, and 6 merged.

Every row of a name has one class per aggregate, whatever the order of summation (expected_class below):

  fin     lognormal(0, 2)
  pinf    lognormal, and 2 +inf per (file, bucket)
  ninf    lognormal, and 2 -inf per (file, bucket)
  both    lognormal, and 2 +inf and 2 -inf per (file, bucket)
  naninf  lognormal, and 2 NaN and 2 +inf per (file, bucket)
  ovfp    uniform [1e308, 1.7e308]: single-signed, every cell's exact total >= 2 * DBL_MAX
  ovfn    the negatives of ovfp's distribution
  ovfm    8 per (file, bucket), single-signed: a glob's cell totals 0.65 .. 0.75 * DBL_MAX (finite in every order: the
          partial sums of positive values only grow), the merged cell 1.3 .. 1.5 * DBL_MAX (+inf in every order).  Two
          finite glob totals cannot reach 2 * DBL_MAX; with one sign the class needs only a total clear of DBL_MAX.
  bigfin  8 per (file, bucket), about 1.7e306: finite per glob and merged
  negz    -0.0 only
  zmix    +0.0 in f0 and f1, -0.0 in f2
  intinf  integers in [0, 999]; in f2 one +inf per bucket

`mixed` differs from `clean` by NULL values in f1 (2 % of its rows, ordinary values only: no infinity, NaN, zero or
ovfm / bigfin row is NULL, so the classes hold), which makes f1's tile `has_nulls`.
"""
import math
import sys
from fractions import Fraction

import numpy as np

KINDS = ["fin", "pinf", "ninf", "both", "naninf", "ovfp", "ovfn", "ovfm", "bigfin", "negz", "zmix", "intinf"]
ROWS, NFILES, GLOB, STEP, NBUCKETS = 4096, 3, 2, 600_000, 6
DBL_MAX = sys.float_info.max
SVC, ATTR, LAT = "svc", "attr.k", "lat$number"
LAT_DURATION = "lat$duration"
NULL_FRAC = 0.02


def _columns(i, rng, nulls):
    from lakeside_amd import synth
    per_bucket = [ROWS // NBUCKETS + (1 if b < ROWS % NBUCKETS else 0) for b in range(NBUCKETS)]
    ts, kind, val, special = [], [], [], []
    for b, nb in enumerate(per_bucket):
        counts = {k: 8 for k in ("ovfm", "bigfin")}
        rest = [k for k in KINDS if k not in counts]
        share = (nb - 16) // len(rest)
        for k in rest:
            counts[k] = share
        counts["fin"] += nb - 16 - share * len(rest)
        ks, vs, sp = [], [], []
        for k in KINDS:
            m = counts[k]
            v = rng.lognormal(0.0, 2.0, m)
            s = np.zeros(m, bool)
            if k in ("pinf", "both", "naninf"):
                v[0:2], s[0:2] = np.inf, True
            if k in ("ninf", "both"):
                v[2:4], s[2:4] = -np.inf, True
            if k == "naninf":
                v[2:4], s[2:4] = np.nan, True
            if k in ("ovfp", "ovfn"):
                v = rng.uniform(1e308, 1.7e308, m) * (1.0 if k == "ovfp" else -1.0)
            if k == "ovfm":   # the glob's cell: 16 values in glob 0 (f0, f1), 8 in glob 1 (f2)
                v, s = rng.uniform(0.65, 0.75, m) * DBL_MAX / (16.0 if i < 2 else 8.0), np.ones(m, bool)
            if k == "bigfin":
                v, s = rng.uniform(1.6e306, 1.8e306, m), np.ones(m, bool)
            if k == "negz":
                v, s = np.full(m, -0.0), np.ones(m, bool)
            if k == "zmix":
                v, s = np.full(m, -0.0 if i == 2 else 0.0), np.ones(m, bool)
            if k == "intinf":
                v = rng.integers(0, 1000, m).astype(np.float64)
                if i == 2:
                    v[0], s[0] = np.inf, True
            p = rng.permutation(m)
            ks += [k] * m
            vs.append(v[p])
            sp.append(s[p])
        p = rng.permutation(nb)
        kind.append(np.array(ks, dtype=object)[p])
        val.append(np.concatenate(vs)[p])
        special.append(np.concatenate(sp)[p])
        ts.append(synth.T0 + b * STEP + np.sort(rng.integers(0, STEP, nb)))
    ts, kind, val, special = (np.concatenate(x) for x in (ts, kind, val, special))
    null = np.zeros(ROWS, bool)
    if nulls:
        cand = np.nonzero(~special)[0]
        null[rng.choice(cand, int(ROWS * NULL_FRAC), replace=False)] = True
    svc = rng.permutation(np.arange(ROWS) % 512)
    return ts, kind, val, null, svc, rng.integers(0, 1000, ROWS)


def write_files(root, label):
    """The three files of set `label` ("clean" / "mixed") under `root`; returns (paths, blobs)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from oracle import dataexpr as dx
    paths, blobs = [], []
    for i in range(NFILES):
        rng = np.random.default_rng(9100 + i)   # the sets differ by the NULL mask only
        ts, kind, val, null, svc, attr = _columns(i, rng, label == "mixed" and i == 1)
        t = pa.table({
            dx.TIMESTAMP: pa.array(ts, pa.int64()),
            dx.VALUE: pa.array(val, pa.float64(), mask=null),
            dx.NAME: pa.array(kind.tolist(), pa.string()),
            SVC: pa.array([f"s{k:03d}" for k in svc], pa.string()),
            ATTR: pa.array(attr, pa.int64()),
            LAT: pa.array(val.copy(), pa.float64(), mask=null),
            LAT_DURATION: pa.array(val.copy(), pa.float64(), mask=null),
        })
        path = str(root / f"nf_{label}_{i}.parquet")
        strings = [dx.NAME, SVC]
        pq.write_table(t, path, compression="NONE", use_dictionary=strings, row_group_size=ROWS,
                       data_page_size=1 << 20, column_encoding={c: "PLAIN" for c in t.column_names if c not in strings})
        paths.append(path)
        with open(path, "rb") as f:
            blobs.append(f.read())
    return paths, blobs


def segments(step=STEP):
    from lakeside_amd import synth
    return [synth.segment_request(i, step=step, hour=0) for i in range(NFILES)]


def all_names():
    from lakeside_amd import synth
    return synth.leaf(synth.NAME, "!=", "no_such_name")


# ---------------------------------------------------------------------------------------------------------------
# Row classes.  scope: 0 / 1 = the glob's rows, "merged" = the merged rows.
# ---------------------------------------------------------------------------------------------------------------
def value_class(v):
    if v != v:
        return "nan"
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    if v == 0.0:
        return "-0" if math.copysign(1.0, v) < 0 else "+0"
    return "fin"


FIN, PINF, NINF, NAN, NZ, PZ = {"fin"}, {"+inf"}, {"-inf"}, {"nan"}, {"-0"}, {"+0"}


def expected_class(name, agg, scope):
    """The classes a row of `name` may have (a set; one class except for a zero sum, whose sign is not pinned)."""
    if agg == "count":
        return FIN
    f2 = scope in (1, "merged")   # the row covers f2
    if agg in ("sum", "avg"):
        return {"fin": FIN, "pinf": PINF, "ninf": NINF, "both": NAN, "naninf": NAN, "ovfp": PINF, "ovfn": NINF,
                "ovfm": PINF if scope == "merged" else FIN, "bigfin": FIN, "negz": NZ | PZ, "zmix": NZ | PZ,
                "intinf": PINF if f2 else FIN | PZ}[name]
    if agg == "min":
        return {"ninf": NINF, "both": NINF, "ovfn": FIN, "negz": NZ, "zmix": NZ if f2 else PZ,
                "intinf": FIN | PZ}.get(name, FIN)
    if agg == "max":
        return {"pinf": PINF, "both": PINF, "naninf": NAN, "negz": NZ, "zmix": NZ if scope == 1 else PZ,
                "intinf": PINF if f2 else FIN}.get(name, FIN)
    raise NotImplementedError(agg)


def assert_classes(rows, agg, scope, label="", names=KINDS, per_name=NBUCKETS, tag="name"):
    """Every name of `names` has `per_name` rows and every row its expected class."""
    seen = {k: [] for k in names}
    for ts, v, tags in rows:
        assert tags.get(tag) in seen, f"{label}: unexpected row {ts} {tags}"
        seen[tags[tag]].append(v)
    for k, vs in seen.items():
        assert len(vs) == per_name, f"{label}: {k} has {len(vs)} rows, expected {per_name}"
        want = expected_class(k, agg, scope)
        bad = [v for v in vs if value_class(v) not in want]
        assert not bad, f"{label}: {k} {agg} rows {bad!r} are not of class {sorted(want)}"


def exact_fraction(values):
    return sum((Fraction(float(v)) for v in values), Fraction(0))
