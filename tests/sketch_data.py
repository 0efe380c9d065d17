"""Data of the DDSketch bin tests (tests/test_sketch_cpu.py on the CPU, tests/test_gpu_sketch_bins.py on the MI355X):
values at the bin boundaries of the index mapping, at the edges of its range and beyond it, and the files that carry
them through every statement of `index = floor(ln|v| * MULTIPLIER)`.

The exact index.  For a trackable magnitude a, x(a) = ln(a) * MULTIPLIER with MULTIPLIER the double of
oracle/ddsketch.py, evaluated with `decimal` at 70 digits (x_of).  A conforming site computes fl(log1(a) * MULTIPLIER)
with log1 within 1 ulp of ln a (HIP's documented bound for double log; Java's Math.log promises the same).  MULTIPLIER
~ 50.25 lies in [32, 64), so ulp(x) is 32 or 64 ulp(ln a) and the computed value is within 50.25 / 32 + 0.5 < 2.1 ulp(x)
of x(a).  The margin of an integer k != 0 is M(k) = 3 * 2^(floor(log2 |k|) - 52), above 2.1 ulp of every x next to k:

  decided   |x(a) - nearest integer| >= M: the index is floor(x(a)) on every site, no tolerance
  crossing  x(a) closer than M to the integer k: the index is k - 1 or k (the reference itself is undefined between them)
  a = 1.0   index 0 (log(1) = +0 exactly)

Boundary family: per k of BOUNDARY_KS (kmin + 1 and kmax appended, derived here) four magnitudes -- lo (the largest
double with x < k - M), b (the largest with x < k), c (the smallest with x >= k), hi (the smallest with x >= k + M) --
each in both signs.  For small |k| the window is narrower than one ulp of a: lo / hi coincide with b / c and are decided.
Broad family: 4,000 magnitudes log-uniform over the indexable range, random signs, every one decided (asserted).

Files (one tile each: one row group and one page of at most 8,192 rows, PLAIN timestamps and values, dictionary strings,
uncompressed): name `probe` carries the probes and `filler` 1.5, 15 filler rows per probe row, so `name eq probe` lists a
tile's rows sparsely and `name in (probe, filler)` densely; `attr.case` is unique per boundary / edge probe (one sketch
per value) and "filler" for filler rows; `attr.n` is an INT64 column (7 in every row) whose groupBy sends a logs request
through the general row scan.  The metrics twin has rollup columns, timestamps on the 1 s step grid and one row per
(timestamp, name, case): MAX(rollup) is the value itself and reaches the host's accept."""
import collections
import decimal
import functools
import math
import struct
import sys

import numpy as np

from oracle import ddsketch as dd

D = decimal.Decimal
CTX = decimal.Context(prec=70)
MULT = D(dd.MULTIPLIER)                       # the double, exactly
DBL_MIN, DBL_MAX = sys.float_info.min, sys.float_info.max
FIRST = math.nextafter(dd.MIN_INDEXABLE, math.inf)   # the smallest indexed magnitude
LAST = dd.MAX_INDEXABLE

BOUNDARY_KS = ([k for k in range(-8, 9) if k] +
               [s * k for k in (50, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096, 8191, 8192, 16384, 32767, 32768, 35000)
                for s in (1, -1)])
BROAD_N, BROAD_SEED, BROAD_BANDS = 4000, 20260, 8
FILLER_VALUE, FILLER_PER_PROBE = 1.5, 15
NAME, VALUE, TIMESTAMP = "_cardinalhq.name", "_cardinalhq.value", "_cardinalhq.timestamp"
CASE, NUM, NUM_VALUE = "attr.case", "attr.n", 7
PROBE, FILLER = "probe", "filler"
METRIC_NAMES = [f"probe{i}" for i in range(4)]
STEP, METRICS_STEP = 600_000, 1000
TILE_ROWS = 8192
UNTRACKABLE = [("nan", math.nan), ("pinf", math.inf), ("ninf", -math.inf),
               ("over", math.nextafter(dd.MAX_INDEXABLE, math.inf)), ("ndblmax", -DBL_MAX)]


def bits(a: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", a))[0]


def from_bits(u: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def x_of(a: float) -> decimal.Decimal:
    """ln(a) * MULTIPLIER to 70 digits, for a double a > 0."""
    return CTX.multiply(CTX.ln(D(a)), MULT)


def margin(k: int) -> decimal.Decimal:
    """M(k); the integer 0 (x within 2^-52 of 0: no double but 1.0 itself) takes M(1)."""
    return CTX.divide(D(3), D(2 ** (52 - ((abs(k) or 1).bit_length() - 1))))   # exact: at most 52 digits


# kind: "decided" (index = floor x), "crossing" (index = the integer k; k - 1 is allowed too), "zero" (the zero bin)
Class = collections.namedtuple("Class", "kind index floor")


def classify(a: float) -> Class:
    """The class of a magnitude MIN_INDEXABLE < a <= MAX_INDEXABLE."""
    if a == 1.0:
        return Class("decided", 0, 0)
    x = x_of(a)
    k = int(x.to_integral_value(rounding=decimal.ROUND_HALF_EVEN))
    fl = int(x.to_integral_value(rounding=decimal.ROUND_FLOOR))
    if abs(CTX.subtract(x, D(k))) >= margin(k):
        return Class("decided", fl, fl)
    return Class("crossing", k, fl)


def allowed(c: Class):
    return {c.index} if c.kind == "decided" else {c.index - 1, c.index}


def first_at_least(t) -> float:
    """The smallest double a in [FIRST, LAST] with x(a) >= t (bisection over the bit pattern: x grows with it)."""
    lo, hi = bits(FIRST), bits(LAST)
    if x_of(LAST) < t:
        raise ValueError(f"no indexable double reaches x = {t}")
    while lo < hi:
        mid = (lo + hi) // 2
        if x_of(from_bits(mid)) >= t:
            hi = mid
        else:
            lo = mid + 1
    return from_bits(lo)


@functools.lru_cache(None)
def index_range():
    """(kmin, kmax): the indices of the first and the last indexed magnitude."""
    return (int(x_of(FIRST).to_integral_value(rounding=decimal.ROUND_FLOOR)),
            int(x_of(LAST).to_integral_value(rounding=decimal.ROUND_FLOOR)))


@functools.lru_cache(None)
def boundary_ks():
    kmin, kmax = index_range()
    return tuple(BOUNDARY_KS) + (kmin + 1, kmax)


@functools.lru_cache(None)
def boundary(k: int):
    """(lo, b, c, hi) of the integer k."""
    m = margin(k)
    c = first_at_least(D(k))
    return (math.nextafter(first_at_least(CTX.subtract(D(k), m)), 0.0), math.nextafter(c, 0.0), c, first_at_least(CTX.add(D(k), m)))


# A probe: one value under its own `attr.case` (broad probes share 16); value None = a NULL row (reads as 0.0)
Probe = collections.namedtuple("Probe", "case value cls")
ZERO = Class("zero", None, None)


def _probe(case, v):
    a = abs(v)
    return Probe(case, v, ZERO if a <= dd.MIN_INDEXABLE else classify(a))


@functools.lru_cache(None)
def boundary_probes():
    out = []
    for k in boundary_ks():
        for role, a in zip(("lo", "b", "c", "hi"), boundary(k)):
            for sign, s in (("p", 1.0), ("n", -1.0)):
                out.append(_probe(f"k{k:+d}.{role}.{sign}", s * a))
    return tuple(out)


@functools.lru_cache(None)
def edge_probes():
    out = [Probe("zero.null", None, ZERO)]
    below = math.nextafter(dd.MIN_INDEXABLE, 0.0)
    for sign, s in (("p", 1.0), ("n", -1.0)):
        for tag, a in (("zero.0", 0.0), ("zero.denorm", 5e-324), ("zero.dblmin", DBL_MIN), ("zero.below", below),
                       ("zero.minidx", dd.MIN_INDEXABLE), ("first", FIRST), ("last", LAST), ("one", 1.0),
                       ("one.before", math.nextafter(1.0, 0.0)), ("one.after", math.nextafter(1.0, 2.0))):
            out.append(_probe(f"{tag}.{sign}", s * a))
    return tuple(out)


WIDE_CASE = "wide"


def wide_probes():
    """One case tag with the first and the last indexed value: a sketch spanning the whole index range."""
    return (_probe(WIDE_CASE, FIRST), _probe(WIDE_CASE, LAST))


@functools.lru_cache(None)
def broad_probes():
    """4,000 magnitudes log-uniform over (MIN_INDEXABLE, MAX_INDEXABLE], random signs, under 16 case tags (sign x 8
    magnitude bands); every one is decided (the expected share of crossing values is about 1e-11: change the seed if
    one ever is not)."""
    rng = np.random.default_rng(BROAD_SEED)
    l0, l1 = math.log(FIRST), math.log(LAST)
    u = rng.uniform(l0, l1, BROAD_N)
    neg = rng.random(BROAD_N) < 0.5
    out = []
    for ui, ng in zip(u.tolist(), neg.tolist()):
        a = min(max(math.exp(ui), FIRST), LAST)
        band = min(int((ui - l0) / (l1 - l0) * BROAD_BANDS), BROAD_BANDS - 1)
        p = _probe(f"broad.{'n' if ng else 'p'}{band}", -a if ng else a)
        assert p.cls.kind == "decided", (a, p.cls)
        out.append(p)
    return tuple(out)


def bins_of(probes):
    """(pos, neg, zero) of the sketch over decided / zero probes, as oracle.ddsketch.Sketch.bins() reports it."""
    pos, neg, zero = {}, {}, 0.0
    for p in probes:
        if p.cls.kind == "zero":
            zero += 1.0
        else:
            assert p.cls.kind == "decided", p
            st = neg if p.value < 0 else pos
            st[p.cls.index] = st.get(p.cls.index, 0.0) + 1.0
    return pos, neg, zero


def match_sketch(sk, probes, label=""):
    """Asserts that the decoded sketch `sk` holds exactly `probes`: every decided probe in bin floor(x) of its sign, every
    zero probe in the zero count, every crossing probe in k - 1 or k, nothing else.  Returns [(probe, index found)] of
    the crossing probes."""
    got = collections.Counter()
    for neg, st in ((False, sk.pos), (True, sk.neg)):
        for i, c in st.items():
            assert c == int(c) and c > 0, (label, i, c)
            got[(neg, i)] += int(c)
    zero = sum(1 for p in probes if p.cls.kind == "zero")
    assert sk.zero == float(zero), f"{label}: zero count {sk.zero}, expected {zero}"
    for p in probes:
        if p.cls.kind == "decided":
            key = (p.value < 0, p.cls.index)
            assert got[key] > 0, f"{label}: {p.case} value {p.value!r} is not in bin {key}; bins left {dict(got)}"
            got[key] -= 1
    found = []
    for p in probes:
        if p.cls.kind == "crossing":
            keys = [(p.value < 0, i) for i in (p.cls.index - 1, p.cls.index) if got[(p.value < 0, i)] > 0]
            assert keys, f"{label}: {p.case} value {p.value!r} is in neither bin of {sorted(allowed(p.cls))}; bins left {dict(got)}"
            got[keys[0]] -= 1
            found.append((p, keys[0][1]))
    left = {k: c for k, c in got.items() if c}
    assert not left, f"{label}: unexpected bins {left}"
    return found


# ---------------------------------------------------------------------------------------------------------------------
# The host's dd::Sketch through lk_dd_sim (liblakeside_text.so)
# ---------------------------------------------------------------------------------------------------------------------
HostSketch = collections.namedtuple("HostSketch", "blob quantiles rejected consts total")
_SIM = None


def host_sketch(vals=(), bins=(), merge_vals=(), merge_bins=(), qs=()):
    """Sketch A = accept over `vals`, then add_bin over `bins` = [(kernel bin id, count)]; B likewise from merge_*;
    A.merge(B).  Returns A's serialized bytes, its quantiles at `qs`, the position of the first rejected value (over vals
    then merge_vals; None when every value was accepted), the constants and the total count."""
    import ctypes
    import os
    global _SIM
    if _SIM is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        _SIM = ctypes.CDLL(os.path.join(root, "lakeside_amd", "liblakeside_text.so"))
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        _SIM.lk_dd_sim.argtypes = [vp, sz, vp, vp, sz, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, sz]
        _SIM.lk_dd_sim.restype = ctypes.c_long

    def side(v, b):
        v = np.ascontiguousarray(v, np.float64)
        ids = np.ascontiguousarray([i for i, _ in b], np.uint32)
        cnt = np.ascontiguousarray([c for _, c in b], np.float64)
        return v, ids, cnt

    v, ids, cnt = side(vals, bins)
    mv, mids, mcnt = side(merge_vals, merge_bins)
    q = np.ascontiguousarray(qs, np.float64)
    out_q, consts, total = np.zeros(len(q)), np.zeros(8), np.zeros(1)
    rejected = ctypes.c_long(0)
    buf = np.zeros(1 << 21, np.uint8)   # two full-range stores are 1.14 MB
    n = _SIM.lk_dd_sim(v.ctypes.data, len(v), ids.ctypes.data, cnt.ctypes.data, len(ids), mv.ctypes.data, len(mv),
                       mids.ctypes.data, mcnt.ctypes.data, len(mids), q.ctypes.data, len(q), out_q.ctypes.data,
                       ctypes.addressof(rejected), consts.ctypes.data, total.ctypes.data, buf.ctypes.data, len(buf))
    if n < 0:
        raise ValueError(f"lk_dd_sim: {n}")
    return HostSketch(buf[:n].tobytes(), out_q.tolist(), None if rejected.value < 0 else rejected.value,
                      consts.tolist(), float(total[0]))


DD_BIAS = 40000                # layout.hpp; test_sketch_cpu.py checks them against the library's
DD_HALF = 2 * DD_BIAS
DD_NBINS = 1 + 2 * DD_HALF


def kernel_bin(index, neg):
    """The kernels' bin id of a sketch index."""
    return 1 + DD_BIAS + index + (DD_HALF if neg else 0)


# ---------------------------------------------------------------------------------------------------------------------
# Files
# ---------------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "ts name case value probe")   # probe: the Probe, or None for a filler row


def logs_rows(probes, hour=0):
    """Probe and filler rows of one logs file, timestamps ascending through the hour."""
    from lakeside_amd import synth
    n = len(probes) * (1 + FILLER_PER_PROBE)
    assert n <= TILE_ROWS, n
    t0 = synth.T0 + hour * synth.HOUR
    rows = []
    for j, p in enumerate(probes):
        for f in range(1 + FILLER_PER_PROBE):
            i = j * (1 + FILLER_PER_PROBE) + f
            ts = t0 + (i * synth.HOUR) // n
            at = (j * 7) % (1 + FILLER_PER_PROBE)     # the probe's place among its fillers
            rows.append(Row(ts, PROBE, p.case, p.value, p) if f == at else Row(ts, FILLER, FILLER, FILLER_VALUE, None))
    return rows


def metrics_rows(probes, hour=0):
    """The metrics twin: one row per (timestamp, name, case) on the 1 s grid -- four probes (names probe0 .. probe3) and
    one filler row per timestamp."""
    from lakeside_amd import synth
    t0 = synth.T0 + hour * synth.HOUR
    assert len(probes) <= 4 * (synth.HOUR // METRICS_STEP)
    rows = []
    for j, p in enumerate(probes):
        ts = t0 + (j // 4) * METRICS_STEP
        if j % 4 == 0:
            rows.append(Row(ts, FILLER, FILLER, FILLER_VALUE, None))
        rows.append(Row(ts, METRIC_NAMES[j % 4], p.case, p.value, p))
    return rows


def write_file(path, rows, metrics=False, num_as_text=False):
    """One tile.  num_as_text: the VARCHAR twin the oracle reads for a request grouped by `attr.n`."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    assert len(rows) <= TILE_ROWS and [r.ts for r in rows] == sorted(r.ts for r in rows)
    vals = pa.array([0.0 if r.value is None else r.value for r in rows], pa.float64(),
                    mask=np.array([r.value is None for r in rows]))
    cols = {TIMESTAMP: pa.array([r.ts for r in rows], pa.int64())}
    if metrics:
        cols["rollup_sum"] = vals
        cols["rollup_max"] = vals
    else:
        cols[VALUE] = vals
    cols[NAME] = pa.array([r.name for r in rows], pa.string())
    cols[CASE] = pa.array([r.case for r in rows], pa.string())
    strings = [NAME, CASE]
    if num_as_text:
        cols[NUM] = pa.array([str(NUM_VALUE)] * len(rows), pa.string())
        strings.append(NUM)
    else:
        cols[NUM] = pa.array([NUM_VALUE] * len(rows), pa.int64())
    t = pa.table(cols)
    pq.write_table(t, str(path), compression="NONE", use_dictionary=strings, row_group_size=TILE_ROWS,
                   data_page_size=1 << 20, column_encoding={c: "PLAIN" for c in t.column_names if c not in strings})
    return str(path)


def expected_sketches(rows, names, step, win=None):
    """{(sketch timestamp, case): [probes / None per filler row]} of the rows whose name is in `names` and whose
    timestamp lies in win = [lo, hi): the sketch timestamp is ts - ts % step (logs), or the raw one (step None)."""
    out = collections.defaultdict(list)
    for r in rows:
        if r.name in names and (win is None or win[0] <= r.ts < win[1]):
            out[(r.ts if step is None else r.ts - r.ts % step, r.case)].append(r.probe)
    return dict(out)


GOOD, BAD = "good", "bad"


def untrackable_rows(value, metrics=False):
    """A small file: 60 trackable rows under the name `good` (cases g0 .. g3) and, last, one row of `value` under the
    name `bad`; the bad row's timestamp lies 50 minutes into the hour, every other row in the first 40."""
    from lakeside_amd import synth
    rng = np.random.default_rng(31)
    v = rng.lognormal(0.0, 2.0, 60) * np.where(rng.random(60) < 0.3, -1.0, 1.0)
    grid = METRICS_STEP if metrics else 1
    rows = [Row(synth.T0 + (i * 40 * 60_000 // 60) // grid * grid + (0 if metrics else i), GOOD, f"g{i % 4}", float(v[i]), None)
            for i in range(60)]
    rows.append(Row(synth.T0 + 50 * 60_000, BAD, BAD, value, None))
    return rows


BAD_TS_OFFSET = 50 * 60_000
