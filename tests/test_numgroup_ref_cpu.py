"""tests/numgroup_ref.py pinned against the reference's own SQL: for all-INT64, INT32 + INT64 and all-DOUBLE (no NaN)
globs, `GROUP BY step_ts, "status", name` run on SQLite over the *original* files (oracle.sqlplan.run_sql) gives the
rows the oracle gives over the VARCHAR twins.  SQLite's group values print as Python prints them, so the DOUBLE tags
are mapped through numeric_tag_text({"float64"}, float(s)); integers print alike.  SQLite cannot pin NaN (stored as
NULL) or mixed integer / float unions (2^53 + 1 stays an integer there): those rest on numeric_tag_text, which the
numeric tag cases (tests/golden/numtag_cases.json) pin.  Bar: tests/test_oracle.py's -- tags, timestamps, counts, min
and max exact; sums within 1e-12 relative."""
import json
import math

import pytest

from oracle import dataexpr as dx
from oracle import sqlplan
from tests import numgroup_data as nd
from tests import numgroup_ref as nr

UNIONS = {"int64": ("A", "A"), "int32_int64": ("D", "A"), "double": ("Bfinite", "Bfinite")}


@pytest.fixture(scope="module")
def globs(tmp_path_factory):
    root = tmp_path_factory.mktemp("numgroup_ref")
    out = {}
    for k, (name, kinds) in enumerate(UNIONS.items()):
        paths = [nd.write_file(root / f"{name}_{j}.parquet", kind, seed=100 + 10 * k + j, rows=700 + 50 * j)
                 for j, kind in enumerate(kinds)]
        out[name] = (paths, nr.write_twins(paths, [nd.STATUS], 2, str(root / f"twins_{name}")))
    return out


def _request(agg):
    from lakeside_amd import synth
    segs = [synth.segment_request(i, hour=0) for i in range(2)]
    return json.dumps(synth.pushdown(synth.leaf(synth.NAME, "in", "metric_00", "metric_02"), segs, agg, [nd.STATUS]))


@pytest.mark.parametrize("agg", ["sum", "count", "min", "max"])
@pytest.mark.parametrize("union", list(UNIONS))
def test_twins_match_reference_sql(globs, union, agg):
    paths, twins = globs[union]
    pr = dx.parse_pushdown(_request(agg))
    want = []
    for ts, v, tags in sqlplan.run_sql(pr, [0, 1], paths):
        if union == "double" and nd.STATUS in tags:
            tags = dict(tags, **{nd.STATUS: dx.numeric_tag_text({"float64"}, float(tags[nd.STATUS]))})
        want.append((ts, v, tags))
    got = dx.evaluate_per_glob(pr, twins, 2)[0]
    key = lambda r: (r[0], sorted(r[2].items()))   # noqa: E731
    got, want = sorted(got, key=key), sorted(want, key=key)
    assert len(got) > 100
    assert [key(r) for r in got] == [key(r) for r in want]
    assert any(nd.STATUS not in r[2] for r in got), "NULL status rows group apart, their tag absent"
    for g, w in zip(got, want):
        if agg == "sum":
            assert math.isclose(g[1], w[1], rel_tol=1e-12, abs_tol=0.0) or g[1] == w[1], (g, w)
        else:
            assert g[1] == w[1], (g, w)


def test_twin_text_of_the_union_type(tmp_path):
    """What SQLite cannot pin, stated once: the union type decides the text, NULL stays NULL, every NaN is one text."""
    import pyarrow.parquet as pq
    paths = [nd.write_file(tmp_path / "a.parquet", "A", 1, rows=400), nd.write_file(tmp_path / "b.parquet", "B", 2, rows=400),
             nd.write_file(tmp_path / "d.parquet", "D", 3, rows=400), nd.write_file(tmp_path / "c.parquet", "C", 4, rows=400),
             nd.write_file(tmp_path / "f.parquet", "F", 5, rows=400), nd.write_file(tmp_path / "g.parquet", "G", 6, rows=400)]
    twins = nr.write_twins(paths, [nd.STATUS], 2, str(tmp_path / "twins"))
    texts = [set(pq.read_table(p).column(nd.STATUS).to_pylist()) if i != 4 else None for i, p in enumerate(twins)]
    # {A, B}: DOUBLE -- 2^53 + 1 joins 2^53, 200 prints as 200.0, -1 as -1.0
    # (2^62 and 1e23 as Java 17's Double.toString prints them: not the shortest digits)
    from oracle.exemplar import java_double_text
    assert java_double_text(2.0 ** 62) == "4.6116860184273879E18" and java_double_text(1e23) == "9.999999999999999E22"
    assert texts[0] == {None, "200.0", "404.0", "500.0", "-1.0", "9.007199254740992E15", "4.6116860184273879E18",
                        "-9.223372036854776E18"}
    assert texts[1] == {None, "200.0", "0.0", "NaN", "9.999999999999999E22", "9.007199254740992E15", "0.1"}
    # {D, C}: FLOAT -- 2^24 + 1 joins 2^24
    assert texts[2] == {None, "200.0", "404.0", "-1.0", "1.6777216E7"}
    assert texts[3] == {None, "200.0", "0.1", "1.6777216E7", "NaN", "0.0"}
    # {F, G}: the column exists in the glob (all NULL); F's twin still has no such column
    assert nd.STATUS not in pq.read_table(twins[4]).column_names
    assert texts[5] == {None}
