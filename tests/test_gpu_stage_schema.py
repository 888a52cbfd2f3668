"""The schema bg_stage_validate reports for a plan equals the schema the
executed plan carries: names and dtypes column by column, and for
Decimal128 columns the executed precision and scale equal the rules written
out here by hand (a join output keeps its source column's type; a Decimal128
sum is precision 38; a decimal avg is precision + 4 capped at 38, scale + 4;
a partial avg's "$s" sum keeps the input precision).

Sizes are the smallest that cross a 64-row validity word (70 build rows),
a probe-chunk edge with a short last chunk (200 rows in chunks of 64) and
the multi-piece concat of a chunked or build-tailed join."""
import decimal

import numpy as np
import pyarrow as pa
import pytest

from datafusion_ballista_amd import gpu, stage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = gpu.GpuStageContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(ctx):
    """Register every input once for the module."""
    rng = np.random.default_rng(83)

    def dec(n, scale_div, typ, null_p):
        vals = rng.integers(-10**6, 10**6, size=n)
        mask = rng.random(n) < null_p
        return pa.array([None if m else decimal.Decimal(int(v)) / scale_div
                         for v, m in zip(vals, mask)], type=typ)

    nb, npr, na = 70, 200, 300
    t = {
        "sch_b": pa.table({
            "bk": pa.array(rng.integers(0, 40, size=nb, dtype=np.int64),
                           mask=rng.random(nb) < 0.1),
            "bid": pa.array(np.arange(nb, dtype=np.int64)),
            "bdec": dec(nb, 100, pa.decimal128(15, 2), 0.2)}),
        "sch_p": pa.table({
            "pk": pa.array(rng.integers(0, 60, size=npr, dtype=np.int64),
                           mask=rng.random(npr) < 0.1),
            "pid": pa.array(np.arange(npr, dtype=np.int64)),
            "pdec": dec(npr, 1000, pa.decimal128(12, 3), 0.2)}),
        "sch_a": pa.table({
            "g": pa.array(rng.integers(0, 7, size=na, dtype=np.int64)),
            "i": pa.array(rng.integers(-10**6, 10**6, size=na,
                                       dtype=np.int64),
                          mask=rng.random(na) < 0.2),
            "d": dec(na, 100, pa.decimal128(15, 2), 0.2),
            "f": pa.array(rng.random(na), mask=rng.random(na) < 0.2)}),
    }
    keep = [stage.register_table(ctx, name, tab) for name, tab in t.items()]
    yield t
    for name in t:
        stage.unregister_table(name)
    del keep


def _doc(plan, **kw):
    d = {"job_id": "job-sch", "stage_id": 1, "task_id": 0,
         "work_dir": "/tmp/stage-tests", "plan": plan}
    d.update(kw)
    return d


def scan_of(tables, name):
    return {"op": "scan", "schema": stage.schema_json(tables[name].schema),
            "source": {"kind": "device", "table": name}}


def check_schema(doc, want):
    """want: [(name, dtype, (precision, scale) | None)].  Returns the
    executed result."""
    validated = stage.validate(doc)["schema"]
    res = stage.execute(doc)
    executed = res["schema"]
    assert [(f["name"], f["dtype"]) for f in validated] == \
        [(f["name"], f["dtype"]) for f in executed]
    got = [(f["name"], f["dtype"],
            (f["precision"], f["scale"]) if f["dtype"] == "decimal128"
            else None) for f in executed]
    assert got == want
    return res


# -- joins ------------------------------------------------------------------
B_OUT = [("bid", "int64", None), ("b_dec", "decimal128", (15, 2))]
P_OUT = [("pid", "int64", None), ("pdec", "decimal128", (12, 3))]
JOIN_TYPES = {  # type -> (build outputs?, probe outputs?)
    "inner": (True, True), "semi": (False, True), "anti": (False, True),
    "left": (True, True), "semi_build": (True, False),
    "anti_build": (True, False), "outer_build": (True, True),
    "full": (True, True)}


def join_rows(tables, jt):
    """Row count of each join type, NULL keys matching nothing."""
    bk = tables["sch_b"]["bk"].to_pylist()
    pk = tables["sch_p"]["pk"].to_pylist()
    per_probe = [0 if k is None else sum(1 for b in bk if b == k)
                 for k in pk]
    inner = sum(per_probe)
    lone_probe = sum(1 for m in per_probe if m == 0)
    hit = {k for k in pk if k is not None}
    hit_build = sum(1 for b in bk if b is not None and b in hit)
    lone_build = len(bk) - hit_build
    return {"inner": inner, "semi": len(pk) - lone_probe, "anti": lone_probe,
            "left": inner + lone_probe, "semi_build": hit_build,
            "anti_build": lone_build, "outer_build": inner + lone_build,
            "full": inner + lone_probe + lone_build}[jt]


@pytest.mark.parametrize("chunk", [0, 64], ids=["whole", "chunk64"])
@pytest.mark.parametrize("jt", list(JOIN_TYPES))
def test_join_schema(ctx, tables, jt, chunk):
    with_build, with_probe = JOIN_TYPES[jt]
    output, want = [], []
    if with_build:
        output += [{"side": "build", "col": "bid"},
                   {"side": "build", "col": "bdec", "as": "b_dec"}]
        want += B_OUT
    if with_probe:
        output += [{"side": "probe", "col": "pid"},
                   {"side": "probe", "col": "pdec"}]
        want += P_OUT
    plan = {"op": "hash_join", "build": scan_of(tables, "sch_b"),
            "probe": scan_of(tables, "sch_p"), "build_keys": ["bk"],
            "probe_keys": ["pk"], "join_type": jt, "output": output}
    if chunk:
        plan["probe_chunk_rows"] = chunk
    res = check_schema(_doc({"op": "collect", "input": plan}), want)
    assert len(res["rows"]) == join_rows(tables, jt)


# -- aggregates -------------------------------------------------------------
AGGS = [{"fn": "sum", "as": "sd", "expr": {"col": "d"}},
        {"fn": "sum", "as": "si", "expr": {"col": "i"}},
        {"fn": "min", "as": "mi", "expr": {"col": "i"}},
        {"fn": "max", "as": "mf", "expr": {"col": "f"}},
        {"fn": "count", "as": "ci", "expr": {"col": "i"}},
        {"fn": "count", "as": "cs"},
        {"fn": "avg", "as": "ad", "expr": {"col": "d"}},
        {"fn": "avg", "as": "af", "expr": {"col": "f"}}]
FINAL_SCHEMA = [
    ("g", "int64", None), ("sd", "decimal128", (38, 2)),
    ("si", "int64", None), ("mi", "int64", None), ("mf", "float64", None),
    ("ci", "int64", None), ("cs", "int64", None),
    ("ad", "decimal128", (19, 6)), ("af", "float64", None)]
PARTIAL_SCHEMA = [
    ("g", "int64", None),
    ("sd", "decimal128", (38, 2)), ("sd$n", "int64", None),
    ("si", "int64", None), ("si$n", "int64", None),
    ("mi", "int64", None), ("mi$n", "int64", None),
    ("mf", "float64", None), ("mf$n", "int64", None),
    ("ci", "int64", None), ("cs", "int64", None),
    ("ad$s", "decimal128", (15, 2)), ("ad$n", "int64", None),
    ("af$s", "float64", None), ("af$n", "int64", None)]


def agg_node(mode, inp, aggs=AGGS):
    return {"op": "hash_aggregate", "mode": mode, "group_by": ["g"],
            "aggs": aggs, "input": inp}


def test_single_aggregate_schema(ctx, tables):
    res = check_schema(_doc({"op": "collect", "input": agg_node(
        "single", scan_of(tables, "sch_a"))}), FINAL_SCHEMA)
    assert len(res["rows"]) == 7


def test_partial_schema(ctx, tables):
    res = check_schema(_doc({"op": "collect", "input": agg_node(
        "partial", scan_of(tables, "sch_a"))}), PARTIAL_SCHEMA)
    assert len(res["rows"]) == 7


def test_partial_final_schema_over_shuffle(ctx, tables, tmp_path):
    # the hash-repartitioning writer carries no float64 payload, so the
    # aggregates over "f" stay with the collect-rooted tests above; and a
    # final aggregate spends two of the kernel's eight slots on each
    # sum/min/avg (value + "$n"), one on each count: 2+2+1+1+2 = 8
    aggs = [a for a in AGGS if a["as"] in ("sd", "mi", "ci", "cs", "ad")]
    kept = {"g"} | {a["as"] for a in aggs}
    partial_schema = [f for f in PARTIAL_SCHEMA if f[0].split("$")[0] in kept]
    final_schema = [f for f in FINAL_SCHEMA if f[0] in kept]
    assert len(aggs) == 5 and len(partial_schema) == 9

    partial = agg_node("partial", scan_of(tables, "sch_a"), aggs)
    # what the partial stage emits is what the shuffle file carries
    part_schema = pa.schema([(n, pa.decimal128(*ps) if ps else pa.int64())
                             for n, _, ps in partial_schema])
    wdoc = _doc({"op": "sort_shuffle_write", "k": 1, "keys": [{"col": "g"}],
                 "input": partial}, work_dir=str(tmp_path),
                schema_msg_hex=stage.schema_msg_hex(part_schema))
    assert [(f["name"], f["dtype"]) for f in stage.validate(wdoc)["schema"]] \
        == [(n, dt) for n, dt, _ in partial_schema]
    path = stage.execute(wdoc)["partitions"][0]["path"]

    scan = {"op": "scan", "schema": stage.schema_json(part_schema),
            "source": {"kind": "shuffle", "data": path,
                       "index": path + ".index", "partitions": [0]}}
    final_aggs = [{"fn": a["fn"], "as": a["as"]} for a in aggs]
    res = check_schema(_doc({"op": "collect", "input": agg_node(
        "final", scan, final_aggs)}), final_schema)
    assert len(res["rows"]) == 7
