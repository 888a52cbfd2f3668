#!/usr/bin/env python3
"""Stage-interpreter fuzz: random tables (dtypes x NULLs x cardinalities)
through random plan trees (filter -> optional hash join -> group-by
aggregate [-> sort/limit]), every run checked against pyarrow compute.
Covers the plan grammar end to end: expression eval, LIKE, join types with
and without a residual filter, nested-loop joins (no keys) on all eight
types, partial/final over a real shuffle file round trip (every 5th round).

Usage: python scripts/fuzz_stage.py [rounds] [seed]"""
import decimal
import operator
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import pyarrow.compute as pc  # noqa: E402

from datafusion_ballista_amd import gpu, stage  # noqa: E402


def rand_table(rng, n, with_utf8=True):
    cols = {"k": pa.array(rng.integers(0, max(2, n // 50), size=n,
                                       dtype=np.int64))}
    vmask = rng.random(n) < rng.choice([0.0, 0.25])
    cols["v"] = pa.array(rng.integers(-10**8, 10**8, size=n,
                                      dtype=np.int64), mask=vmask)
    cols["d"] = pa.array(rng.integers(8000, 11000, size=n,
                                      dtype=np.int32), type=pa.date32())
    cols["x"] = pa.array(rng.standard_normal(n))
    # Decimal(38,2) over both limbs and both signs (min/max compare i128)
    pmask = rng.random(n) < rng.choice([0.0, 0.25])
    wide = [int(a) * int(b) for a, b in zip(
        rng.integers(-2**62, 2**62, size=n), rng.integers(0, 2**62, size=n))]
    cols["p"] = pa.array(
        [None if m else decimal.Decimal(
            (1 if w < 0 else 0, tuple(int(c) for c in str(abs(w))), -2))
         for w, m in zip(wide, pmask)], type=pa.decimal128(38, 2))
    if with_utf8:
        words = ["PROMO A", "alpha green", "BRASS x", "", "special req",
                 "zed"]
        smask = rng.random(n) < rng.choice([0.0, 0.1])
        cols["s"] = pa.array(
            [None if m else words[i % len(words)] + str(i % 13)
             for i, m in enumerate(smask)])
    return pa.table(cols)


def run_round(ctx, rng, trial, tmpdir):
    n = int(rng.integers(100, 30_000))
    t = rand_table(rng, n)
    name = f"fz{trial}"
    keep = stage.register_table(ctx, name, t)
    scan = {"op": "scan", "schema": stage.schema_json(t.schema),
            "source": {"kind": "device", "table": name}}
    doc = lambda plan, **kw: {  # noqa: E731
        "job_id": f"fz{trial}", "stage_id": 1, "task_id": 0,
        "work_dir": tmpdir, "plan": plan, **kw}

    # random filter
    preds = []
    lo = int(rng.integers(8000, 10500))
    hi = lo + int(rng.integers(50, 2000))
    which = rng.integers(0, 4)
    mask = np.ones(n, dtype=bool)
    d_np = t["d"].to_numpy().astype("datetime64[D]").astype(np.int64)
    if which == 0:
        preds = [{"col": "d", "cmp": "ge_lt", "lo": lo, "hi": hi}]
        mask = (d_np >= lo) & (d_np < hi)
    elif which == 1:
        preds = [{"col": "d", "cmp": "lt", "hi": hi}]
        mask = d_np < hi
    elif which == 2:
        import re
        pat = str(rng.choice(["PROMO%", "%green%", "%x1%", "%req%"]))
        preds = [{"col": "s", "like": pat}]
        body = ".*".join(re.escape(f) for f in pat.split("%") if f)
        if pat.startswith("%"):
            body = ".*" + body
        if pat.endswith("%"):
            body = body + ".*"
        rx = re.compile(body, re.S)
        sv = t["s"].to_pylist()
        mask = np.array([v is not None and bool(rx.fullmatch(v))
                         for v in sv])
    else:
        preds = []

    ft = t.filter(pa.array(mask)) if preds else t
    plan = {"op": "filter", "predicates": preds, "input": scan} if preds \
        else scan

    # group-by aggregate
    agg_plan = {"op": "hash_aggregate", "mode": "single",
                "group_by": ["k"],
                "aggs": [{"fn": "sum", "as": "sv", "expr": {"col": "v"}},
                         {"fn": "min", "as": "mn", "expr": {"col": "v"}},
                         {"fn": "max", "as": "mxx", "expr": {"col": "x"}},
                         {"fn": "count", "as": "c"},
                         {"fn": "avg", "as": "ax", "expr": {"col": "x"}}],
                "input": plan}
    res = stage.execute(doc({"op": "collect", "input": agg_plan}))
    if ft.num_rows:
        want = ft.group_by("k").aggregate(
            [("v", "sum"), ("v", "min"), ("x", "max"), ("k", "count"),
             ("x", "mean")]).sort_by("k")
        got = sorted(res["rows"], key=lambda r: r[0])
        assert len(got) == want.num_rows, (trial, len(got), want.num_rows)
        for i, r in enumerate(got):
            assert r[0] == want["k"][i].as_py()
            assert r[1] == want["v_sum"][i].as_py(), (trial, "sum", r)
            assert r[2] == want["v_min"][i].as_py(), (trial, "min", r)
            wx = want["x_max"][i].as_py()
            assert (r[3] is None) == (wx is None)
            if wx is not None:
                assert abs(r[3] - wx) < 1e-12
            assert r[4] == want["k_count"][i].as_py()
    else:
        assert res["rows"] == []

    # min/max over a decimal, a string and a date column (the row-index
    # accumulators and the 32-bit ops), exact against pyarrow
    mm_cols = ["p", "s", "d"]
    mm_plan = {"op": "hash_aggregate", "mode": "single", "group_by": ["k"],
               "aggs": [{"fn": fn, "as": f"{c}_{fn}", "expr": {"col": c}}
                        for c in mm_cols for fn in ("min", "max")],
               "input": plan}
    res = stage.execute(doc({"op": "collect", "input": mm_plan}))
    if ft.num_rows:
        want = ft.group_by("k").aggregate(
            [(c, fn) for c in mm_cols for fn in ("min", "max")]).sort_by("k")

        def cells(col):
            if pa.types.is_decimal(col.type):  # unscaled int, exact
                out = []
                for dv in col.to_pylist():
                    if dv is None:
                        out.append(None)
                        continue
                    sign, digits, _ = dv.as_tuple()
                    iv = int("".join(map(str, digits)))
                    out.append(str(-iv if sign else iv))
                return out
            if pa.types.is_date32(col.type):
                return col.cast(pa.int32()).to_pylist()
            return col.to_pylist()

        got = sorted(res["rows"], key=lambda r: r[0])
        assert len(got) == want.num_rows, (trial, len(got), want.num_rows)
        assert [r[0] for r in got] == want["k"].to_pylist()
        for j, nm in enumerate(f"{c}_{fn}" for c in mm_cols
                               for fn in ("min", "max")):
            assert [r[1 + j] for r in got] == cells(want[nm]), (trial, nm)
    else:
        assert res["rows"] == []

    # every 5th: two-phase partial -> shuffle file -> final
    if trial % 5 == 0 and ft.num_rows:
        part_schema = pa.schema([
            ("k", pa.int64()), ("sv", pa.int64()), ("sv$n", pa.int64()),
            ("c", pa.int64())])
        partial = {"op": "hash_aggregate", "mode": "partial",
                   "group_by": ["k"],
                   "aggs": [{"fn": "sum", "as": "sv", "expr": {"col": "v"}},
                            {"fn": "count", "as": "c"}],
                   "input": plan}
        k = int(rng.integers(2, 6))
        r1 = stage.execute(doc(
            {"op": "sort_shuffle_write", "k": k, "keys": [{"col": "k"}],
             "input": partial},
            schema_msg_hex=stage.schema_msg_hex(part_schema)))
        pth = r1["partitions"][0]["path"]
        final = {"op": "hash_aggregate", "mode": "final", "group_by": ["k"],
                 "aggs": [{"fn": "sum", "as": "sv"},
                          {"fn": "count", "as": "c"}],
                 "input": {"op": "scan",
                           "schema": stage.schema_json(part_schema),
                           "source": {"kind": "shuffle", "data": pth,
                                      "index": pth + ".index",
                                      "partitions": list(range(k))}}}
        res2 = stage.execute(doc({"op": "collect", "input": final}))
        want = ft.group_by("k").aggregate(
            [("v", "sum"), ("k", "count")]).sort_by("k")
        got = sorted(res2["rows"], key=lambda r: r[0])
        assert len(got) == want.num_rows
        for i, r in enumerate(got):
            assert r[0] == want["k"][i].as_py()
            assert r[1] == want["v_sum"][i].as_py(), (trial, "2p sum", r)
            assert r[2] == want["k_count"][i].as_py()

    # random join type against build side
    jt = str(rng.choice(["inner", "semi", "anti", "left"]))
    nb = int(rng.integers(10, 500))
    bkeys = rng.choice(np.arange(0, max(2, n // 50), dtype=np.int64),
                       size=nb, replace=True)
    ubk = np.unique(bkeys)
    bw = rng.integers(-10**8, 10**8, size=len(ubk), dtype=np.int64)
    bwmask = rng.random(len(ubk)) < 0.1
    bt = pa.table({"bk": pa.array(ubk),
                   "bv": pa.array(np.arange(len(ubk), dtype=np.int64)),
                   "bw": pa.array(bw, mask=bwmask)})
    keep2 = stage.register_table(ctx, name + "b", bt)
    jp = {"op": "hash_join",
          "build": {"op": "scan", "schema": stage.schema_json(bt.schema),
                    "source": {"kind": "device", "table": name + "b"}},
          "probe": scan, "build_keys": ["bk"], "probe_keys": ["k"],
          "join_type": jt,
          "output": [{"side": "probe", "col": "k"}]}
    # build keys are unique: a probe row has at most one candidate, and
    # matches when that candidate passes the filter (if there is one)
    bw_of = {int(k): None if m else int(w)
             for k, w, m in zip(ubk, bw, bwmask)}
    kv = t["k"].to_numpy()
    matched = np.array([int(x) in bw_of for x in kv])
    if rng.random() < 0.5:
        cmp = str(rng.choice(["lt", "le", "gt", "ge", "eq", "ne"]))
        groups = [{"cross": [{"build": "bw", "cmp": cmp, "probe": "v"}]}]
        op = getattr(operator, cmp)
        vv = t["v"].to_pylist()
        ok = np.array([matched[i] and vv[i] is not None and
                       bw_of[int(kv[i])] is not None and
                       op(bw_of[int(kv[i])], vv[i]) for i in range(n)])
        if rng.random() < 0.5:      # OR a probe-side group
            cut = int(rng.integers(8000, 11000))
            groups.append({"probe": [{"col": "d", "cmp": "lt", "hi": cut}]})
            ok |= matched & (d_np < cut)
        jp["filter"] = {"any": groups}
        matched = ok
    res3 = stage.execute(doc({"op": "collect", "input": jp}))
    if jt == "inner" or jt == "semi":
        want_n = int(matched.sum())
    elif jt == "anti":
        want_n = n - int(matched.sum())
    else:
        want_n = n
    assert len(res3["rows"]) == want_n, (trial, jt, len(res3["rows"]),
                                         want_n)

    # nested-loop join (no keys): a small build side (at most 64 rows)
    # against the whole table under a random cross compare, any of the eight
    # types, checked like the join above by its row count (counted on the
    # device: an inner nested-loop join can emit nb * n rows)
    njt = str(rng.choice(["inner", "semi", "anti", "left", "semi_build",
                          "anti_build", "outer_build", "full"]))
    nnb = int(rng.integers(1, 65))
    nw = rng.integers(-10**8, 10**8, size=nnb, dtype=np.int64)
    nwmask = rng.random(nnb) < 0.1
    nt = pa.table({"bv": pa.array(np.arange(nnb, dtype=np.int64)),
                   "bw": pa.array(nw, mask=nwmask)})
    keep3 = stage.register_table(ctx, name + "n", nt)
    build_only = njt in ("semi_build", "anti_build")
    nj = {"op": "nested_loop_join",
          "build": {"op": "scan", "schema": stage.schema_json(nt.schema),
                    "source": {"kind": "device", "table": name + "n"}},
          "probe": scan, "join_type": njt,
          "output": [{"side": "build", "col": "bv"} if build_only
                     else {"side": "probe", "col": "k"}]}
    if rng.random() < 0.5:
        nj["probe_chunk_rows"] = int(rng.integers(64, 4096))
    v_ok = ~t["v"].is_null().to_numpy()
    v_i = pc.fill_null(t["v"], 0).to_numpy()
    passing = np.ones((nnb, n), dtype=bool)            # no filter: cross join
    if rng.random() < 0.8:
        cmp = str(rng.choice(["lt", "le", "gt", "ge", "eq", "ne"]))
        groups = [{"cross": [{"build": "bw", "cmp": cmp, "probe": "v"}]}]
        passing = (getattr(operator, cmp)(nw[:, None], v_i[None, :]) &
                   ~nwmask[:, None] & v_ok[None, :])
        if rng.random() < 0.5:      # OR a probe-side group
            cut = int(rng.integers(8000, 11000))
            groups.append({"probe": [{"col": "d", "cmp": "lt", "hi": cut}]})
            passing = passing | (d_np < cut)[None, :]
        nj["filter"] = {"any": groups}
    pairs = int(passing.sum())
    lone_probe = n - int(passing.any(axis=0).sum())
    lone_build = nnb - int(passing.any(axis=1).sum())
    want_n = {"inner": pairs, "semi": n - lone_probe, "anti": lone_probe,
              "left": pairs + lone_probe, "semi_build": nnb - lone_build,
              "anti_build": lone_build, "outer_build": pairs + lone_build,
              "full": pairs + lone_probe + lone_build}[njt]
    res4 = stage.execute(doc({"op": "collect", "input": {
        "op": "hash_aggregate", "mode": "single", "group_by": [],
        "aggs": [{"fn": "count", "as": "c"}], "input": nj}}))
    got_n = res4["rows"][0][0] if res4["rows"] else 0
    assert got_n == want_n, (trial, "nested_loop_join", njt, got_n, want_n)

    stage.unregister_table(name)
    stage.unregister_table(name + "b")
    stage.unregister_table(name + "n")
    del keep, keep2, keep3


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time())
    print(f"STAGE FUZZ seed={seed} rounds={rounds}", flush=True)
    rng = np.random.default_rng(seed)
    ctx = gpu.GpuStageContext(0)
    t0 = time.time()
    with tempfile.TemporaryDirectory() as td:
        for trial in range(rounds):
            run_round(ctx, rng, trial, td)
            if (trial + 1) % 10 == 0:
                print(f"round {trial+1}: ok ({time.time()-t0:.1f}s)",
                      flush=True)
    print(f"STAGE FUZZ OK: {rounds} rounds in {time.time()-t0:.1f}s",
          flush=True)


if __name__ == "__main__":
    main()
