#!/usr/bin/env python3
"""Join residual filters at q13's SF100 sizes: customer (15 M rows, the
build side) against orders (150 M rows), dbgen-shaped keys, one Int64 filter
column on each side (c_x = c_custkey % 7, o_x = order number % 7, so
`c_x != o_x` passes about 6 candidates in 7).

Measured, each as the median and min..max of REPEATS warm runs, the two
plans of a pair alternated run by run in this one process:
  fused / emulated     inner join with filter {cross: c_x ne o_x}, against
                       the plan that gave the same rows before: inner join
                       (the Int64 fast path) with both filter columns in its
                       output, then a filter node with rhs.  The fused plan
                       must not be slower than the emulation by more than the
                       emulation's own min..max spread ("within_bar").
  semi_build_filtered  semi_build with a one-term filter that passes every
  / semi_build         candidate (c_x < 7), against semi_build without one:
                       what the filter itself costs.  Recorded only.
  abi_breakdown        where the fused plan's time goes: count + fill of the
                       inner join at the C ABI, through the Int64 fast table
                       (what the emulation's join runs on), the general table
                       without a filter, and the general table with the
                       `ne` filter (what the fused plan runs on).
Every join feeds a no-group sum+count, so no plan pays for shipping rows to
the host; the two plans of a pair must report the same count and key sum.
Each timed step runs under its own time limit: a watchdog ends the process
if one overruns."""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from datafusion_ballista_amd import gpu  # noqa: E402

N_BUILD = 15_000_000
N_PROBE = 150_000_000
REPEATS = 5
STEP_LIMIT_S = 120

CUSTOMER = [{"name": "c_custkey", "dtype": "int64"},
            {"name": "c_x", "dtype": "int64"}]
ORDERS = [{"name": "o_orderkey", "dtype": "int64"},
          {"name": "o_custkey", "dtype": "int64"},
          {"name": "o_x", "dtype": "int64"},
          {"name": "o_seven", "dtype": "int64"}]


def scan(name, schema):
    return {"op": "scan", "schema": schema,
            "source": {"kind": "device", "table": name}}


def doc(join_type, filt=None, extra_output=(), after=None):
    """sum(c_custkey) + count over a customer-build / orders-probe join;
    `after` wraps the join (the emulation's filter node)."""
    output = [{"side": "build", "col": "c_custkey"}]
    if join_type == "inner":
        output.append({"side": "probe", "col": "o_orderkey"})
    output += list(extra_output)
    join = {"op": "hash_join", "join_type": join_type, "output": output,
            "build": scan("customer", CUSTOMER),
            "probe": scan("orders", ORDERS),
            "build_keys": ["c_custkey"], "probe_keys": ["o_custkey"]}
    if filt:
        join["filter"] = filt
    if after:
        join = dict(after, input=join)
    return {"job_id": "perf-jf", "stage_id": 1, "task_id": 0,
            "work_dir": "/tmp/perf-jf",
            "plan": {"op": "collect", "input": {
                "op": "hash_aggregate", "mode": "single", "group_by": [],
                "aggs": [{"fn": "sum", "as": "s",
                          "expr": {"col": "c_custkey"}},
                         {"fn": "count", "as": "c"}],
                "input": join}}}


def cross(cmp, probe_col):
    return {"any": [{"cross": [{"build": "c_x", "cmp": cmp,
                                "probe": probe_col}]}]}


PAIRS = {
    "inner_ne": {
        "fused": doc("inner", cross("ne", "o_x")),
        "emulated": doc(
            "inner",
            extra_output=[{"side": "build", "col": "c_x"},
                          {"side": "probe", "col": "o_x"}],
            after={"op": "filter", "predicates": [
                {"col": "c_x", "cmp": "ne", "rhs": {"col": "o_x"}}]}),
    },
    "semi_build_all_pass": {
        "semi_build_filtered": doc("semi_build", cross("lt", "o_seven")),
        "semi_build": doc("semi_build"),
    },
}


class Lib:
    """The library with the two tables registered."""

    def __init__(self, tables):
        self.L = gpu.load_library()
        assert self.L.bg_init(0) == 0
        self.hash = self.L.bg_source_hash().decode()
        for name, cols in tables.items():
            arr = (gpu.BgColumn * len(cols))()
            names = (ctypes.c_char_p * len(cols))()
            for i, (cn, t) in enumerate(cols):
                arr[i] = gpu.BgColumn(gpu.BG_DT_INT64, 0, 0, 0,
                                      ctypes.c_void_p(t.data_ptr()), None,
                                      None, t.shape[0])
                names[i] = cn.encode()
            assert self.L.bg_stage_register_table(
                name.encode(), arr, names, len(cols),
                cols[0][1].shape[0]) == 0

    def run(self, plan_doc):
        """-> (seconds, [sum, count]); the call returns its result rows, so
        the device work has finished when it does."""
        out = ctypes.c_char_p()
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        t0 = time.perf_counter()
        rc = self.L.bg_execute_stage(json.dumps(plan_doc).encode(),
                                     ctypes.byref(out))
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        if rc != 0:
            raise RuntimeError(self.L.bg_last_error().decode())
        row = json.loads(out.value.decode())["rows"][0]
        return dt, [int(row[0]), int(row[1])]


def abi_breakdown(L, c_custkey, c_x, o_custkey, o_x):
    """Count + fill of the inner join, seconds per phase (median of REPEATS
    after one warm-up), on the three probe paths."""
    def col(t):
        return (gpu.BgColumn * 1)(gpu.BgColumn(
            gpu.BG_DT_INT64, 0, 0, 0, ctypes.c_void_p(t.data_ptr()), None,
            None, t.shape[0]))

    bkey, pkey, n = col(c_custkey), col(o_custkey), o_custkey.shape[0]
    term = (gpu.BgJoinFilterTerm * 1)(gpu.BgJoinFilterTerm(
        gpu.BG_JF_CROSS, 0, gpu.BG_DT_INT64, gpu.BG_CMP_NE, c_x.data_ptr(),
        None, o_x.data_ptr(), None))
    out_p = torch.empty(n, dtype=torch.int32, device=o_custkey.device)
    out_b = torch.empty(n, dtype=torch.int32, device=o_custkey.device)
    m = ctypes.c_int64()

    def ok(rc):
        if rc != 0:
            raise RuntimeError(L.bg_last_error().decode())

    def timed(call):
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        ok(L.bg_synchronize())
        t0 = time.perf_counter()
        ok(call())
        ok(L.bg_synchronize())
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        return dt

    fast, general = ctypes.c_void_p(), ctypes.c_void_p()
    ok(L.bg_hashjoin_build(bkey, c_custkey.shape[0], ctypes.byref(fast)))
    ok(L.bg_hashjoin_build2(bkey, 1, c_custkey.shape[0],
                            ctypes.byref(general)))
    op, ob = out_p.data_ptr(), out_b.data_ptr()
    paths = {
        "int64_fast_table": (
            lambda: L.bg_hashjoin_probe_count(fast, pkey, n, ctypes.byref(m)),
            lambda: L.bg_hashjoin_probe_fill(fast, pkey, n, op, ob)),
        "general_table": (
            lambda: L.bg_hashjoin_probe_count2(general, pkey, 1, n, 0,
                                               ctypes.byref(m)),
            lambda: L.bg_hashjoin_probe_fill2(general, pkey, 1, n, 0, op,
                                              ob)),
        "general_table_filtered": (
            lambda: L.bg_hashjoin_probe_count2_filtered(
                general, pkey, 1, n, 0, term, 1, ctypes.byref(m)),
            lambda: L.bg_hashjoin_probe_fill2_filtered(
                general, pkey, 1, n, 0, term, 1, op, ob)),
    }
    rec = {}
    for name, (count, fill) in paths.items():
        tc, tf = [], []
        for i in range(REPEATS + 1):
            c = timed(count)
            assert 0 < m.value <= n      # the pair buffers hold n pairs
            f = timed(fill)
            if i:                        # run 0 warms up
                tc.append(c)
                tf.append(f)
        rec[name] = {"pairs": m.value, "count": spread(tc),
                     "fill": spread(tf)}
    ok(L.bg_hashjoin_free(fast))
    ok(L.bg_hashjoin_free2(general))
    return rec


def spread(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs),
            "max_s": max(xs), "runs_s": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "perf_join_filter.json"))
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrink both sides (rehearsal only)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    nb, npr = int(N_BUILD * args.scale), int(N_PROBE * args.scale)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    c_custkey = torch.arange(1, nb + 1, device=dev, dtype=torch.int64)
    c_x = c_custkey % 7
    # buyers are the custkeys that are no multiple of 3, as in dbgen
    r = torch.randint(0, nb // 3 * 2, (npr,), generator=g, device=dev,
                      dtype=torch.int64)
    o_custkey = r + r // 2 + 1
    del r
    number = torch.arange(npr, device=dev, dtype=torch.int64)
    o_x = number % 7
    tables = {"customer": [("c_custkey", c_custkey),
                           ("c_x", c_x)],
              "orders": [("o_orderkey", number * 4 + 1),
                         ("o_custkey", o_custkey),
                         ("o_x", o_x),
                         ("o_seven", torch.full_like(number, 7))]}
    del number
    torch.cuda.synchronize()
    lib = Lib(tables)
    rec = {"build_rows": nb, "probe_rows": npr, "repeats": REPEATS,
           "timing": "host clock around bg_execute_stage (returns rows, so "
                     "device work is complete); 1 warm-up run per plan; the "
                     "plans of a pair alternate",
           "source_hash": lib.hash, "pairs": {}}
    for pair, docs in PAIRS.items():
        results = {}
        for name, d in docs.items():
            _, results[name] = lib.run(d)               # warm-up
        times = {name: [] for name in docs}
        for _ in range(REPEATS):                        # alternated
            for name, d in docs.items():
                dt, res = lib.run(d)
                assert res == results[name]
                times[name].append(dt)
        (na, a), (nb_, b) = results.items()
        assert a == b, f"{pair}: {na} {a} != {nb_} {b}"
        out = {name: dict(spread(times[name]), sum_custkey=results[name][0],
                          rows=results[name][1]) for name in docs}
        new, old = (out[n] for n in docs)
        out["first_minus_second_median_s"] = new["median_s"] - old["median_s"]
        out["second_min_max_spread_s"] = old["max_s"] - old["min_s"]
        if pair == "inner_ne":
            out["within_bar"] = (out["first_minus_second_median_s"]
                                 <= out["second_min_max_spread_s"])
        rec["pairs"][pair] = out
        print(json.dumps({pair: {k: v["median_s"] if isinstance(v, dict)
                                 else v for k, v in out.items()}}),
              flush=True)
    rec["abi_breakdown"] = abi_breakdown(lib.L, c_custkey, c_x, o_custkey,
                                         o_x)
    print(json.dumps({"abi_breakdown": {
        k: {"pairs": v["pairs"], "count_median_s": v["count"]["median_s"],
            "fill_median_s": v["fill"]["median_s"]}
        for k, v in rec["abi_breakdown"].items()}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
