#!/usr/bin/env python3
"""Build-side-preserving joins at q13's SF100 sizes: customer (15 M rows,
the build side) against orders (150 M rows), dbgen-shaped keys (every third
customer places no order, ~15 orders per buying customer).

Measured, each as the median of REPEATS warm runs in this one process:
  semi_build / outer_build      hash table on customer, orders probes
  swapped semi / swapped left   the only plan that gave the same rows
                                before: hash table on ORDERS, customer
                                probes (the existing probe-preserving types)
  inner                         the untouched Int64 fast path, on this
                                library and - with --parent-lib - on the
                                parent commit's library, alternated run by
                                run, next to the parent's own spread
Every join feeds a no-group sum+count, so no plan pays for shipping rows to
the host and both plans of a pair aggregate the same rows; the two plans of
a pair must report the same count and sum.  Each timed step runs under its
own time limit: a watchdog ends the process if one overruns."""
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

CUSTOMER = [{"name": "c_custkey", "dtype": "int64"}]
ORDERS = [{"name": "o_orderkey", "dtype": "int64"},
          {"name": "o_custkey", "dtype": "int64"}]


def scan(name, schema):
    return {"op": "scan", "schema": schema,
            "source": {"kind": "device", "table": name}}


def plan(join_type, swapped):
    cust, orders = scan("customer", CUSTOMER), scan("orders", ORDERS)
    cside = "probe" if swapped else "build"
    output = [{"side": cside, "col": "c_custkey"}]
    if join_type in ("outer_build", "left", "inner"):
        output.append({"side": "build" if swapped else "probe",
                       "col": "o_orderkey"})
    join = {"op": "hash_join", "join_type": join_type, "output": output,
            "build": orders if swapped else cust,
            "probe": cust if swapped else orders,
            "build_keys": ["o_custkey" if swapped else "c_custkey"],
            "probe_keys": ["c_custkey" if swapped else "o_custkey"]}
    return {"job_id": "perf-jbs", "stage_id": 1, "task_id": 0,
            "work_dir": "/tmp/perf-jbs",
            "plan": {"op": "collect", "input": {
                "op": "hash_aggregate", "mode": "single", "group_by": [],
                "aggs": [{"fn": "sum", "as": "s",
                          "expr": {"col": "c_custkey"}},
                         {"fn": "count", "as": "c"}],
                "input": join}}}


class Lib:
    """One loaded copy of the library with the two tables registered."""

    def __init__(self, path, tables):
        if path is None:
            self.L = gpu.load_library()
        else:
            self.L = ctypes.CDLL(path)
            for name, sig in gpu._SIGNATURES.items():
                fn = getattr(self.L, name, None)
                if fn is not None:   # the parent lacks this change's entries
                    fn.restype = gpu._CODES[sig[0]]
                    fn.argtypes = [gpu._CODES[c] for c in sig[2:]]
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
                ctypes.c_int64(cols[0][1].shape[0])) == 0

    def run(self, doc):
        """-> (seconds, [sum, count]); the call returns its result rows, so
        the device work has finished when it does."""
        out = ctypes.c_char_p()
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        t0 = time.perf_counter()
        rc = self.L.bg_execute_stage(json.dumps(doc).encode(),
                                     ctypes.byref(out))
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        if rc != 0:
            raise RuntimeError(self.L.bg_last_error().decode())
        row = json.loads(out.value.decode())["rows"][0]
        return dt, [int(row[0]), int(row[1])]


def spread(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs),
            "max_s": max(xs), "runs_s": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's "
                    "libballista_gpu.so, for the alternated inner-join run")
    ap.add_argument("--out", default=os.path.join(
        ROOT, "bench_outputs", "perf_join_build_side.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    c_custkey = torch.arange(1, N_BUILD + 1, device=dev, dtype=torch.int64)
    # buyers are the custkeys that are no multiple of 3, as in dbgen
    r = torch.randint(0, N_BUILD // 3 * 2, (N_PROBE,), generator=g,
                      device=dev, dtype=torch.int64)
    o_custkey = r + r // 2 + 1
    o_orderkey = torch.arange(N_PROBE, device=dev, dtype=torch.int64) * 4 + 1
    del r
    torch.cuda.synchronize()
    tables = {"customer": [("c_custkey", c_custkey)],
              "orders": [("o_orderkey", o_orderkey),
                         ("o_custkey", o_custkey)]}
    new = Lib(None, tables)
    rec = {"build_rows": N_BUILD, "probe_rows": N_PROBE, "repeats": REPEATS,
           "timing": "host clock around bg_execute_stage (returns rows, so "
                     "device work is complete); 1 warm-up run per plan",
           "source_hash": new.hash, "plans": {}}

    for jt_new, jt_old in (("semi_build", "semi"), ("outer_build", "left")):
        docs = {jt_new: plan(jt_new, False),
                "swapped_" + jt_old: plan(jt_old, True)}
        results = {}
        for name, doc in docs.items():
            _, results[name] = new.run(doc)         # warm-up
        times = {name: [] for name in docs}
        for _ in range(REPEATS):                    # alternated
            for name, doc in docs.items():
                dt, res = new.run(doc)
                assert res == results[name]
                times[name].append(dt)
        a, b = results[jt_new], results["swapped_" + jt_old]
        assert a == b, f"{jt_new} {a} != swapped {jt_old} {b}"
        for name in docs:
            rec["plans"][name] = dict(spread(times[name]),
                                      sum_custkey=results[name][0],
                                      rows=results[name][1])
        print(json.dumps({k: rec["plans"][k]["median_s"] for k in docs}),
              flush=True)

    # the untouched path: inner, this library against the parent's
    libs = {"new": new}
    if args.parent_lib:
        libs["parent"] = Lib(os.path.abspath(args.parent_lib), tables)
        rec["parent_source_hash"] = libs["parent"].hash
        assert libs["parent"].hash != new.hash
    doc = plan("inner", False)
    results = {k: lib.run(doc)[1] for k, lib in libs.items()}   # warm-up
    assert len({tuple(v) for v in results.values()}) == 1, results
    times = {k: [] for k in libs}
    for _ in range(2 * REPEATS):
        for k, lib in libs.items():
            dt, res = lib.run(doc)
            assert res == results[k]
            times[k].append(dt)
    rec["inner"] = {k: dict(spread(v), rows=results[k][1])
                    for k, v in times.items()}
    if "parent" in times:
        rec["inner"]["new_minus_parent_median_s"] = (
            statistics.median(times["new"])
            - statistics.median(times["parent"]))
        rec["inner"]["parent_run_to_run_spread_s"] = (
            max(times["parent"]) - min(times["parent"]))
    else:
        rec["inner"]["parent"] = "not measured (no --parent-lib)"
    print(json.dumps(rec["inner"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
