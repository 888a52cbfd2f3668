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
With --parent-lib every plan and every phase of the breakdown also runs on
the parent commit's library, alternated run by run with this tree's, and is
recorded under "parent" next to it: the check that a change to the probe
kernels left their speed where it was.
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
    """One loaded copy of the library with the two tables registered."""

    def __init__(self, path, tables):
        if path is None:
            self.L = gpu.load_library()
        else:
            self.L = ctypes.CDLL(path)
            for name, sig in gpu._SIGNATURES.items():
                fn = getattr(self.L, name, None)
                if fn is not None:   # the parent may lack newer entries
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


def abi_breakdown(libs, repeats, c_custkey, c_x, o_custkey, o_x):
    """Count + fill of the inner join, seconds per phase (median of `repeats`
    after one warm-up), on the three probe paths; -> {library: {path: ...}},
    the libraries taking turns run by run."""
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

    def ok(L, rc):
        if rc != 0:
            raise RuntimeError(L.bg_last_error().decode())

    def timed(L, call):
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        ok(L, L.bg_synchronize())
        t0 = time.perf_counter()
        ok(L, call())
        ok(L, L.bg_synchronize())
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        return dt

    op, ob = out_p.data_ptr(), out_b.data_ptr()

    def paths_of(L):
        fast, general = ctypes.c_void_p(), ctypes.c_void_p()
        ok(L, L.bg_hashjoin_build(bkey, c_custkey.shape[0],
                                  ctypes.byref(fast)))
        ok(L, L.bg_hashjoin_build2(bkey, 1, c_custkey.shape[0],
                                   ctypes.byref(general)))
        return fast, general, {
            "int64_fast_table": (
                lambda: L.bg_hashjoin_probe_count(fast, pkey, n,
                                                  ctypes.byref(m)),
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

    tables = {k: paths_of(lib.L) for k, lib in libs.items()}
    rec = {k: {} for k in libs}
    for name in next(iter(tables.values()))[2]:
        tc, tf = {k: [] for k in libs}, {k: [] for k in libs}
        pairs = {}
        for i in range(repeats + 1):
            turn = list(libs.items())        # alternated, first one too
            for k, lib in turn[::-1] if i % 2 else turn:
                count, fill = tables[k][2][name]
                c = timed(lib.L, count)
                assert 0 < m.value <= n      # the pair buffers hold n pairs
                pairs[k] = m.value
                f = timed(lib.L, fill)
                if i:                        # run 0 warms up
                    tc[k].append(c)
                    tf[k].append(f)
        assert len(set(pairs.values())) == 1, pairs
        for k in libs:
            rec[k][name] = {"pairs": pairs[k], "count": spread(tc[k]),
                            "fill": spread(tf[k])}
    for k, lib in libs.items():
        ok(lib.L, lib.L.bg_hashjoin_free(tables[k][0]))
        ok(lib.L, lib.L.bg_hashjoin_free2(tables[k][1]))
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
    ap.add_argument("--parent-lib", help="the parent commit's "
                    "libballista_gpu.so: every plan and phase also runs on "
                    "it, alternated with this tree's library")
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    repeats = args.repeats
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
    libs = {"new": Lib(None, tables)}
    rec = {"build_rows": nb, "probe_rows": npr, "repeats": repeats,
           "timing": "host clock around bg_execute_stage (returns rows, so "
                     "device work is complete); 1 warm-up run per plan; the "
                     "plans of a pair, and the libraries, alternate",
           "source_hash": libs["new"].hash, "pairs": {}}
    if args.parent_lib:
        libs["parent"] = Lib(os.path.abspath(args.parent_lib), tables)
        rec["parent_source_hash"] = libs["parent"].hash
        assert libs["parent"].hash != libs["new"].hash
    for pair, docs in PAIRS.items():
        results = {(k, name): lib.run(d)[1] for name, d in docs.items()
                   for k, lib in libs.items()}          # warm-up
        times = {key: [] for key in results}
        for r in range(repeats):                        # alternated
            # the library that goes first changes every round: whichever
            # runs a plan second finds the plan's tables in the cache
            turn = list(libs.items())[::-1 if r % 2 else 1]
            for name, d in docs.items():
                for k, lib in turn:
                    dt, res = lib.run(d)
                    assert res == results[k, name]
                    times[k, name].append(dt)
        assert len({tuple(v) for v in results.values()}) == 1, results
        by_lib = {k: {name: dict(spread(times[k, name]),
                                 sum_custkey=results[k, name][0],
                                 rows=results[k, name][1]) for name in docs}
                  for k in libs}
        out = by_lib["new"]
        new, old = (out[n] for n in docs)
        out["first_minus_second_median_s"] = new["median_s"] - old["median_s"]
        out["second_min_max_spread_s"] = old["max_s"] - old["min_s"]
        if pair == "inner_ne":
            out["within_bar"] = (out["first_minus_second_median_s"]
                                 <= out["second_min_max_spread_s"])
        if "parent" in by_lib:
            out["parent"] = by_lib["parent"]
        rec["pairs"][pair] = out
        print(json.dumps({pair: {
            k: {name: v["median_s"] for name, v in by_lib[k].items()
                if name in docs} for k in libs}}), flush=True)
    abi = abi_breakdown(libs, repeats, c_custkey, c_x, o_custkey, o_x)
    rec["abi_breakdown"] = abi["new"]
    if "parent" in abi:
        rec["abi_breakdown_parent"] = abi["parent"]
    print(json.dumps({"abi_breakdown": {
        lib: {k: {"pairs": v["pairs"],
                  "count_median_s": v["count"]["median_s"],
                  "fill_median_s": v["fill"]["median_s"]}
              for k, v in paths.items()} for lib, paths in abi.items()}}),
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
