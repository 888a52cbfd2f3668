#!/usr/bin/env python3
"""What the window pass costs next to the sort it follows, and q53's shape
against the only way the parent commit can compute the same column.

  rows       150 M: Int64 partition key (150 rows per partition, 1 M
             partitions), Int64 order key (peer groups of two), a
             Decimal128(15,2) value; already sorted for the C-ABI figures
  abi        1  bg_window_bounds + bg_window_rank(RANK)
             2  bounds + frame + running SUM over Decimal128
                (rows unbounded preceding .. current row)
             3  bounds + frame + whole-partition AVG (SUM, COUNT,
                bg_avg_finalize)
             next to them bg_sort_rows2 over the same two keys, shuffled, in
             the same process; each with the bytes the kernels must move
             under the DESIGN section 7 model and the rate that implies as a
             share of the measured copy rate
  stages     4  q53's shape through bg_execute_stage on one registered,
                unsorted table: sort + window(avg over the whole partition)
                against hash_aggregate(avg per key) + inner hash_join back
                onto the rows; both keep every row and return one (collect
                limit 1)

Nothing here is a gate: the figures are recorded and the faster side named.
Every sample sits between two device events on the library's stream (the
null stream), after one untimed call; medians of REPEATS samples per
process.  Every child is a fresh process under a time limit; the two stage
plans alternate, ROUNDS times."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ROWS = 150_000_000
PART_ROWS = 150
REPEATS = 7
ROUNDS = 2
CHILD_LIMIT_S = 500
HBM_COPY_TB_S = 6.29       # measured float4 copy on the same part (DESIGN)

# Bytes per row the kernels must move.  Bitmaps, the
# n/64-entry carry arrays and the per-span carries are under 1 % and left
# out; a prefix read that every row of a partition shares counts once per
# partition, i.e. not at all at 150 rows per partition.
MODEL = {
    # heads read both keys once; each of the two fills writes start + end
    "bounds": 8 + 8 + 2 * (4 + 4),
    # reads part_start + peer_start, writes the i64 rank
    "rank": 4 + 4 + 8,
    # ROWS frame: reads part_start + part_end, writes lo + hi
    "frame": 4 + 4 + 4 + 4,
    # Decimal128 SUM: the value is read by the span-total pass and by the
    # rescan, which writes the 16 B prefix; the per-row pass reads
    # part_start, hi and writes value + validity
    "sum_dec_scan": 16 + 16 + 16,
    "sum_dec_rows": 4 + 4 + 16,
    # running frames read the prefix at hi - 1 and at the partition start
    "sum_dec_running_reads": 16,
    # COUNT over a column without NULLs is hi - lo: no prefix
    "count_rows": 4 + 4 + 8,
    # bg_avg_finalize: sum + count in, value + validity out
    "avg_finalize": 16 + 8 + 16,
}


def model_bytes(which, n):
    m = MODEL
    per_row = {
        "bounds_rank": m["bounds"] + m["rank"],
        "bounds_running_sum": m["bounds"] + m["frame"] + m["sum_dec_scan"] +
        m["sum_dec_rows"] + m["sum_dec_running_reads"],
        "bounds_partition_avg": m["bounds"] + m["frame"] + m["sum_dec_scan"] +
        m["sum_dec_rows"] + m["count_rows"] + m["avg_finalize"],
    }[which]
    return per_row * n


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs),
            "max_ms": max(xs), "runs_ms": xs}


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def make_data(torch, n):
    """Seeded.  part/order are sorted; perm is the shuffle the stages and the
    sort see."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(5301)
    row = torch.arange(n, device=dev, dtype=torch.int64)
    part = row // PART_ROWS
    order = (row % PART_ROWS) // 2
    x = torch.randint(-99_999_99, 99_999_99, (n,), generator=g, device=dev,
                      dtype=torch.int64)
    dec = torch.empty((n, 2), device=dev, dtype=torch.int64)
    dec[:, 0] = x
    dec[:, 1] = x >> 63
    perm = torch.randperm(n, generator=g, device=dev)
    return {"part": part, "order": order, "dec": dec, "perm": perm}


def timed(torch, fn):
    fn()                                        # the untimed call
    torch.cuda.synchronize()
    runs = []
    for _ in range(REPEATS):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1))
    return spread(runs)


def child_abi(args, gpu, torch, L):
    n = args.rows
    d = make_data(torch, n)
    dev = torch.device("cuda:0")

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: rc={rc} {L.bg_last_error().decode()}")

    def col(dtype, t, p=0, s=0):
        return gpu.BgColumn(dtype, p, s, 0, ptr(t), None, None, n)

    pk = (gpu.BgColumn * 1)(col(gpu.BG_DT_INT64, d["part"]))
    okc = (gpu.BgColumn * 1)(col(gpu.BG_DT_INT64, d["order"]))
    val = col(gpu.BG_DT_DECIMAL128, d["dec"], 15, 2)
    u32 = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(6)]
    ps, pe, qs, qe, lo, hi = u32
    i64 = torch.empty(n, device=dev, dtype=torch.int64)
    d16 = torch.empty((n, 2), device=dev, dtype=torch.int64)
    avg = torch.empty((n, 2), device=dev, dtype=torch.int64)
    vbits = torch.empty((n + 63) // 64 * 8 + 8, device=dev, dtype=torch.uint8)

    def bounds():
        ok(L.bg_window_bounds(pk, 1, okc, 1, n, ptr(ps), ptr(pe), ptr(qs),
                              ptr(qe)), "bg_window_bounds")

    def frame(end_kind):
        ok(L.bg_window_frame(gpu.BG_WIN_ROWS, gpu.BG_WIN_UNBOUNDED, 0,
                             end_kind, 0, None, 0, ptr(ps), ptr(pe), ptr(qs),
                             ptr(qe), n, ptr(lo), ptr(hi)), "bg_window_frame")

    def agg(fn, out, valid):
        ok(L.bg_window_agg(fn, ctypes.byref(val), ptr(ps), None, ptr(hi), n,
                           ptr(out), valid), "bg_window_agg")

    def bounds_rank():
        bounds()
        ok(L.bg_window_rank(gpu.BG_WIN_RANK, ptr(ps), ptr(qs), n, ptr(i64)),
           "bg_window_rank")

    def bounds_running_sum():
        bounds()
        frame(gpu.BG_WIN_CURRENT_ROW)
        agg(gpu.BG_WIN_SUM, d16, ptr(vbits))

    def bounds_partition_avg():
        bounds()
        frame(gpu.BG_WIN_UNBOUNDED)
        agg(gpu.BG_WIN_SUM, d16, ptr(vbits))
        agg(gpu.BG_WIN_COUNT, i64, None)
        ok(L.bg_memset(ptr(vbits), 0xFF, vbits.numel()), "bg_memset")
        ok(L.bg_avg_finalize(ptr(d16), 16, 0, ptr(i64), 8, 4, n, ptr(avg),
                             ptr(vbits)), "bg_avg_finalize")

    out = {}
    for name, fn in (("bounds_rank", bounds_rank),
                     ("bounds_running_sum", bounds_running_sum),
                     ("bounds_partition_avg", bounds_partition_avg)):
        s = timed(torch, fn)
        mb = model_bytes(name, n)
        s["model_bytes"] = mb
        s["model_GB_per_s"] = mb / (s["median_ms"] * 1e-3) / 1e9
        s["share_of_measured_copy_6_29_TB_s"] = \
            mb / (s["median_ms"] * 1e-3) / 1e12 / HBM_COPY_TB_S
        out[name] = s
    # spot values: rank and running sum of the last rows against torch
    bounds_rank()
    first = (n - 1) // PART_ROWS * PART_ROWS
    want_rank = (d["order"][first:] * 2 + 1)
    assert torch.equal(i64[first:], want_rank), "rank spot check"
    bounds_running_sum()
    torch.cuda.synchronize()
    want_sum = torch.cumsum(d["dec"][first:, 0], 0)
    assert torch.equal(d16[first:, 0], want_sum), "running sum spot check"

    # the sort the window follows: the same two keys, shuffled
    sp = d["part"][d["perm"]].contiguous()
    so = d["order"][d["perm"]].contiguous()
    keys = (gpu.BgColumn * 2)(col(gpu.BG_DT_INT64, sp),
                              col(gpu.BG_DT_INT64, so))
    zeros = (ctypes.c_int32 * 2)(0, 0)
    perm_out = torch.empty(n, device=dev, dtype=torch.int32)

    def sort():
        ok(L.bg_sort_rows2(keys, zeros, zeros, 2, n, ptr(perm_out)),
           "bg_sort_rows2")
    out["sort_rows2_same_keys"] = timed(torch, sort)
    return out


def q53_plans(n_parts):
    scan = {"op": "scan",
            "schema": [{"name": "k", "dtype": "int64"},
                       {"name": "x", "dtype": "decimal128", "precision": 15,
                        "scale": 2}],
            "source": {"kind": "device", "table": "perf_window"}}
    whole = {"units": "rows", "start": "unbounded", "end": "unbounded"}
    window = {"op": "window", "partition_by": ["k"], "order_by": [],
              "exprs": [{"fn": "avg", "as": "a", "expr": {"col": "x"},
                         "frame": whole}],
              "input": {"op": "sort", "keys": [{"col": "k"}], "input": scan}}
    join = {"op": "hash_join", "join_type": "inner",
            "build": {"op": "hash_aggregate", "mode": "single",
                      "group_by": ["k"], "estimated_groups": n_parts,
                      "aggs": [{"fn": "avg", "as": "a",
                                "expr": {"col": "x"}}],
                      "input": scan},
            "probe": scan, "build_keys": ["k"], "probe_keys": ["k"],
            "output": [{"side": "probe", "col": "k"},
                       {"side": "probe", "col": "x"},
                       {"side": "build", "col": "a"}]}
    return {"window_stage": window, "hash_stage": join}


def child_stage(args, gpu, torch, L):
    n = args.rows
    d = make_data(torch, n)
    k = d["part"][d["perm"]].contiguous()
    x = d["dec"][d["perm"]].contiguous()
    cols = (gpu.BgColumn * 2)(
        gpu.BgColumn(gpu.BG_DT_INT64, 0, 0, 0, ptr(k), None, None, n),
        gpu.BgColumn(gpu.BG_DT_DECIMAL128, 15, 2, 0, ptr(x), None, None, n))
    names = (ctypes.c_char_p * 2)(b"k", b"x")
    assert L.bg_stage_register_table(b"perf_window", cols, names, 2, n) == 0
    del d
    plan = q53_plans((n + PART_ROWS - 1) // PART_ROWS)[args.child]
    doc = json.dumps({"job_id": "perf", "stage_id": 1, "task_id": 0,
                      "work_dir": "/tmp/perf_window",
                      "plan": {"op": "collect", "limit": 1,
                               "input": plan}}).encode()
    last = {}

    def run():
        out = ctypes.c_char_p()
        rc = L.bg_execute_stage(doc, ctypes.byref(out))
        if rc != 0:
            raise RuntimeError(f"stage rc={rc}: {L.bg_last_error().decode()}")
        last["res"] = json.loads(out.value.decode())
    s = timed(torch, run)
    s["schema"] = last["res"]["schema"]
    L.bg_stage_unregister_table(b"perf_window")
    return s


def child(args):
    import torch
    from datafusion_ballista_amd import gpu
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    L = gpu.load_library()
    assert L.bg_init(0) == 0
    fn = child_abi if args.child == "abi" else child_stage
    out = {"source_hash": L.bg_source_hash().decode(),
           "device": torch.cuda.get_device_name(0),
           "result": fn(args, gpu, torch, L)}
    print("RESULT " + json.dumps(out), flush=True)


def spawn(mode, rows):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode,
           "--rows", str(rows)]
    p = subprocess.run(cmd, capture_output=True, text=True,
                       timeout=CHILD_LIMIT_S)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{mode} child failed (rc={p.returncode}): stopping")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(line[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "perf_window.json"))
    ap.add_argument("--rows", type=int, default=N_ROWS,
                    help="rows (fewer: rehearsal only)")
    ap.add_argument("--child", choices=["abi", "window_stage", "hash_stage"])
    args = ap.parse_args()
    if args.child:
        return child(args)

    n = args.rows
    abi = spawn("abi", n)
    stages = {"window_stage": [], "hash_stage": []}
    for _ in range(ROUNDS):  # alternated, a fresh process each
        for mode in stages:
            stages[mode].append(spawn(mode, n))
    rec = {"rows": n, "rows_per_partition": PART_ROWS,
           "partitions": (n + PART_ROWS - 1) // PART_ROWS,
           "repeats_per_process": REPEATS, "stage_rounds": ROUNDS,
           "timing": "device events around the calls on the null stream, 1 "
                     "untimed call first, fresh process per child",
           "device": abi["device"], "source_hash": abi["source_hash"],
           "measured": "every *_ms field and what is derived from it",
           "modelled": "model_bytes (bytes per row: model_bytes_per_row)",
           "model_bytes_per_row": MODEL,
           "gated": False,
           "abi": abi["result"]}
    sort_ms = abi["result"]["sort_rows2_same_keys"]["median_ms"]
    for name in ("bounds_rank", "bounds_running_sum", "bounds_partition_avg"):
        s = rec["abi"][name]
        s["over_sort_median"] = s["median_ms"] / sort_ms
        s["costs_less_than_the_sort"] = s["median_ms"] < sort_ms
    q53 = {}
    for mode, rs in stages.items():
        q53[mode] = spread([x for r in rs for x in r["result"]["runs_ms"]])
        q53[mode]["schema"] = rs[0]["result"]["schema"]
    w, h = q53["window_stage"], q53["hash_stage"]
    q53["plans"] = {"window_stage": "sort(k) -> window(avg(x) over "
                                    "(partition by k))",
                    "hash_stage": "hash_aggregate(avg(x) by k) -> inner "
                                  "hash_join back onto the rows"}
    q53["window_over_hash_median"] = w["median_ms"] / h["median_ms"]
    q53["faster"] = "window_stage" if w["median_ms"] < h["median_ms"] \
        else "hash_stage"
    rec["q53_shape_stages"] = q53
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({
        "sort_ms": round(sort_ms, 3),
        **{k: round(rec["abi"][k]["median_ms"], 3)
           for k in ("bounds_rank", "bounds_running_sum",
                     "bounds_partition_avg")},
        "q53_window_ms": round(w["median_ms"], 3),
        "q53_hash_ms": round(h["median_ms"], 3),
        "q53_faster": q53["faster"]}), flush=True)


if __name__ == "__main__":
    main()
