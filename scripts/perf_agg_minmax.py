#!/usr/bin/env python3
"""MIN/MAX over Decimal128 / Utf8 (the row-index accumulators) at the C ABI,
and what the new switch cases cost the aggregate ops that were there before.

minmax     three shapes, each timed for
             min_row_dec128  MIN_ROW over Decimal128 values that fit an i64
             min_i64         MIN_I64 over the same values as Int64 (the op
                             that existed before: the baseline of the ratio)
             min_row_utf8    MIN_ROW over Utf8 strings of 25 bytes
             a (q2-like)       8 M rows, 2 M groups (global table; the LDS
                               attempt overflows first and is part of the time)
             b (q1-like, LDS) 64 M rows, 50 groups
             c (q15-like)      8 M rows, 1 group
           The MIN_ROW winners are checked against the MIN_I64 values on
           the device before anything is timed.
existing   (with --baseline-lib: the library built from the parent commit)
           two shapes of ops this work does not touch, SUM_DEC128 over
           32 M rows / 3 M groups (global table) and a q1-shaped record
           (4 x SUM_DEC128 + SUM_I64, 64 M rows, 6 groups, LDS tables),
           each library in fresh processes of its own, the two alternated
           ROUNDS times.  "within_parent_spread": the branch's median is not
           above the slowest of the parent's own repeats.

Every figure is bg_last_kernel_ms (device events around the aggregate
kernels) as median and min..max of REPEATS runs after one warm-up; the host
clock around the call is recorded beside it.  Each child process runs under
its own time limit and the first failure ends the script."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 7
ROUNDS = 3
CHILD_LIMIT_S = 240

SHAPES = {"a_q2_like": (8_000_000, 2_000_000),
          "b_q1_like_lds": (64_000_000, 50),
          "c_q15_like": (8_000_000, 1)}
STR_BYTES = 25


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs),
            "max_ms": max(xs), "runs_ms": xs}


class Agg:
    """bg_hashagg over torch tensors with reusable output buffers."""

    def __init__(self, gpu, torch, max_groups, naggs):
        self.gpu, self.L = gpu, gpu.load_library()
        assert self.L.bg_init(0) == 0
        dev = torch.device("cuda:0")
        self.cap = max_groups
        self.first = torch.empty(max_groups, dtype=torch.int32, device=dev)
        self.acc = torch.empty((max_groups, naggs, 2), dtype=torch.int64,
                               device=dev)
        self.counts = torch.empty(max_groups, dtype=torch.int64, device=dev)
        self.ng = ctypes.c_int64()

    def col(self, t, dtype, offsets=None):
        n = offsets.shape[0] - 1 if offsets is not None else t.shape[0]
        return self.gpu.BgColumn(
            dtype, 0, 0, 0, ctypes.c_void_p(t.data_ptr()), None,
            ctypes.c_void_p(offsets.data_ptr()) if offsets is not None
            else None, n)

    def run(self, key, cols, ops, n):
        """-> (kernel ms, host ms)"""
        karr = (self.gpu.BgColumn * 1)(key)
        aarr = (self.gpu.BgColumn * len(cols))(*cols)
        oarr = (ctypes.c_int32 * len(ops))(*ops)
        t0 = time.perf_counter()
        rc = self.L.bg_hashagg(karr, 1, aarr, oarr, len(ops), None, n,
                               self.cap, self.first.data_ptr(),
                               self.acc.data_ptr(), self.counts.data_ptr(),
                               ctypes.byref(self.ng))
        host = (time.perf_counter() - t0) * 1e3
        if rc != 0:
            raise RuntimeError(self.L.bg_last_error().decode())
        return self.L.bg_last_kernel_ms(), host

    def timed(self, key, cols, ops, n):
        self.run(key, cols, ops, n)  # warm-up
        runs = [self.run(key, cols, ops, n) for _ in range(REPEATS)]
        return dict(spread([k for k, _ in runs]),
                    host_median_ms=statistics.median(h for _, h in runs),
                    ngroups=self.ng.value)


def load(lib):
    import torch
    from datafusion_ballista_amd import gpu
    if lib:
        # a library built from another commit: declare what it exports
        probe = ctypes.CDLL(lib)
        for name in list(gpu._SIGNATURES):
            if not hasattr(probe, name):
                del gpu._SIGNATURES[name]
        gpu.lib_path = lambda: lib
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    return gpu, torch


def child_minmax(args):
    gpu, torch = load(args.lib)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(41)
    out = {}
    for name, (n, groups) in SHAPES.items():
        n = max(int(n * args.scale), 1 << 17)
        groups = max(int(groups * args.scale), 1) if groups > 50 else groups
        agg = Agg(gpu, torch, max(2 * groups, 64), 1)
        keys = torch.randint(0, groups, (n,), generator=g, device=dev,
                             dtype=torch.int64)
        v = torch.randint(-10**15, 10**15, (n,), generator=g, device=dev,
                          dtype=torch.int64)
        dec = torch.stack([v, v >> 63], dim=1).contiguous()  # sign-extended
        sdata = torch.randint(97, 123, (n * STR_BYTES,), generator=g,
                              device=dev, dtype=torch.uint8)
        soffs = (torch.arange(n + 1, device=dev, dtype=torch.int64)
                 * STR_BYTES).to(torch.int32)
        torch.cuda.synchronize()
        kc = agg.col(keys, gpu.BG_DT_INT64)
        cases = {
            "min_row_dec128": (agg.col(dec, gpu.BG_DT_DECIMAL128),
                               gpu.BG_AGG_OP_MIN_ROW),
            "min_i64": (agg.col(v, gpu.BG_DT_INT64), gpu.BG_AGG_OP_MIN_I64),
            "min_row_utf8": (agg.col(sdata, gpu.BG_DT_UTF8, soffs),
                             gpu.BG_AGG_OP_MIN_ROW),
        }
        # the winners' values must equal the MIN_I64 values, group by
        # group (ordered by key: slot order can differ between two runs)
        agg.run(kc, [cases["min_row_dec128"][0]], [gpu.BG_AGG_OP_MIN_ROW], n)
        ng = agg.ng.value
        rows = agg.acc[:ng, 0, 0].clone() - 1
        assert bool((rows >= 0).all())
        by_key = torch.argsort(keys[agg.first[:ng].long()])
        got = v[rows][by_key]
        agg.run(kc, [cases["min_i64"][0]], [gpu.BG_AGG_OP_MIN_I64], n)
        assert ng == agg.ng.value
        by_key = torch.argsort(keys[agg.first[:ng].long()])
        want = (~agg.acc[:ng, 0, 0] ^ torch.iinfo(torch.int64).min)[by_key]
        assert bool((got == want).all()), name
        rec = {"rows": n, "groups": ng}
        for cname, (c, op) in cases.items():
            rec[cname] = agg.timed(kc, [c], [op], n)
        rec["dec128_over_i64"] = (rec["min_row_dec128"]["median_ms"] /
                                  rec["min_i64"]["median_ms"])
        rec["utf8_over_i64"] = (rec["min_row_utf8"]["median_ms"] /
                                rec["min_i64"]["median_ms"])
        out[name] = rec
        del keys, v, dec, sdata, soffs, agg
    print("RESULT " + json.dumps(out), flush=True)


def child_existing(args):
    gpu, torch = load(args.lib)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(43)
    out = {}
    n = max(int(32_000_000 * args.scale), 1 << 17)
    groups = max(int(3_000_000 * args.scale), 64)
    agg = Agg(gpu, torch, groups + groups // 8, 1)
    keys = torch.randint(0, groups, (n,), generator=g, device=dev,
                         dtype=torch.int64)
    dec = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    dec[:, 0] = torch.randint(0, 10**9, (n,), generator=g, device=dev)
    torch.cuda.synchronize()
    out["sum_dec128_32M_rows_3M_groups"] = agg.timed(
        agg.col(keys, gpu.BG_DT_INT64), [agg.col(dec, gpu.BG_DT_DECIMAL128)],
        [gpu.BG_AGG_OP_SUM_DEC128], n)
    del keys, dec, agg

    n = max(int(64_000_000 * args.scale), 1 << 17)
    agg = Agg(gpu, torch, 64, 5)
    keys = torch.randint(0, 6, (n,), generator=g, device=dev,
                         dtype=torch.int64)
    dec = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    dec[:, 0] = torch.randint(0, 10**7, (n,), generator=g, device=dev)
    qty = torch.randint(0, 50, (n,), generator=g, device=dev,
                        dtype=torch.int64)
    torch.cuda.synchronize()
    dc = agg.col(dec, gpu.BG_DT_DECIMAL128)
    out["q1_record_64M_rows_6_groups_lds"] = agg.timed(
        agg.col(keys, gpu.BG_DT_INT64),
        [dc, dc, dc, dc, agg.col(qty, gpu.BG_DT_INT64)],
        [gpu.BG_AGG_OP_SUM_DEC128] * 4 + [gpu.BG_AGG_OP_SUM_I64], n)
    out["source_hash"] = agg.L.bg_source_hash().decode()
    print("RESULT " + json.dumps(out), flush=True)


def spawn(mode, lib, scale):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode,
           "--scale", str(scale)]
    if lib:
        cmd += ["--lib", lib]
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
        ROOT, "profiles", "perf_agg_minmax.json"))
    ap.add_argument("--baseline-lib", help="libballista_gpu.so built from "
                    "the parent commit, for the existing-ops comparison")
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrink every shape (rehearsal only)")
    ap.add_argument("--child", choices=["minmax", "existing"])
    ap.add_argument("--lib")
    args = ap.parse_args()
    if args.child:
        return {"minmax": child_minmax,
                "existing": child_existing}[args.child](args)

    rec = {"repeats": REPEATS, "string_bytes": STR_BYTES,
           "timing": "bg_last_kernel_ms (device events around the aggregate "
                     "kernels, a failed LDS attempt included); 1 warm-up; "
                     "median and min..max of the repeats",
           "scale": args.scale}
    rec["minmax"] = spawn("minmax", None, args.scale)
    print(json.dumps({k: {"dec128_over_i64": v["dec128_over_i64"],
                          "utf8_over_i64": v["utf8_over_i64"],
                          "min_i64_ms": v["min_i64"]["median_ms"]}
                      for k, v in rec["minmax"].items()}), flush=True)
    if args.baseline_lib:
        base = os.path.abspath(args.baseline_lib)
        runs = {"parent": [], "branch": []}
        for _ in range(ROUNDS):  # alternated, a fresh process each
            runs["parent"].append(spawn("existing", base, args.scale))
            runs["branch"].append(spawn("existing", None, args.scale))
        ab = {"rounds": ROUNDS,
              "parent_source_hash": runs["parent"][0]["source_hash"],
              "branch_source_hash": runs["branch"][0]["source_hash"]}
        for shape in (k for k in runs["parent"][0] if k != "source_hash"):
            p = [x for r in runs["parent"] for x in r[shape]["runs_ms"]]
            b = [x for r in runs["branch"] for x in r[shape]["runs_ms"]]
            ab[shape] = {"parent": spread(p), "branch": spread(b),
                         "branch_over_parent_median":
                             statistics.median(b) / statistics.median(p),
                         "within_parent_spread":
                             statistics.median(b) <= max(p)}
            print(json.dumps({shape: {k: v if not isinstance(v, dict)
                                      else v["median_ms"]
                                      for k, v in ab[shape].items()}}),
                  flush=True)
        rec["existing_ops"] = ab
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
