#!/usr/bin/env python3
"""The cast / Float64 / decimal-division kernels at lineitem's SF100-class
size (150 M rows, seeded device-generated inputs), alternated launch by
launch in this one process.

  hot cast   bg_cast Decimal128(15,2) -> (30,15), q17's filter operand:
             16 B in, 16 B out per row.  Declared as (15,2) the source
             cannot overflow and the call launches the plain kernel;
             declared as (38,2) the same values take the checked kernel
             (validity walk, ballot, failure counter read back).
    yardstick  bg_project_dec128 op 4 (a * lit) with lit = 10^13 on the
               same column: the same traffic and the same product
  recorded   Decimal128 -> Float64 (24 B/row), bg_project_f64 a * b
             (24 B/row), bg_div_dec128 (48 B/row)

Every sample is one call between two device events on the library's stream
(the null stream, torch's default), after WARMUP untimed calls, so a
checked call's sample includes its 8-byte counter read-back.  Results are
checked at the measured size: the cast against the yardstick's output bit
for bit, the others on a leading slice against Python ints and floats.
Each timed step runs under its own time limit: a watchdog ends the process
if one overruns."""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from datafusion_ballista_amd import gpu  # noqa: E402

N_ROWS = 150_000_000
REPEATS = 15
WARMUP = 3
STEP_LIMIT_S = 120
HBM_SPEC_TB_S = 8.0        # MI355X HBM3E, datasheet
HBM_COPY_TB_S = 6.29       # measured float4 copy on the same part
CHECK_ROWS = 4096


def ok(rc, L, what):
    if rc != 0:
        raise RuntimeError(f"{what}: rc={rc} {L.bg_last_error().decode()}")


def timed(call):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    faulthandler.cancel_dump_traceback_later()
    return e0.elapsed_time(e1)


def alternate(series):
    """series: {name: call} -> {name: [ms...]}, one sample of each per round
    so that drift hits every series alike."""
    for call in series.values():
        for _ in range(WARMUP):
            timed(call)
    runs = {k: [] for k in series}
    for _ in range(REPEATS):
        for k, call in series.items():
            runs[k].append(timed(call))
    return runs


def summary(ms, rows, bytes_per_row):
    med = statistics.median(ms)
    tb_s = rows * bytes_per_row / (med * 1e-3) / 1e12
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms),
            "relative_spread": (max(ms) - min(ms)) / med, "runs_ms": ms,
            "model_bytes_per_row": bytes_per_row,
            "model_GB_per_s": tb_s * 1e3,
            "share_of_hbm_spec_8_0_TB_s": tb_s / HBM_SPEC_TB_S,
            "share_of_measured_copy_6_29_TB_s": tb_s / HBM_COPY_TB_S}


def dec128_from_i64(v):
    """int64[n] -> int64[n, 2]: little-endian (lo, sign-extended hi)."""
    out = torch.empty((v.numel(), 2), device=v.device, dtype=torch.int64)
    out[:, 0] = v
    out[:, 1] = v >> 63
    return out


def dec_col(t, n, p, s):
    return gpu.BgColumn(gpu.BG_DT_DECIMAL128, p, s, 0,
                        ctypes.c_void_p(t.data_ptr()), None, None, n)


def head_ints(t, k):
    """first k Decimal128 rows of an int64[n, 2] tensor as Python ints."""
    return [(lo & 0xFFFFFFFFFFFFFFFF) | (hi << 64)
            for lo, hi in t[:k].cpu().tolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "perf_cast_exprs.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    n = args.rows
    k = min(CHECK_ROWS, n)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    L = gpu.load_library()
    ok(L.bg_init(0), L, "bg_init")
    rec = {"rows": n, "repeats": REPEATS, "warmup": WARMUP,
           "timing": "device events around one call, null stream; series "
                     "alternated; a checked call includes its counter "
                     "read-back",
           "device": torch.cuda.get_device_name(0),
           "source_hash": L.bg_source_hash().decode(), "kernels": {}}
    kern = rec["kernels"]

    # ---- the hot cast against bg_project_dec128 op 4 ----
    qty_i = torch.randint(100, 5100, (n,), generator=g, device=dev,
                          dtype=torch.int64)
    qty = dec128_from_i64(qty_i)
    out_a = torch.empty((n, 2), device=dev, dtype=torch.int64)
    out_b = torch.empty((n, 2), device=dev, dtype=torch.int64)
    tight, loose = dec_col(qty, n, 15, 2), dec_col(qty, n, 38, 2)
    pa_, pb_ = (ctypes.c_void_p(out_a.data_ptr()),
                ctypes.c_void_p(out_b.data_ptr()))
    failed = ctypes.c_int64()

    def cast_plain():
        ok(L.bg_cast(ctypes.byref(tight), gpu.BG_DT_DECIMAL128, 30, 15, n,
                     pa_, None), L, "bg_cast")

    def cast_checked():
        ok(L.bg_cast(ctypes.byref(loose), gpu.BG_DT_DECIMAL128, 30, 15, n,
                     pa_, ctypes.byref(failed)), L, "bg_cast")

    def op4():
        ok(L.bg_project_dec128(gpu.BG_PROJ_MUL_LIT, ctypes.byref(tight), None,
                               10**13, 0, n, pb_), L, "bg_project_dec128")

    op4()
    for call in (cast_plain, cast_checked):
        out_a.zero_()
        call()
        assert torch.equal(out_a, out_b), "cast differs from a * 10^13"
    assert head_ints(out_a, k) == [v * 10**13
                                   for v in qty_i[:k].cpu().tolist()]
    runs = alternate({"cast_dec15_2_to_30_15_checked": cast_checked,
                      "yardstick_project_dec128_mul_lit": op4,
                      "cast_dec15_2_to_30_15_unchecked": cast_plain})
    for name, ms in runs.items():
        kern[name] = summary(ms, n, 32)
    yard = kern["yardstick_project_dec128_mul_lit"]
    allowed = 1.0 + 2.0 * yard["relative_spread"]
    rec["hot_cast_vs_yardstick"] = {
        "allowed_ratio": allowed,
        "allowed_is": "1 + 2 * yardstick (max-min)/median, this session",
        "checked_ratio_of_medians":
            kern["cast_dec15_2_to_30_15_checked"]["median_ms"]
            / yard["median_ms"],
        "unchecked_ratio_of_medians":
            kern["cast_dec15_2_to_30_15_unchecked"]["median_ms"]
            / yard["median_ms"]}
    h = rec["hot_cast_vs_yardstick"]
    h["checked_within_margin"] = h["checked_ratio_of_medians"] <= allowed
    h["unchecked_within_margin"] = h["unchecked_ratio_of_medians"] <= allowed
    print(json.dumps(h), flush=True)
    del out_b

    # ---- Decimal128 -> Float64, Float64 a * b, Decimal128 a / b ----
    f_a = torch.empty(n, device=dev, dtype=torch.float64)
    pf_a = ctypes.c_void_p(f_a.data_ptr())

    def to_f64():
        ok(L.bg_cast(ctypes.byref(tight), gpu.BG_DT_FLOAT64, 0, 0, n, pf_a,
                     None), L, "bg_cast")

    to_f64()
    assert f_a[:k].cpu().tolist() == [float(v) / 100.0
                                      for v in qty_i[:k].cpu().tolist()]
    f_b = torch.rand(n, generator=g, device=dev, dtype=torch.float64) + 0.5
    f_o = torch.empty(n, device=dev, dtype=torch.float64)
    ca = gpu.BgColumn(gpu.BG_DT_FLOAT64, 0, 0, 0, pf_a, None, None, n)
    cb = gpu.BgColumn(gpu.BG_DT_FLOAT64, 0, 0, 0,
                      ctypes.c_void_p(f_b.data_ptr()), None, None, n)
    pf_o = ctypes.c_void_p(f_o.data_ptr())

    def f64_mul():
        ok(L.bg_project_f64(gpu.BG_F64_MUL, ctypes.byref(ca),
                            ctypes.byref(cb), 0.0, n, pf_o), L,
           "bg_project_f64")

    f64_mul()
    assert f_o[:k].cpu().tolist() == [x * y for x, y in zip(
        f_a[:k].cpu().tolist(), f_b[:k].cpu().tolist())]
    runs = alternate({"cast_dec128_to_f64": to_f64,
                      "project_f64_mul": f64_mul})
    kern["cast_dec128_to_f64"] = summary(runs["cast_dec128_to_f64"], n, 24)
    kern["project_f64_mul"] = summary(runs["project_f64_mul"], n, 24)
    del f_a, f_b, f_o

    den_i = torch.randint(1, 10**9, (n,), generator=g, device=dev,
                          dtype=torch.int64)
    den = dec128_from_i64(den_i)
    num_c, den_c = dec_col(qty, n, 38, 4), dec_col(den, n, 38, 4)

    def div():
        ok(L.bg_div_dec128(ctypes.byref(num_c), ctypes.byref(den_c), 4, n,
                           pa_, ctypes.byref(failed)), L, "bg_div_dec128")

    div()
    assert head_ints(out_a, k) == [
        a * 10**4 // b for a, b in zip(qty_i[:k].cpu().tolist(),
                                       den_i[:k].cpu().tolist())]
    runs = alternate({"div_dec128_mul_pow_4": div})
    d = summary(runs["div_dec128_mul_pow_4"], n, 48)
    stream = kern["project_f64_mul"]["model_GB_per_s"]
    d["bound"] = ("ALU (the 128-bit divide): under half the byte rate the "
                  "streaming kernels reach"
                  if d["model_GB_per_s"] < 0.5 * stream else
                  "memory: within 2x of the streaming kernels' byte rate")
    kern["div_dec128_mul_pow_4"] = d
    print(json.dumps({name: [round(v["median_ms"], 4),
                             round(v["model_GB_per_s"], 1)]
                      for name, v in kern.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
