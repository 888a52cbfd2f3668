#!/usr/bin/env python3
"""HBM-traffic calibration for k_q6_agg (run under rocprofv3 --pmc
FETCH_SIZE, in a run of its own — no tracing combined).

k_q6_agg is a short-circuit scan: dates are read for every row (4 B), and
each later column (discount, quantity, price; 16 B each) only where a row
of the line passed every earlier test.  The script launches it on cases
with analytically known byte counts, so the PMC FETCH_SIZE per dispatch can
be calibrated on this exact access pattern (MI355X_MICROARCH.md §HBM: gfx950
FETCH_SIZE reports 1/2 of wide coalesced reads — calibrate, don't assume):
  all_fail_date:   date window empty -> only the dates = 4 B/row
  all_pass:        full ranges       -> all four columns = 52 B/row
  every_other_line:      own date column, passes for rows (i/8)%2==0, other
     ranges wide open -> every second 128-B line of the three decimal
     columns = 4 + 48/2 = 28 B/row at either fetch granule; calibrates how
     FETCH_SIZE counts a holed stream
  every_other_half_line: passes for rows (i/4)%2==0 -> the first 64 B of
     every line: 52 B/row if HBM is fetched in 128-B granules, 28 B/row if
     in 64-B granules; measures the fetch granularity
  real_q6:         1994 window, the bench's predicate set -> 22.0 B/row
     modelled at 128-B granules, 14.9 B/row at 64-B (8M-row CPU model)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from datafusion_ballista_amd import gpu, tpch_synth  # noqa: E402

N = 200_000_000


def main():
    assert torch.cuda.is_available()
    ctx = gpu.GpuStageContext(0)
    dev = torch.device("cuda:0")
    cols = tpch_synth.lineitem_torch(N, dev, seed=77)
    # control date columns: 100 passes the [50, 150) window, 0 fails it
    i = torch.arange(N, device=dev)
    every_other_line = torch.where((i // 8) % 2 == 0, 100, 0).to(torch.int32)
    every_other_half = torch.where((i // 4) % 2 == 0, 100, 0).to(torch.int32)
    del i
    torch.cuda.synchronize()

    def col_of(t, dtype):
        return gpu.BgColumn(dtype, 15, 2, 0, t.data_ptr(), None, None, t.shape[0])

    sd = col_of(cols["l_shipdate"], gpu.BG_DT_DATE32)
    sd_line = col_of(every_other_line, gpu.BG_DT_DATE32)
    sd_half = col_of(every_other_half, gpu.BG_DT_DATE32)
    cd = col_of(cols["l_discount"], gpu.BG_DT_DECIMAL128)
    cq = col_of(cols["l_quantity"], gpu.BG_DT_DECIMAL128)
    cp = col_of(cols["l_extendedprice"], gpu.BG_DT_DECIMAL128)

    # (name, date column, predicate set, bytes/row at 128-B, at 64-B granules)
    cases = [
        ("all_fail_date", sd, (0, 0, 0, 10, 10**9), 4, 4),
        ("all_pass", sd, (0, 20000, 0, 10, 10**9), 52, 52),
        ("every_other_line", sd_line, (50, 150, 0, 10, 10**9), 28, 28),
        ("every_other_half_line", sd_half, (50, 150, 0, 10, 10**9), 52, 28),
        ("real_q6", sd, (tpch_synth.Q6_DATE_LO, tpch_synth.Q6_DATE_HI,
                         tpch_synth.Q6_DISC_LO, tpch_synth.Q6_DISC_HI,
                         tpch_synth.Q6_QTY_LT), 22.0, 14.9),
    ]
    # untimed warm-up on a 1M-row prefix: the first k_q6_agg dispatch of the
    # process is not one of the cases
    warm = [col_of(t[:1_000_000], dt) for t, dt in
            ((cols["l_shipdate"], gpu.BG_DT_DATE32),
             (cols["l_discount"], gpu.BG_DT_DECIMAL128),
             (cols["l_quantity"], gpu.BG_DT_DECIMAL128),
             (cols["l_extendedprice"], gpu.BG_DT_DECIMAL128))]
    ctx.q6_agg(*warm, *cases[-1][2])
    results = []
    for name, dates, (dlo, dhi, plo, phi, qlt), b128, b64 in cases:
        cnt, total = ctx.q6_agg(dates, cd, cq, cp, dlo, dhi, plo, phi, qlt)
        ms = ctx.L.bg_last_kernel_ms()
        results.append({"case": name, "rows": N, "count": cnt,
                        "kernel_ms": ms,
                        "model_bytes_128B_granule": b128 * N,
                        "model_bytes_64B_granule": b64 * N,
                        "gbps_vs_128B_model": b128 * N / ms / 1e6})
        print(json.dumps(results[-1]), flush=True)
    with open(os.path.join(ROOT, "gpurun_out", "pmc_cases.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
