#!/usr/bin/env python3
"""Flagship bench: TPC-H q6 SF100 hot path (scan+filter+SUM(Decimal128)) on
MI355X, inputs resident in HBM — BASELINE.json configs[1], the largest
single-GPU configuration ("TPC-H q6 SF100 on 1 MI355X, Parquet resident in
HBM").  A "step" = one full q6 pass over the SF100-shaped lineitem columns
(600,037,902 rows pinned by tpch_plan_stability/fixtures.rs:50; synthetic —
no network for real dbgen data).

Contract: python bench.py --gpus N --steps K --warmup W [--full]
                          [--dump-outputs DIR]
  - a plain run does only what the headline figure needs: set up, warm up,
    time the K steps, print the result line.  --full adds every other
    measurement (today: the cpu_baseline leg).  --dump-outputs DIR writes
    what the last timed step returned to its caller as DIR/<name>.npy
    (float64); inputs are seeded, so two builds compare output for output.
  - W untimed warmup steps, then exactly K timed steps bracketed by a
    barrier + torch.cuda.synchronize() on both sides; MAX over ranks;
    rank 0 prints ONE JSON line.
  - value = whole-job rows/s over all N GPUs; scaling "weak" (each rank owns
    its own SF100-shaped shard; the only exchange is the final-aggregate
    merge of one Decimal128 partial per rank — q6 has no data-path
    collective).
  - roofline: dominant kernel = k_q6_agg; achieved = algorithmic bytes
    (52 B/row: Date32 4 + 3 x Decimal128 16) / kernel ms
    measured with hipEvents on the launch stream inside libballista_gpu.so
    (bg_last_kernel_ms); peak 8 TB/s HBM3E (MI355X_MICROARCH.md);
    traffic from profiles/pmc_q6.json when a PMC calibration exists.
  - cpu_baseline: the oracle's q6 C path (kind "port", test infrastructure
    used here only as the reported baseline) timed on this box's host cores
    over a bounded sample.  Only with --full.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ROWS_SF100 = 600_037_902  # lineitem row count at SF100 (fixtures.rs:50)
BYTES_PER_ROW = 52        # Date32(4) + 3 x Decimal128(16) — SURVEY.md §8d
HBM_PEAK_GBS = 8000.0     # 8 TB/s HBM3E spec peak (MI355X_MICROARCH.md)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rows", type=int, default=ROWS_SF100,
                   help="rows per GPU (default SF100 lineitem)")
    p.add_argument("--mode", choices=["q6", "q5"], default="q6",
                   help="q6: flagship resident scan+filter+agg (driver "
                        "contract); q5: q5-class hash-repartition resident "
                        "shuffle (hash->split->all-to-all->final agg, "
                        "SURVEY.md §8e)")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements the headline figure does "
                        "not need (the all-core cpu_baseline leg); off by "
                        "default so a plain run stays lean")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed "
                        "step returned as DIR/<name>.npy (float64)")
    p.add_argument("--cpu-sample-rows", type=int, default=100_000_000)
    p.add_argument("--skip-cpu-baseline", action="store_true",
                   help="with --full: leave the cpu_baseline leg out")
    return p.parse_args()


def setup_dist(args):
    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl")
        torch.cuda.set_device(local_rank)
        return dist, rank, world, local_rank
    torch.cuda.set_device(local_rank)
    return None, rank, world, local_rank


def i128_to_limbs(v: int):
    """exact i128 -> 4 x 32-bit limbs (for exact allreduce in int64)."""
    u = v & ((1 << 128) - 1)
    return [(u >> (32 * i)) & 0xFFFFFFFF for i in range(4)]


def limbs_to_i128(limbs):
    u = 0
    for i, l in enumerate(limbs):
        u += int(l) << (32 * i)
    u &= (1 << 128) - 1
    if u >= 1 << 127:
        u -= 1 << 128
    return u


def dump_outputs(dirname, arrays):
    """--dump-outputs: one float64 .npy per named output of the last timed
    step.  Exact integers wider than 2^53 go out as 32-bit limbs (little
    endian), each exact in float64, next to their rounded float64 value."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, vals in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"),
                np.asarray(vals, dtype=np.float64))


def cpu_baseline_leg(sample_rows: int):
    """Oracle q6 C path on ALL host cores (OpenMP; SURVEY.md §8d: the CPU
    baseline runs on the box's host cores, core count stated) — a reported
    baseline, not the target."""
    import numpy as np
    import oracle
    from datafusion_ballista_amd import tpch_synth
    cores = os.cpu_count() or 1
    li = tpch_synth.lineitem_numpy(sample_rows, seed=123)
    d16 = tpch_synth.dec128_pairs_np(li["l_discount"]).view(np.uint8).reshape(-1)
    q16 = tpch_synth.dec128_pairs_np(li["l_quantity"]).view(np.uint8).reshape(-1)
    p16 = tpch_synth.dec128_pairs_np(li["l_extendedprice"]).view(np.uint8).reshape(-1)
    # bounded sample, repeated until >= ~10 s of CPU work (the contract's
    # 10-30 s window) — the rate is per-row so repetition is neutral
    def one_pass():
        oracle.q6_omp(li["l_shipdate"], d16, q16, p16, tpch_synth.Q6_DATE_LO,
                      tpch_synth.Q6_DATE_HI, tpch_synth.Q6_DISC_LO,
                      tpch_synth.Q6_DISC_HI, tpch_synth.Q6_QTY_LT)
    t0 = time.perf_counter()
    one_pass()
    dt = time.perf_counter() - t0
    passes = 1
    target = 10.0
    while dt < target and passes < 1024:
        more = min(1023, max(1, int((target - dt) / max(dt / passes, 1e-3))))
        for _ in range(more):
            one_pass()
        passes += more
        dt = time.perf_counter() - t0
    return {
        "value": sample_rows * passes / dt,
        "unit": "rows/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{sample_rows} synthetic q6-shaped rows x {passes} passes, "
                  f"{dt:.2f}s C oracle (OpenMP, {cores} cores)",
    }


def q5_mode(args, dist, rank, world, local_rank):
    """q5-class resident shuffle: each rank hash-
    repartitions its shard into K = 16*world global partitions on device
    (compute_partition_indices + split + partition-major materialise,
    writer.rs:1259-1279/564-753), the partition-major buffers cross ranks
    as an RCCL all-to-all over xGMI (exchange.py; replaces the remote-read
    byte movement of shuffle_reader.rs:704-716), and each rank runs the
    FINAL grouped aggregate over the raw rows it received.  Byte
    conservation and an exact global-sum invariant assert every step;
    partition ownership of received keys is device-verified on step 1."""
    import ctypes

    import numpy as np
    import torch

    from datafusion_ballista_amd import exchange, gpu

    device = torch.device(f"cuda:{local_rank}")
    ctx = gpu.GpuStageContext(local_rank)
    n = args.rows if args.rows != ROWS_SF100 else 150_000_000
    k_local = 16
    K = k_local * world
    g = torch.Generator(device=device)
    g.manual_seed(500 + rank)
    nkeys = 15_000_000 * world
    keys = torch.randint(0, nkeys, (n,), generator=g, device=device,
                         dtype=torch.int64)
    price = torch.zeros((n, 2), dtype=torch.int64, device=device)
    price[:, 0] = torch.randint(90000, 10495100, (n,), generator=g,
                                device=device)
    qty = torch.randint(1, 51, (n,), generator=g, device=device,
                        dtype=torch.int64)
    torch.cuda.synchronize()

    # exact global invariant, computed once
    local_sum = int(price[:, 0].sum().item())
    local_rows = n
    if dist is not None:
        t = torch.tensor(i128_to_limbs(local_sum) + [local_rows],
                         dtype=torch.int64, device=device)
        dist.all_reduce(t)
        m = t.cpu().tolist()
        global_sum, global_rows = limbs_to_i128(m[:4]), m[4]
    else:
        global_sum, global_rows = local_sum, local_rows

    def col_of(t, dtype):
        return gpu.BgColumn(dtype, 15, 2, 0, t.data_ptr(), None, None,
                            t.shape[0])

    idx = torch.empty(n, dtype=torch.int32, device=device)
    offs = torch.empty(K + 1, dtype=torch.int64, device=device)
    out_keys = torch.empty(n, dtype=torch.int64, device=device)
    out_price = torch.empty((n, 2), dtype=torch.int64, device=device)
    out_qty = torch.empty(n, dtype=torch.int64, device=device)

    agg_cap = max(2 * nkeys // max(world, 1), 1 << 20)
    agg_first = ctx.alloc(4 * agg_cap)
    agg_acc = ctx.alloc(16 * 2 * agg_cap)
    agg_counts = ctx.alloc(8 * agg_cap)

    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    repart_ms = []
    checked = {"ownership": False}
    last = {}

    def step():
        kc = col_of(keys, gpu.BG_DT_INT64)
        payload = (gpu.BgColumn * 3)(col_of(keys, gpu.BG_DT_INT64),
                                     col_of(price, gpu.BG_DT_DECIMAL128),
                                     col_of(qty, gpu.BG_DT_INT64))
        outp = (ctypes.c_void_p * 3)(out_keys.data_ptr(),
                                     out_price.data_ptr(),
                                     out_qty.data_ptr())
        ev0.record()
        gpu._check(ctx.L.bg_hash_repartition(
            ctypes.byref(kc), 1, payload, 3, ctypes.c_int64(n),
            ctypes.c_uint32(K), ctypes.c_void_p(idx.data_ptr()),
            ctypes.c_void_p(offs.data_ptr()), outp), "bg_hash_repartition")
        ev1.record()
        offsets = offs.cpu().numpy()
        # exchange: keys (1 i64/row), price (2 i64/row), qty (1 i64/row)
        if dist is not None:
            rk, splits = exchange.all_to_all_rows(out_keys, offsets, world)
            rp, _ = exchange.all_to_all_rows(out_price.view(-1), offsets * 2,
                                             world)
            rq, _ = exchange.all_to_all_rows(out_qty, offsets, world)
        else:
            rk, rp, rq = out_keys, out_price.view(-1), out_qty
            splits = [n]
        m = rk.shape[0]
        # final grouped aggregate over the received raw rows (device
        # outputs; parity of the aggregate itself is pinned by the test
        # suite — the bench asserts the EXCHANGE invariants below)
        rkc = gpu.BgColumn(gpu.BG_DT_INT64, 0, 0, 0, rk.data_ptr(), None,
                           None, m)
        rpc = gpu.BgColumn(gpu.BG_DT_DECIMAL128, 15, 2, 0, rp.data_ptr(),
                           None, None, m)
        rqc = gpu.BgColumn(gpu.BG_DT_INT64, 0, 0, 0, rq.data_ptr(), None,
                           None, m)
        karr = (gpu.BgColumn * 1)(rkc)
        aarr = (gpu.BgColumn * 2)(rpc, rqc)
        oarr = (ctypes.c_int32 * 2)(gpu.BG_AGG_OP_SUM_DEC128,
                                    gpu.BG_AGG_OP_SUM_I64)
        ng = ctypes.c_int64()
        gpu._check(ctx.L.bg_hashagg(
            karr, 1, aarr, oarr, 2, None, ctypes.c_int64(m),
            ctypes.c_int64(agg_cap), agg_first.ptr, agg_acc.ptr,
            agg_counts.ptr, ctypes.byref(ng)), "bg_hashagg")
        torch.cuda.synchronize()
        repart_ms.append(ev0.elapsed_time(ev1))
        # conservation + exact global-sum invariants (every step): the
        # received price ints sum exactly to the generated global sum
        part_sum = int(rp.view(-1, 2)[:, 0].sum().item())
        rows_recv = m
        if dist is not None:
            t = torch.tensor(i128_to_limbs(part_sum) + [rows_recv],
                             dtype=torch.int64, device=device)
            dist.all_reduce(t)
            mm = t.cpu().tolist()
            tot_sum, tot_rows = limbs_to_i128(mm[:4]), mm[4]
        else:
            tot_sum, tot_rows = part_sum, rows_recv
        assert tot_rows == global_rows, (tot_rows, global_rows)
        assert tot_sum == global_sum, (tot_sum, global_sum)
        assert int(ng.value) > 0
        if not checked["ownership"] and dist is not None:
            # received keys must hash to MY partitions (device check)
            hb = ctx.alloc(max(8 * m, 8))
            pb = ctx.alloc(max(4 * m, 4))
            gpu._check(ctx.L.bg_hash_columns(ctypes.byref(rkc), 1,
                                             ctypes.c_int64(m), hb.ptr),
                       "hash")
            gpu._check(ctx.L.bg_partition_ids(hb.ptr, ctypes.c_int64(m),
                                              ctypes.c_uint32(K), pb.ptr),
                       "pids")
            pids = pb.download(np.uint32, m)
            owners = pids // k_local
            assert (owners == rank).all(), "foreign rows received"
            checked["ownership"] = True
        last.update(rows_received=m, groups=int(ng.value),
                    price_sum=part_sum)
        return m

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        import torch
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier_sync()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0:
        total_rows = n * world * args.steps
        value = total_rows / elapsed
        kms = sorted(repart_ms)[len(repart_ms) // 2]
        # repartition algorithmic bytes/row: read key+payload
        # once + write once (2 x 32 B) + hash/pids/idx/rank bookkeeping 16 B
        bytes_per_row = 80.0
        achieved_gbs = n * bytes_per_row / (kms * 1e-3) / 1e9
        out = {
            "metric": "tpch_q5class_resident_shuffle_rows_per_s",
            "value": value,
            "unit": "rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int128",
            "data": "synthetic",
            "config": {
                "workload": "tpch_q5class_resident_shuffle",
                "rows_per_gpu": n,
                "k_partitions": K,
                "exchanged_bytes_per_row": 32,
                "parallelism": f"shuffle{world}",
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved_gbs,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved_gbs / HBM_PEAK_GBS,
                "traffic": None,
                "kernel": "bg_hash_repartition pipeline",
                "kernel_ms_median": kms,
            },
            "cpu_baseline": None,
        }
    if args.dump_outputs:
        # this rank's final-aggregate inputs and group count, last step
        dump_outputs(args.dump_outputs, {
            f"rows_received_rank{rank}": [last["rows_received"]],
            f"groups_rank{rank}": [last["groups"]],
            f"price_sum_rank{rank}": [float(last["price_sum"])],
            f"price_sum_limbs_rank{rank}": i128_to_limbs(last["price_sum"]),
        })
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def main():
    args = parse_args()
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU visible; bench requires MI355X"}))
        sys.exit(1)
    dist, rank, world, local_rank = setup_dist(args)
    if args.mode == "q5":
        q5_mode(args, dist, rank, world, local_rank)
        return
    device = torch.device(f"cuda:{local_rank}")

    from datafusion_ballista_amd import gpu, tpch_synth
    ctx = gpu.GpuStageContext(local_rank)

    n = args.rows
    # generate the shard directly in HBM (no host staging)
    cols = tpch_synth.lineitem_torch(n, device, seed=1000 + rank)
    torch.cuda.synchronize()

    def col_of(t, dtype):
        return gpu.BgColumn(dtype, 15, 2, 0, t.data_ptr(), None, None,
                            t.shape[0])

    sd = col_of(cols["l_shipdate"], gpu.BG_DT_DATE32)
    cd = col_of(cols["l_discount"], gpu.BG_DT_DECIMAL128)
    cq = col_of(cols["l_quantity"], gpu.BG_DT_DECIMAL128)
    cp = col_of(cols["l_extendedprice"], gpu.BG_DT_DECIMAL128)

    def step():
        cnt, total = ctx.q6_agg(sd, cd, cq, cp, tpch_synth.Q6_DATE_LO,
                                tpch_synth.Q6_DATE_HI, tpch_synth.Q6_DISC_LO,
                                tpch_synth.Q6_DISC_HI, tpch_synth.Q6_QTY_LT)
        # final-aggregate merge across ranks (exact: 32-bit limbs in int64)
        if dist is not None:
            t = torch.tensor(i128_to_limbs(total) + [cnt], dtype=torch.int64,
                             device=device)
            dist.all_reduce(t)
            merged = t.cpu().tolist()
            total = limbs_to_i128(merged[:4])
            cnt = merged[4]
        return cnt, total

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    kernel_ms_samples = []
    for _ in range(args.warmup):
        step()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        cnt, total = step()
        kernel_ms_samples.append(ctx.L.bg_last_kernel_ms())
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0 and args.dump_outputs:
        # what the caller of the timed path received in the last step: the
        # selected-row count and the exact Decimal128 revenue sum
        dump_outputs(args.dump_outputs, {
            "q6_count": [cnt],
            "q6_sum": [float(total)],
            "q6_sum_limbs": i128_to_limbs(total),
        })

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1000.0
        total_rows = n * world * args.steps
        value = total_rows / elapsed

        kms = sorted(kernel_ms_samples)[len(kernel_ms_samples) // 2]
        # Algorithmic bytes per row: the three predicate
        # columns are read for every row (Date32 4 + Decimal128 16 + 16 =
        # 36 B); the price column is only needed for selected rows, and the
        # kernel's predicated load touches a 128-B line iff any of its 8 rows
        # is selected: + 16 B x (1-(1-s)^8).  PMC-verified (profiles/
        # pmc_q6.json): measured HBM traffic 38.2 B/row at s=0.0181 vs 38.18
        # analytic — traffic == algorithmic, no wasted re-reads.
        s_sel = float(cnt) / n
        bytes_per_row = 36.0 + 16.0 * (1.0 - (1.0 - s_sel) ** 8)
        algo_bytes = float(n) * bytes_per_row
        achieved_gbs = algo_bytes / (kms * 1e-3) / 1e9

        traffic = None
        pmc_path = os.path.join(ROOT, "profiles", "pmc_q6.json")
        if os.path.exists(pmc_path):
            try:
                cal = json.load(open(pmc_path))
                traffic = cal["hbm_bytes_per_row"] * n
            except Exception:
                traffic = None

        out = {
            "metric": "tpch_q6_sf100_rows_per_s",
            "value": value,
            "unit": "rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int128",
            "data": "synthetic",
            "config": {
                "workload": "tpch_q6_sf100_hbm_resident",
                "rows_per_gpu": n,
                "bytes_per_row_algorithmic": bytes_per_row,
                "bytes_per_row_full_pass": BYTES_PER_ROW,
                "k_filter_selectivity": float(cnt) / n,
                "parallelism": f"dp{world}",
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved_gbs,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved_gbs / HBM_PEAK_GBS,
                "traffic": traffic,
                "kernel": "k_q6_agg",
                "kernel_ms_median": kms,
            },
            "cpu_baseline": None,
        }
        if args.full and not args.skip_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline_leg(args.cpu_sample_rows)
        print(json.dumps(out), flush=True)

    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
