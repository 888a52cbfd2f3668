"""k_q6_agg as a staged short-circuit scan: each column is loaded only by
lanes whose row passed every earlier test.  These tests pin what that can
get wrong — tile and tail handling, the grid-stride wrap, holes at every
position of a 128-B line and at every stage, full-width Decimal128
comparisons, element-aligned (not line-aligned) column bases and the
BG_Q6_NT switch.  Bit-exact against oracle.q6; values whose high limb is
set are also recomputed with Python ints.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from datafusion_ballista_amd import gpu, tpch_synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernels.hip: BG_BLOCK, BG_Q6_U, BG_MAX_BLOCKS — one tile is T rows
BLOCK, Q6_U, MAX_BLOCKS = 256, 8, 2048
T = BLOCK * Q6_U
N_WRAP = MAX_BLOCKS * T + 258  # smallest sizes at which block 0 takes 2 tiles
N_PAT = 3 * T + 5

Q6 = (tpch_synth.Q6_DATE_LO, tpch_synth.Q6_DATE_HI, tpch_synth.Q6_DISC_LO,
      tpch_synth.Q6_DISC_HI, tpch_synth.Q6_QTY_LT)
OPEN = (-2**31, 2**31 - 1, -2**62, 2**62, 2**62)


@pytest.fixture(scope="module")
def ctx():
    c = gpu.GpuStageContext(0)
    yield c
    c.close()


def dec_bytes(vals):
    return tpch_synth.dec128_pairs_np(np.asarray(vals, dtype=np.int64)) \
        .view(np.uint8).reshape(-1)


def upload(ctx, sd, d16, q16, p16, pad=0):
    """-> column factory over one upload.  pad=1 puts one element in front
    of every column and advances d_data past it (+4 B / +16 B)."""
    bufs = []

    def up(arr, esz):
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        if pad:
            a = np.concatenate([np.full(esz * pad, 0xA5, np.uint8), a])
        bufs.append(ctx.upload(a))
        return bufs[-1].ptr.value + esz * pad

    ptrs = [up(np.asarray(sd, np.int32), 4), up(d16, 16), up(q16, 16),
            up(p16, 16)]
    dts = [gpu.BG_DT_DATE32] + [gpu.BG_DT_DECIMAL128] * 3

    def cols(n):
        out = [gpu.BgColumn(dt, 15, 2, 0, p, None, None, n)
               for dt, p in zip(dts, ptrs)]
        for c in out:
            c._keep = bufs
        return out
    return cols


@pytest.fixture(scope="module")
def synth(ctx):
    li = tpch_synth.lineitem_numpy(N_WRAP, seed=61)
    host = (li["l_shipdate"], dec_bytes(li["l_discount"]),
            dec_bytes(li["l_quantity"]), dec_bytes(li["l_extendedprice"]))
    return host, upload(ctx, *host)


def want(host, n, p):
    sd, d16, q16, p16 = host
    return oracle.q6(sd[:n], d16[:16 * n], q16[:16 * n], p16[:16 * n], *p)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T,
                               T + 1, N_PAT, N_WRAP])
def test_sizes(ctx, synth, n):
    host, cols = synth
    for p in (Q6, OPEN):
        assert ctx.q6_agg(*cols(n), *p) == want(host, n, p)
    if n >= T:
        assert want(host, n, Q6)[0] > 0


# ---------------------------------------------------------------------------
# selection patterns at n = 3T+5
# ---------------------------------------------------------------------------
def pattern_cols(survive, killer):
    """Rows where survive[i] pass all three tests of Q6; every other row is
    failed by the column killer[i] (0 date, 1 discount, 2 quantity) and
    passes the two others."""
    n = len(survive)
    rng = np.random.default_rng(17)
    sd = np.full(n, Q6[0] + 10, np.int32)
    disc = np.full(n, 6, np.int64)
    qty = np.full(n, 100, np.int64)
    price = rng.integers(90_000, 10_495_100, n, dtype=np.int64)
    dead = ~survive
    sd[dead & (killer == 0)] = Q6[1]          # d < date_hi fails
    disc[dead & (killer == 1)] = Q6[3] + 1
    qty[dead & (killer == 2)] = Q6[4]         # qty < qty_lt fails
    return sd, dec_bytes(disc), dec_bytes(qty), dec_bytes(price)


def run_pattern(ctx, survive, killer):
    host = pattern_cols(survive, killer)
    n = len(survive)
    got = ctx.q6_agg(*upload(ctx, *host)(n), *Q6)
    assert got == want(host, n, Q6)
    assert got[0] == int(survive.sum())


def test_pattern_all_pass(ctx):
    run_pattern(ctx, np.ones(N_PAT, bool), np.zeros(N_PAT, np.int64))


def test_pattern_no_date_passes(ctx):
    run_pattern(ctx, np.zeros(N_PAT, bool), np.zeros(N_PAT, np.int64))


def test_pattern_date_passes_no_discount(ctx):
    run_pattern(ctx, np.zeros(N_PAT, bool), np.ones(N_PAT, np.int64))


@pytest.mark.parametrize("k", range(8))
def test_pattern_one_survivor_per_line(ctx, k):
    i = np.arange(N_PAT)
    # the seven dead rows of a line are spread over all three stages
    run_pattern(ctx, i % 8 == k, i % 3)


def test_pattern_survivors_in_last_rows(ctx):
    i = np.arange(N_PAT)
    run_pattern(ctx, i >= N_PAT - 5, i % 3)


# ---------------------------------------------------------------------------
# full-width values
# ---------------------------------------------------------------------------
def wrap128(v):
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >= 1 << 127 else v


def test_full_width_values(ctx):
    n = N_PAT
    rng = np.random.default_rng(23)
    sd = np.full(n, Q6[0] + 1, np.int32)
    # low limb inside the range, high limb 0 / 1 / -1
    hi_d = rng.choice([0, 1, -1], n)
    hi_q = rng.choice([0, 1, -1], n)
    P = (Q6[0], Q6[1], 5, 10**6, Q6[4])
    disc = [int(h) * 2**64 + int(lo) for h, lo in       # only hi == 0 passes
            zip(hi_d, rng.choice([6, 999_983], n))]
    qty = [int(h) * 2**64 + 100 for h in hi_q]      # hi == 1 fails, -1 passes
    # three in four negative, all near 10^15: one price x disc already
    # needs the high limb
    price = [int(s) * (10**15 - int(r)) for s, r in
             zip(rng.choice([1, -1, -1, -1], n), rng.integers(1, 1000, n))]
    host = (sd, oracle.dec128_from_ints(disc), oracle.dec128_from_ints(qty),
            oracle.dec128_from_ints(price))
    keep = [P[2] <= d <= P[3] and q < P[4] for d, q in zip(disc, qty)]
    py = (sum(keep), wrap128(sum(p * d for p, d, k in zip(price, disc, keep)
                                 if k)))
    assert 0 < py[0] < n and any(q < 0 for q, k in zip(qty, keep) if k)
    assert max(abs(p * d) for p, d, k in zip(price, disc, keep) if k) > 2**64
    got = ctx.q6_agg(*upload(ctx, *host)(n), *P)
    assert got == py
    assert got == want(host, n, P)


# ---------------------------------------------------------------------------
# element-aligned bases, BG_Q6_NT switch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [T + 1, N_PAT])
def test_misaligned_bases(ctx, synth, n):
    host = tuple(a[:k * n] for a, k in zip(synth[0], (1, 16, 16, 16)))
    cols = upload(ctx, *host, pad=1)
    for p in (Q6, OPEN):
        assert ctx.q6_agg(*cols(n), *p) == want(host, n, p)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import oracle
from datafusion_ballista_amd import gpu, tpch_synth
n = int(sys.argv[2])
li = tpch_synth.lineitem_numpy(n, seed=29)
b = lambda v: tpch_synth.dec128_pairs_np(v).view(np.uint8).reshape(-1)
d16, q16, p16 = b(li["l_discount"]), b(li["l_quantity"]), b(li["l_extendedprice"])
ctx = gpu.GpuStageContext(0)
sd, _ = ctx.upload_column(li["l_shipdate"], gpu.BG_DT_DATE32)
cd, cq, cp = (ctx.column(gpu.BG_DT_DECIMAL128, ctx.upload(a), n)
              for a in (d16, q16, p16))
P = (tpch_synth.Q6_DATE_LO, tpch_synth.Q6_DATE_HI, tpch_synth.Q6_DISC_LO,
     tpch_synth.Q6_DISC_HI, tpch_synth.Q6_QTY_LT)
got = ctx.q6_agg(sd, cd, cq, cp, *P)
exp = oracle.q6(li["l_shipdate"], d16, q16, p16, *P)
assert got == exp and got[0] > 0, (got, exp)
print("Q6_NT0_OK", got[0])
"""


def test_nt_switch_off_in_child_process():
    # BG_Q6_NT is read once per process: a fresh child takes the cached-load
    # instantiation of the kernel
    env = dict(os.environ, BG_Q6_NT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(N_PAT)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Q6_NT0_OK" in r.stdout
