"""Window functions over sorted input (DataFusion BoundedWindowAggExec /
WindowAggExec, Ballista's PartitionedBoundedWindowAggExec): bg_window_bounds /
_rank / _frame / _agg at the C ABI and the window node through
bg_execute_stage.

Every expected value is a plain-Python restatement of the SQL definition in
this file: partitions and peers by comparing key tuples, a frame as the set
of partition rows that satisfy its two bounds, an aggregate as a loop over
that set with int arithmetic reduced mod 2^64 (Int64) or mod 2^128 kept
exact (Decimal128), math.fsum (Float64).  In the 140,003-row cases, where
that double loop would take minutes, a row whose frame keeps the previous
row's start and does not shrink adds the new members to the previous row's
exact state instead of starting over; Float64 is then accumulated as exact
rationals, whose correctly rounded value is what math.fsum returns
(test_incremental_reference_is_the_direct_one pins the two against each
other).  All comparisons are exact but Float64 sum at 1e-6 relative.

Float64 inputs are 0.5 + uniform[0, 999.5): non-negative and inside
[0, 1000), and no frame's sum is near zero.  The smallest frame sum is 0.5
and the largest running prefix inside one partition 7.5e7, so a prefix
difference is expected within ~1e-7 relative of the exact sum.

The multi-block case is two row sets of 140,003 rows, because one layout
cannot hold all of its seams: "long" has the partition [60,000, 135,000),
"seams" has partitions starting exactly at rows 65,536 and 131,072 with
single-row partitions at 65,535 and 131,071; "one" is a single partition."""
import ctypes
import decimal
import gc
import json
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from datafusion_ballista_amd import gpu, stage

pytestmark = pytest.mark.gpu

BG_OK, BG_ERR_INVALID, BG_ERR_UNSUPPORTED = 0, -3, -4
SENTINEL = 0xDEADBEEF
PAD = 64
UNB, CUR = gpu.BG_WIN_UNBOUNDED, gpu.BG_WIN_CURRENT_ROW
PREC, FOLL = gpu.BG_WIN_PRECEDING, gpu.BG_WIN_FOLLOWING
ROWS, RANGE = gpu.BG_WIN_ROWS, gpu.BG_WIN_RANGE
D = decimal.Decimal
M64, M128 = 1 << 64, 1 << 128
NAN_BITS = 0x7FF8000000000000
GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "window_running_sum.json")


@pytest.fixture(scope="module")
def ctx():
    c = gpu.GpuStageContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool_start(ctx):
    gc.collect()
    return ctx.pool_stats()[:2]


@pytest.fixture()
def reg(ctx):
    keep, names = [], []

    def _reg(name, table):
        keep.append(stage.register_table(ctx, name, table))
        names.append(name)
        return table

    yield _reg
    for n in names:
        stage.unregister_table(n)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def ref_bounds(pkeys, okeys):
    """pkeys/okeys: one tuple per row (None = NULL, which equals NULL).
    -> ps, pe, qs, qe lists."""
    n = len(pkeys)
    ps, qs = [0] * n, [0] * n
    for i in range(n):
        new_p = i == 0 or pkeys[i] != pkeys[i - 1]
        new_q = new_p or okeys[i] != okeys[i - 1]
        ps[i] = i if new_p else ps[i - 1]
        qs[i] = i if new_q else qs[i - 1]
    pe, qe = [n] * n, [n] * n
    for i in range(n - 2, -1, -1):
        pe[i] = i + 1 if ps[i + 1] == i + 1 else pe[i + 1]
        qe[i] = i + 1 if qs[i + 1] == i + 1 else qe[i + 1]
    return ps, pe, qs, qe


def ref_ranks(ps, qs):
    n = len(ps)
    rn = [i - ps[i] + 1 for i in range(n)]
    rk = [qs[i] - ps[i] + 1 for i in range(n)]
    dr = [0] * n
    for i in range(n):
        dr[i] = 1 if ps[i] == i else dr[i - 1] + (1 if qs[i] == i else 0)
    return rn, rk, dr


def in_frame(units, start, end, i, j, qs, qe, key, desc):
    """Is partition row j a member of row i's frame?  start/end: (kind,
    offset).  key: the single order key per row (None = NULL), read only by
    RANGE offset bounds."""
    if units == ROWS:
        lo_ok = (start[0] == UNB or
                 j - i >= {CUR: 0, PREC: -start[1], FOLL: start[1]}[start[0]])
        hi_ok = (end[0] == UNB or
                 j - i <= {CUR: 0, PREC: -end[1], FOLL: end[1]}[end[0]])
        return lo_ok and hi_ok

    def side(bound, is_start):
        kind, x = bound
        if kind == UNB:
            return True
        if kind == CUR or key[i] is None:   # a NULL key: its NULL peers
            return j >= qs[i] if is_start else j < qe[i]
        if key[j] is None:
            return False
        d = x if kind == FOLL else -x
        t = key[i] - d if desc else key[i] + d
        if is_start:
            return key[j] <= t if desc else key[j] >= t
        return key[j] >= t if desc else key[j] <= t
    return side(start, True) and side(end, False)


def ref_frames(units, start, end, ps, pe, qs, qe, key=None, desc=False):
    """-> per row the member list of its frame (contiguous by construction
    of sorted input; asserted)."""
    out = []
    for i in range(len(ps)):
        m = [j for j in range(ps[i], pe[i])
             if in_frame(units, start, end, i, j, qs, qe, key, desc)]
        assert m == list(range(m[0], m[-1] + 1)) if m else True
        out.append((m[0], m[-1] + 1) if m else None)
    return out


def wrap(v, mod):
    v %= mod
    return v - mod if v >= mod // 2 else v


def agg_of(fn, members, kind):
    """fn over the non-NULL members; None = SQL NULL."""
    vals = [v for v in members if v is not None]
    if fn == "count":
        return len(vals)
    if not vals:
        return None
    if fn == "sum":
        if kind == "f64":
            return math.fsum(vals)
        return wrap(sum(vals), M64 if kind == "i64" else M128)
    if kind == "f64":    # IEEE total order
        return (min if fn == "min" else max)(vals, key=f64_order)
    return (min if fn == "min" else max)(vals)


def f64_order(x):
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)


def ref_agg(fn, vals, frames, kind):
    """The double loop: one pass over every row's frame members."""
    return [agg_of(fn, [vals[j] for j in range(*f)] if f else [], kind)
            for f in frames]


def ref_agg_growing(fn, vals, frames, kind):
    """Same values, for the large cases: while consecutive rows keep their
    frame's start and do not shrink it (running, whole-partition and peer
    frames) the new members join the previous row's exact state; any other
    row starts over."""
    out, cur = [], None
    for f in frames:
        if f is None:
            out.append(0 if fn == "count" else None)
            continue
        lo, hi = f
        if cur is None or cur["lo"] != lo or hi < cur["hi"]:
            cur = {"lo": lo, "hi": lo, "cnt": 0, "sum": 0, "ext": None}
        for j in range(cur["hi"], hi):
            v = vals[j]
            if v is None:
                continue
            cur["cnt"] += 1
            if fn == "sum":
                cur["sum"] += Fraction(v) if kind == "f64" else v
            elif fn != "count":
                key = f64_order(v) if kind == "f64" else v
                if cur["ext"] is None or \
                        (key < cur["ext"][0] if fn == "min" else
                         key > cur["ext"][0]):
                    cur["ext"] = (key, v)
        cur["hi"] = hi
        if fn == "count":
            out.append(cur["cnt"])
        elif cur["cnt"] == 0:
            out.append(None)
        elif fn == "sum":
            out.append(float(cur["sum"]) if kind == "f64" else
                       wrap(cur["sum"], M64 if kind == "i64" else M128))
        else:
            out.append(cur["ext"][1])
    return out


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
def enc_value(dtype, v):
    """The small key domain {0..3} under each key type, in sort order."""
    if dtype == "utf8":
        return [b"", b"a", b"ab", b"b"][v]
    if dtype == "f64":
        # -0.0 and +0.0 are different keys; the NaN pattern equals itself
        return [-1.5, -0.0, 0.0, NAN_BITS][v]
    return {"i64": (v - 2) * 10**12, "date32": v * 100 - 50,
            "dec": (v - 2) * (2**70 + 12345)}[dtype]


def upload_col(ctx, dtype, values, p=0, s=0, force_validity=False):
    """values: python values, None = NULL -> BgColumn."""
    n = len(values)
    valid = np.array([v is not None for v in values], dtype=bool)
    vbuf = None
    if force_validity or not valid.all():
        vbuf = ctx.upload(np.packbits(valid, bitorder="little")
                          if n else np.zeros(1, dtype=np.uint8))
    if dtype == "utf8":
        col = ctx.upload_utf8_column([v or b"" for v in values] or [b""])
        col.len = n
        if vbuf is not None:
            col.d_validity = vbuf.ptr.value
            col._keep = col._keep + (vbuf,)
        return col
    if dtype == "dec":
        raw = b"".join((v or 0).to_bytes(16, "little", signed=True)
                       for v in values) or bytes(16)
        arr, code = np.frombuffer(raw, dtype=np.uint8), gpu.BG_DT_DECIMAL128
    elif dtype == "f64":
        bits = [v if isinstance(v, int) else
                struct.unpack("<Q", struct.pack(
                    "<d", 0.0 if v is None else v))[0]
                for v in values] or [0]
        arr, code = np.array(bits, dtype=np.uint64), gpu.BG_DT_FLOAT64
    elif dtype in ("date32", "i32"):
        arr = np.array([v or 0 for v in values] or [0], dtype=np.int32)
        code = gpu.BG_DT_DATE32 if dtype == "date32" else gpu.BG_DT_INT32
    else:
        arr = np.array([v or 0 for v in values] or [0], dtype=np.int64)
        code = gpu.BG_DT_INT64
    return ctx.column(code, ctx.upload(arr), n, validity=vbuf, precision=p,
                      scale=s)


class Case:
    """Sorted rows: partition ids ascending, inside a partition the order
    key over {0..3} in the stated direction with its ~10 % NULLs at the
    stated end.  The partition key is pid % 4, NULL where pid % 7 == 6, so
    neighbouring partitions always differ."""

    def __init__(self, n, seed, lengths=None, desc=False, nulls_first=False,
                 peer_run=None):
        rng = np.random.default_rng(seed)
        if lengths is None:
            lengths = []
            while sum(lengths) < n:
                lengths.append(int(rng.choice([1, 2, 63, 64, 65])))
            if n:
                lengths[-1] -= sum(lengths) - n
        assert sum(lengths) == n
        self.n, self.desc, self.nulls_first = n, desc, nulls_first
        self.pid, self.ok = [], []
        for p, ln in enumerate(lengths):
            if peer_run:     # long partitions: many short peer groups
                keys = [j // peer_run for j in range(ln)]
                nn = ln // 10
                keys = keys[:ln - nn]
            else:
                draws = rng.integers(0, 4, size=ln)
                isnull = rng.random(ln) < 0.1
                keys = sorted(int(d) for d, z in zip(draws, isnull) if not z)
                nn = int(isnull.sum())
            if desc:
                keys.reverse()
            self.ok += [None] * nn + keys if nulls_first else \
                keys + [None] * nn
            self.pid += [p] * ln
        self.pk = [None if p % 7 == 6 else p % 4 for p in self.pid]
        self.bounds = ref_bounds([(p,) for p in self.pid],
                                 [(k,) for k in self.ok])

    def values(self, kind, seed, nullable=True):
        rng = np.random.default_rng(seed)
        n = self.n
        if kind == "i64":      # near +-2^62: the running prefix wraps
            v = [int(x) for x in rng.integers(-2**62, 2**62, size=n)]
            v = [x + (2**61 if x > 0 else -2**61) for x in v]
        elif kind == "i32":
            v = [int(x) for x in rng.integers(-2**31, 2**31, size=n)]
        elif kind == "dec":    # magnitudes near 10^36: the low limb carries
            v = [int(x) * 10**18 + int(y) for x, y in
                 zip(rng.integers(-10**18, 10**18, size=n),
                     rng.integers(0, 10**18, size=n))]
        else:
            v = [0.5 + float(x) * 999.5 for x in rng.random(n)]
        if nullable:
            v = [None if z else x for x, z in zip(v, rng.random(n) < 0.1)]
        return v


SIZES = [0, 1, 63, 64, 65, 257]
BIG = 140_003


def big_lengths():
    """Partition lengths of the multi-block case.  Two layouts cannot both
    hold ([60000, 135000) as ONE partition contains 65536 and 131072), so the
    case is two row sets: A has the long partition, B has the seam-aligned
    starts and the single-row partitions beside them."""
    a = [60000, 75000, BIG - 135000]
    b = [65535, 1, 65535, 1, BIG - 131072]
    assert sum(a) == BIG and sum(b) == BIG
    return a, b


@pytest.fixture(scope="module")
def big_cases():
    a, b = big_lengths()
    return {"long": Case(BIG, 11, lengths=a, peer_run=3),
            "seams": Case(BIG, 12, lengths=b, peer_run=3),
            "one": Case(BIG, 13, lengths=[BIG], peer_run=3)}


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
def sentinel_buf(ctx, n, esz):
    return ctx.upload(np.full((n + PAD) * esz // 4, SENTINEL,
                              dtype=np.uint32))


def read_out(buf, n, esz, np_dtype):
    """First n elements; asserts the PAD-element tail is untouched."""
    raw = buf.download(np.uint32, (n + PAD) * esz // 4)
    assert (raw[n * esz // 4:] == SENTINEL).all(), "wrote past n elements"
    return raw[:n * esz // 4].view(np_dtype)


def sentinel_bits(ctx, n):
    return ctx.upload(np.full((n + 7) // 8 + PAD, 0xA5, dtype=np.uint8))


def read_bits(buf, n):
    """The bitmap's ceil(n/8) bytes as bool[n]; bits past n in the last byte
    must be 0 (written whole) and nothing beyond may change."""
    nb = (n + 7) // 8
    raw = buf.download(np.uint8, nb + PAD)
    assert (raw[nb:] == 0xA5).all(), "wrote past ceil(n/8) validity bytes"
    bits = np.unpackbits(raw[:nb], bitorder="little")
    assert not bits[n:].any(), "bits past n set in the last validity byte"
    return bits[:n].astype(bool)


def run_bounds(ctx, part_cols, order_cols, n):
    bufs = [sentinel_buf(ctx, n, 4) for _ in range(4)]
    ctx.window_bounds(part_cols, order_cols, n, *bufs)
    return bufs, [read_out(b, n, 4, np.uint32).tolist() for b in bufs]


def upload_bounds(ctx, bounds):
    return [ctx.upload(np.array(b or [0], dtype=np.uint32)) for b in bounds]


def run_frame(ctx, units, start, end, order_col, desc, dbounds, n):
    lo, hi = sentinel_buf(ctx, n, 4), sentinel_buf(ctx, n, 4)
    ctx.window_frame(units, start, end, order_col, desc, dbounds, n, lo, hi)
    return (lo, hi, read_out(lo, n, 4, np.uint32).tolist(),
            read_out(hi, n, 4, np.uint32).tolist())


OUT_OF = {"i64": (8, np.int64), "i32": (4, np.int32), "f64": (8, np.float64),
          "dec": (16, np.uint8)}
FN_CODE = {"sum": gpu.BG_WIN_SUM, "count": gpu.BG_WIN_COUNT,
           "min": gpu.BG_WIN_MIN, "max": gpu.BG_WIN_MAX}


def run_agg(ctx, fn, col, kind, d_ps, d_lo, d_hi, n):
    """-> python values, None where the validity bit is clear."""
    esz, npdt = OUT_OF["i64" if fn == "count" else kind]
    out = sentinel_buf(ctx, n, esz)
    vbits = sentinel_bits(ctx, n) if fn != "count" else None
    ctx.window_agg(FN_CODE[fn], col, d_ps, d_lo, d_hi, n, out, vbits)
    raw = read_out(out, n, esz, npdt)
    if fn == "count":
        return raw.tolist()
    valid = read_bits(vbits, n)
    if kind == "dec":
        b = raw.tobytes()
        vals = [int.from_bytes(b[16 * i:16 * i + 16], "little", signed=True)
                for i in range(n)]
    else:
        vals = raw.tolist()
    assert all(v == 0 for v, ok in zip(vals, valid) if not ok)
    return [v if ok else None for v, ok in zip(vals, valid)]


def same(got, want, kind, fn):
    if kind == "f64" and fn == "sum":
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if w is not None:
                assert abs(g - w) <= 1e-6 * abs(w), (g, w)
    else:
        assert got == want


# ---------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------
def test_incremental_reference_is_the_direct_one():
    case = Case(257, 5)
    ps, pe, qs, qe = case.bounds
    for units, start, end in [(ROWS, (UNB, 0), (CUR, 0)),
                              (ROWS, (UNB, 0), (UNB, 0)),
                              (RANGE, (UNB, 0), (CUR, 0))]:
        fr = ref_frames(units, start, end, ps, pe, qs, qe)
        for kind in ("i64", "dec", "f64"):
            vals = case.values(kind, 9)
            for fn in ("sum", "count", "min", "max"):
                assert ref_agg_growing(fn, vals, fr, kind) == \
                    ref_agg(fn, vals, fr, kind)


# ---------------------------------------------------------------------------
# ABI level: bounds and ranks
# ---------------------------------------------------------------------------
KEY_TYPES = ["i64", "date32", "dec", "utf8", "f64"]


def check_bounds_and_ranks(ctx, case, dtype):
    n = case.n
    pcol = upload_col(ctx, dtype, [None if v is None else enc_value(dtype, v)
                                   for v in case.pk])
    ocol = upload_col(ctx, dtype, [None if v is None else enc_value(dtype, v)
                                   for v in case.ok])
    bufs, got = run_bounds(ctx, [pcol], [ocol], n)
    want = [list(b) for b in case.bounds]
    assert got == want
    rn, rk, dr = ref_ranks(case.bounds[0], case.bounds[2])
    for fn, exp in ((gpu.BG_WIN_ROW_NUMBER, rn), (gpu.BG_WIN_RANK, rk),
                    (gpu.BG_WIN_DENSE_RANK, dr)):
        out = sentinel_buf(ctx, n, 8)
        ctx.window_rank(fn, bufs[0], bufs[2], n, out)
        assert read_out(out, n, 8, np.int64).tolist() == exp


@pytest.mark.parametrize("dtype", KEY_TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_bounds_and_ranks(ctx, pool_start, n, dtype):
    check_bounds_and_ranks(ctx, Case(n, 100 + n), dtype)


def test_float64_keys_compare_by_bit_pattern(ctx, pool_start):
    # -0.0 | +0.0 | NaN NaN: three peer groups in one partition
    keys = [-0.0, 0.0, NAN_BITS, NAN_BITS]
    ocol = upload_col(ctx, "f64", keys)
    _, got = run_bounds(ctx, [], [ocol], 4)
    assert got == [[0] * 4, [4] * 4, [0, 1, 2, 2], [1, 2, 4, 4]]


def test_every_row_its_own_partition(ctx, pool_start):
    n = 257
    col = upload_col(ctx, "i64", list(range(n)))
    bufs, got = run_bounds(ctx, [col], [], n)
    assert got == [list(range(n)), list(range(1, n + 1))] * 2
    out = sentinel_buf(ctx, n, 8)
    ctx.window_rank(gpu.BG_WIN_DENSE_RANK, bufs[0], bufs[2], n, out)
    assert read_out(out, n, 8, np.int64).tolist() == [1] * n


def test_two_partition_keys_and_two_order_keys(ctx, pool_start):
    case = Case(257, 21)
    rng = np.random.default_rng(3)
    o2 = [int(x) for x in rng.integers(0, 2, size=257)]
    pcols = [upload_col(ctx, "utf8", [None if v is None else
                                       enc_value("utf8", v) for v in case.pk]),
             upload_col(ctx, "i64", [p // 4 for p in case.pid])]
    ocols = [upload_col(ctx, "date32", case.ok), upload_col(ctx, "i64", o2)]
    _, got = run_bounds(ctx, pcols, ocols, 257)
    want = ref_bounds([(k, p // 4) for k, p in zip(case.pk, case.pid)],
                      list(zip(case.ok, o2)))
    assert got == [list(b) for b in want]


@pytest.mark.parametrize("which", ["long", "seams", "one"])
def test_bounds_and_ranks_across_block_seams(ctx, pool_start, big_cases,
                                             which):
    case = big_cases[which]
    ps = case.bounds[0]
    if which == "long":
        assert ps[60000] == 60000 and ps[134999] == 60000
    if which == "seams":
        assert ps[65535] == 65535 and ps[65536] == 65536
        assert ps[131071] == 131071 and ps[131072] == 131072
        assert case.bounds[1][65535] == 65536
    check_bounds_and_ranks(ctx, case, "i64")


# ---------------------------------------------------------------------------
# ABI level: frames and aggregates
# ---------------------------------------------------------------------------
def P(x):
    return (PREC, x)


def F(x):
    return (FOLL, x)


ROWS_FRAMES = [((UNB, 0), (CUR, 0)), ((UNB, 0), (UNB, 0)), (P(2), F(1)),
               (P(3), P(1)), (F(1), F(3)), ((CUR, 0), (UNB, 0))]
RANGE_PEER_FRAMES = [((UNB, 0), (CUR, 0)), ((CUR, 0), (CUR, 0)),
                     ((UNB, 0), (UNB, 0))]
RANGE_OFFSET_FRAMES = [(P(1), F(1)), (P(2), (CUR, 0)), ((CUR, 0), F(2)),
                       (F(1), F(2))]


def check_frame(got_lo, got_hi, want, bounds):
    ps, pe = bounds[0], bounds[1]
    for i, f in enumerate(want):
        assert ps[i] <= got_lo[i] <= got_hi[i] <= pe[i], i
        if f is None:
            assert got_lo[i] == got_hi[i], i
        else:
            assert (got_lo[i], got_hi[i]) == f, i


AGG_INPUTS = [("i64", True), ("i64", False), ("dec", True), ("f64", True),
              ("i32", True)]


def check_aggs(ctx, case, frames, d_bounds, d_lo, d_hi, start_unbounded,
               ref=ref_agg, seed=7, inputs=None):
    """Every aggregate the frame allows, over every input type (or the
    listed ones)."""
    n = case.n
    lo_arg = None if start_unbounded else d_lo
    got = run_agg(ctx, "count", None, "i64", d_bounds[0], lo_arg, d_hi, n)
    assert got == [f[1] - f[0] if f else 0 for f in frames]      # count(*)
    for kind, nullable in inputs or AGG_INPUTS:
        vals = case.values(kind, seed, nullable)
        dt = {"i64": "i64", "i32": "i32", "dec": "dec", "f64": "f64"}[kind]
        col = upload_col(ctx, dt, vals, p=38 if kind == "dec" else 0, s=6)
        fns = ["count"] + ([] if kind == "i32" else ["sum"]) + \
            (["min", "max"] if start_unbounded else [])
        for fn in fns:
            got = run_agg(ctx, fn, col, kind, d_bounds[0], lo_arg, d_hi, n)
            same(got, ref(fn, vals, frames, kind), kind, fn)


@pytest.mark.parametrize("n", SIZES)
def test_rows_frames_and_aggregates(ctx, pool_start, n):
    case = Case(n, 200 + n)
    d_bounds = upload_bounds(ctx, case.bounds)
    for start, end in ROWS_FRAMES:
        want = ref_frames(ROWS, start, end, *case.bounds)
        d_lo, d_hi, lo, hi = run_frame(ctx, ROWS, start, end, None, False,
                                       d_bounds, n)
        check_frame(lo, hi, want, case.bounds)
        check_aggs(ctx, case, want, d_bounds, d_lo, d_hi, start[0] == UNB)


@pytest.mark.parametrize("n", SIZES)
def test_range_peer_frames_with_two_order_keys(ctx, pool_start, n):
    case = Case(n, 300 + n)
    rng = np.random.default_rng(n)
    o2 = [int(x) for x in rng.integers(0, 2, size=n)]
    # the second key sorted inside each peer group of the first
    ps, pe, qs, qe = case.bounds
    for i in sorted(set(qs)):
        o2[i:qe[i]] = sorted(o2[i:qe[i]])
    bounds = ref_bounds([(p,) for p in case.pid], list(zip(case.ok, o2)))
    d_bounds = upload_bounds(ctx, bounds)
    for start, end in RANGE_PEER_FRAMES:
        want = ref_frames(RANGE, start, end, *bounds)
        d_lo, d_hi, lo, hi = run_frame(ctx, RANGE, start, end, None, False,
                                       d_bounds, n)
        check_frame(lo, hi, want, bounds)
        check_aggs(ctx, case, want, d_bounds, d_lo, d_hi, start[0] == UNB)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("dtype", ["i64", "date32"])
def test_range_offset_frames(ctx, pool_start, dtype, nulls_first, desc, n):
    case = Case(n, 400 + n, desc=desc, nulls_first=nulls_first)
    d_bounds = upload_bounds(ctx, case.bounds)
    ocol = upload_col(ctx, dtype, case.ok, force_validity=n == 64)
    for start, end in RANGE_OFFSET_FRAMES:
        want = ref_frames(RANGE, start, end, *case.bounds, key=case.ok,
                          desc=desc)
        d_lo, d_hi, lo, hi = run_frame(ctx, RANGE, start, end, ocol, desc,
                                       d_bounds, n)
        check_frame(lo, hi, want, case.bounds)
        check_aggs(ctx, case, want, d_bounds, d_lo, d_hi, False)


@pytest.mark.parametrize("n", [0, 63, 257])
def test_range_offset_frames_over_float64(ctx, pool_start, n):
    case = Case(n, 500 + n)
    keys = [None if k is None else k * 0.5 for k in case.ok]
    d_bounds = upload_bounds(ctx, case.bounds)
    ocol = upload_col(ctx, "f64", keys)
    for start, end in RANGE_OFFSET_FRAMES:
        fs, fe = (start[0], float(start[1])), (end[0], float(end[1]))
        want = ref_frames(RANGE, fs, fe, *case.bounds, key=keys)
        d_lo, d_hi, lo, hi = run_frame(ctx, RANGE, fs, fe, ocol, False,
                                       d_bounds, n)
        check_frame(lo, hi, want, case.bounds)
        check_aggs(ctx, case, want, d_bounds, d_lo, d_hi, False)


def test_all_null_partition_and_empty_frames(ctx, pool_start):
    # partitions of 3, 4 (all NULL) and 2 rows
    bounds = ref_bounds([(0,)] * 3 + [(1,)] * 4 + [(2,)] * 2, [()] * 9)
    d_bounds = upload_bounds(ctx, bounds)
    vals = [5, None, 7, None, None, None, None, -1, 2]
    col = upload_col(ctx, "i64", vals)
    d_lo, d_hi, lo, hi = run_frame(ctx, ROWS, (UNB, 0), (UNB, 0), None, False,
                                   d_bounds, 9)
    for fn, want in (("sum", [12] * 3 + [None] * 4 + [1] * 2),
                     ("min", [5] * 3 + [None] * 4 + [-1] * 2),
                     ("max", [7] * 3 + [None] * 4 + [2] * 2),
                     ("count", [2] * 3 + [0] * 4 + [2] * 2)):
        assert run_agg(ctx, fn, col, "i64", d_bounds[0], None, d_hi, 9) == want
    # 3 preceding .. 1 preceding is empty on every partition's first row
    d_lo, d_hi, lo, hi = run_frame(ctx, ROWS, P(3), P(1), None, False,
                                   d_bounds, 9)
    assert [a == b for a, b in zip(lo, hi)] == \
        [True, False, False, True, False, False, False, True, False]
    assert run_agg(ctx, "sum", col, "i64", d_bounds[0], d_lo, d_hi, 9) == \
        [None, 5, 5, None, None, None, None, None, -1]
    assert run_agg(ctx, "count", col, "i64", d_bounds[0], d_lo, d_hi, 9) == \
        [0, 1, 1, 0, 0, 0, 0, 0, 1]


# the multi-block shapes: (units, start, end, the aggregate inputs checked)
BIG_SHAPES = {
    "rows_running": (ROWS, (UNB, 0), (CUR, 0), [("i64", True), ("dec", True)]),
    "rows_whole": (ROWS, (UNB, 0), (UNB, 0), [("f64", True), ("i32", True)]),
    "range_running": (RANGE, (UNB, 0), (CUR, 0), [("f64", True)]),
    "rows_sliding": (ROWS, P(2), F(1), [("dec", True), ("f64", True)]),
    "range_peers": (RANGE, (CUR, 0), (CUR, 0), [("i64", False)]),
}


def big_frames(shape, bounds):
    """Frames in closed form: the double loop over a 75,000-row partition
    would take minutes, and the small cases pin these forms to it."""
    ps, pe, qs, qe = bounds
    n = len(ps)
    return {"rows_running": lambda: [(ps[i], i + 1) for i in range(n)],
            "rows_whole": lambda: list(zip(ps, pe)),
            "range_running": lambda: list(zip(ps, qe)),
            "rows_sliding": lambda: [(max(ps[i], i - 2), min(pe[i], i + 2))
                                     for i in range(n)],
            "range_peers": lambda: list(zip(qs, qe))}[shape]()


@pytest.mark.parametrize("shape", sorted(BIG_SHAPES))
@pytest.mark.parametrize("which", ["long", "seams", "one"])
def test_frames_and_aggregates_across_block_seams(ctx, pool_start, big_cases,
                                                  which, shape):
    case = big_cases[which]
    n = case.n
    d_bounds = upload_bounds(ctx, case.bounds)
    units, start, end, inputs = BIG_SHAPES[shape]
    want = big_frames(shape, case.bounds)
    d_lo, d_hi, lo, hi = run_frame(ctx, units, start, end, None, False,
                                   d_bounds, n)
    check_frame(lo, hi, want, case.bounds)
    check_aggs(ctx, case, want, d_bounds, d_lo, d_hi, start[0] == UNB,
               ref=ref_agg if shape == "rows_sliding" else ref_agg_growing,
               inputs=inputs)


@pytest.mark.parametrize("which", ["long", "seams", "one"])
def test_range_offset_frame_across_block_seams(ctx, pool_start, big_cases,
                                               which):
    case = big_cases[which]
    n = case.n
    d_bounds = upload_bounds(ctx, case.bounds)
    ps, pe, qs, qe = case.bounds
    # one RANGE offset frame: peer runs of 3 equal keys, keys k-1 .. k+1
    ocol = upload_col(ctx, "i64", case.ok)
    d_lo, d_hi, lo, hi = run_frame(ctx, RANGE, P(1), F(1), ocol, False,
                                   d_bounds, n)
    want = []
    for i in range(n):
        if case.ok[i] is None:
            want.append((qs[i], qe[i]))
            continue
        a = qs[i]
        if a > ps[i] and case.ok[a - 1] is not None:
            a = qs[a - 1]
        b = qe[i]
        if b < pe[i] and case.ok[b] is not None:
            b = qe[b]
        want.append((a, b))
    check_frame(lo, hi, want, case.bounds)


# ---------------------------------------------------------------------------
# ABI level: errors and the pool
# ---------------------------------------------------------------------------
def test_refusals_leave_the_pool_alone(ctx, pool_start):
    L = ctx.L
    n = 65
    case = Case(n, 1)
    d_bounds = upload_bounds(ctx, case.bounds)
    col = upload_col(ctx, "i64", case.values("i64", 1))
    out, vb = sentinel_buf(ctx, n, 8), sentinel_bits(ctx, n)
    gc.collect()
    before = ctx.pool_stats()[:2]
    rc = L.bg_window_agg(gpu.BG_WIN_MIN, ctypes.byref(col), d_bounds[0].ptr,
                         d_bounds[2].ptr, d_bounds[1].ptr, n, out.ptr, vb.ptr)
    assert rc == BG_ERR_UNSUPPORTED
    assert "MIN/MAX" in L.bg_last_error().decode()
    cols = (gpu.BgColumn * 5)(*[col] * 5)
    rc = L.bg_window_bounds(cols, 5, cols, 1, n, d_bounds[0].ptr, None, None,
                            None)
    assert rc == BG_ERR_INVALID
    rc = L.bg_window_rank(gpu.BG_WIN_RANK, None, None, 2**32 - 1, out.ptr)
    assert rc == BG_ERR_INVALID
    rc = L.bg_window_frame(2, UNB, 0, CUR, 0, None, 0, d_bounds[0].ptr,
                           d_bounds[1].ptr, None, None, n, out.ptr, out.ptr)
    assert rc == BG_ERR_UNSUPPORTED
    rc = L.bg_window_frame(ROWS, PREC, -1, CUR, 0, None, 0, d_bounds[0].ptr,
                           d_bounds[1].ptr, None, None, n, out.ptr, out.ptr)
    assert rc == BG_ERR_INVALID
    assert ctx.pool_stats()[:2] == before
    # nothing was written by any refused call
    assert (out.download(np.uint32, (n + PAD) * 2) == SENTINEL).all()


# ---------------------------------------------------------------------------
# stage level
# ---------------------------------------------------------------------------
def scan_of(table, name):
    return {"op": "scan", "schema": stage.schema_json(table.schema),
            "source": {"kind": "device", "table": name}}


def _doc(plan):
    return {"job_id": "w", "stage_id": 1, "task_id": 0,
            "work_dir": "/tmp/bg_window", "plan": {"op": "collect",
                                                   "input": plan}}


def run_window(table, name, partition_by, order_by, exprs, pre=None):
    """sort by (partition_by, order_by) then window -> (schema, rows)."""
    src = scan_of(table, name) if pre is None else pre
    keys = [{"col": c} for c in partition_by] + order_by
    node = {"op": "window", "partition_by": partition_by,
            "order_by": order_by, "exprs": exprs,
            "input": {"op": "sort", "keys": keys, "input": src}}
    res = stage.execute(_doc(node))
    return res["schema"], [tuple(r) for r in res["rows"]]


def dec_array(unscaled, p, s):
    return pa.array([None if v is None else D(v).scaleb(-s) for v in unscaled],
                    type=pa.decimal128(p, s))


def sort_key(v, desc, nulls_first):
    """Python sort key for one SQL order key."""
    null_rank = 0 if nulls_first else 2
    if v is None:
        return (null_rank, 0)
    return (1, -v if desc else v)


def test_q67_shape_three_ranks_in_one_node(ctx, reg):
    rng = np.random.default_rng(67)
    n = 300
    cat = [int(x) for x in rng.integers(0, 7, size=n)]
    sales = [None if z else int(x) for x, z in
             zip(rng.integers(0, 12, size=n), rng.random(n) < 0.1)]
    t = reg("w67", pa.table({"cat": pa.array(cat, pa.int64()),
                             "sales": pa.array(sales, pa.int64()),
                             "id": pa.array(range(n), pa.int64())}))
    schema, rows = run_window(
        t, "w67", ["cat"], [{"col": "sales", "desc": True}],
        [{"fn": "rank", "as": "rk"}, {"fn": "row_number", "as": "rn"},
         {"fn": "dense_rank", "as": "dr"}])
    assert [f["name"] for f in schema] == ["cat", "sales", "id", "rk", "rn",
                                           "dr"]
    assert all(f["dtype"] == "int64" for f in schema)
    # DESC defaults to NULLS FIRST; the sort is stable, so ties keep id order
    order = sorted(range(n), key=lambda i: (cat[i],
                                            sort_key(sales[i], True, True), i))
    want = []
    for pos, i in enumerate(order):
        part = [j for j in order if cat[j] == cat[i]]
        before = [j for j in part if sort_key(sales[j], True, True) <
                  sort_key(sales[i], True, True)]
        want.append((cat[i], sales[i], i, len(before) + 1,
                     part.index(i) + 1,
                     len({sales[j] for j in before}) + 1))
    assert rows == want


def test_q53_shape_whole_partition_avg_over_decimal(ctx, reg):
    rng = np.random.default_rng(53)
    n = 200
    k = [int(x) for x in rng.integers(0, 9, size=n)]
    x = [None if z else int(v) for v, z in
         zip(rng.integers(-10**9, 10**9, size=n), rng.random(n) < 0.15)]
    t = reg("w53", pa.table({"k": pa.array(k, pa.int64()),
                             "x": dec_array(x, 17, 2)}))
    schema, rows = run_window(
        t, "w53", ["k"], [],
        [{"fn": "avg", "as": "a", "expr": {"col": "x"},
          "frame": {"units": "rows", "start": "unbounded",
                    "end": "unbounded"}}])
    assert schema[-1] == {"name": "a", "dtype": "decimal128", "precision": 21,
                          "scale": 6}
    c = decimal.Context(prec=60, rounding=decimal.ROUND_HALF_UP)
    order = sorted(range(n), key=lambda i: (k[i], i))
    want = []
    for i in order:
        mem = [D(x[j]) for j in range(n) if k[j] == k[i] and x[j] is not None]
        avg = None
        if mem:
            q = c.divide(sum(mem, D(0)) * 10**4, D(len(mem)))
            avg = str(int(q.quantize(D(1), rounding=decimal.ROUND_HALF_UP)))
        want.append((k[i], None if x[i] is None else str(x[i]), avg))
    assert rows == want


def test_q51_shape_running_sum_and_max_over_decimal(ctx, reg):
    rng = np.random.default_rng(51)
    n = 260
    item = [int(v) for v in rng.integers(0, 5, size=n)]
    day = [int(v) for v in rng.permutation(n)]           # distinct dates
    amt = [None if z else int(v) for v, z in
           zip(rng.integers(-10**12, 10**12, size=n), rng.random(n) < 0.1)]
    t = reg("w51", pa.table({"item": pa.array(item, pa.int64()),
                             "d": pa.array(day, pa.date32()),
                             "amt": dec_array(amt, 15, 2)}))
    running = {"units": "rows", "start": "unbounded", "end": "current_row"}
    schema, rows = run_window(
        t, "w51", ["item"], [{"col": "d"}],
        [{"fn": "sum", "as": "cume", "expr": {"col": "amt"}, "frame": running},
         {"fn": "max", "as": "hi", "expr": {"col": "amt"}, "frame": running}])
    assert schema[-2:] == [
        {"name": "cume", "dtype": "decimal128", "precision": 38, "scale": 2},
        {"name": "hi", "dtype": "decimal128", "precision": 15, "scale": 2}]
    want = []
    for i in sorted(range(n), key=lambda i: (item[i], day[i])):
        mem = [D(amt[j]) for j in range(n) if item[j] == item[i] and
               day[j] <= day[i] and amt[j] is not None]
        want.append((item[i], day[i], None if amt[i] is None else str(amt[i]),
                     str(sum(mem, D(0))) if mem else None,
                     str(max(mem)) if mem else None))
    assert rows == want


def test_utf8_partition_key_expression_input_and_pass_through(ctx, reg):
    rng = np.random.default_rng(8)
    n = 150
    names = ["", "a", "ab", "b", None]
    s = [names[int(v)] for v in rng.integers(0, 5, size=n)]
    o = [int(v) for v in rng.permutation(n)]
    x = [None if z else int(v) for v, z in
         zip(rng.integers(-1000, 1000, size=n), rng.random(n) < 0.1)]
    note = [f"row-{i}" for i in range(n)]
    t = reg("wutf", pa.table({"s": pa.array(s, pa.string()),
                              "o": pa.array(o, pa.int64()),
                              "x": dec_array(x, 15, 2),
                              "note": pa.array(note, pa.string())}))
    schema, rows = run_window(
        t, "wutf", ["s"], [{"col": "o"}],
        [{"fn": "sum", "as": "w",
          "expr": {"mul": [{"col": "x"}, {"col": "x"}]},
          "frame": {"units": "rows", "start": {"preceding": 1},
                    "end": {"following": 1}}},
         {"fn": "count", "as": "c",
          "frame": {"units": "range", "start": "unbounded",
                    "end": "unbounded"}}])
    assert [f["name"] for f in schema] == ["s", "o", "x", "note", "w", "c"]
    assert schema[4]["scale"] == 4 and schema[4]["precision"] == 38
    order = sorted(range(n), key=lambda i: (sort_key(
        None if s[i] is None else 0, False, False),
        (s[i] or "").encode(), o[i]))
    want = []
    for pos, i in enumerate(order):
        part = [j for j in order if s[j] == s[i]]
        at = part.index(i)
        mem = [x[j] ** 2 for j in part[max(0, at - 1):at + 2]
               if x[j] is not None]
        want.append((s[i], o[i], None if x[i] is None else str(x[i]), note[i],
                     str(sum(mem)) if mem else None, len(part)))
    assert rows == want


PW_CASES = [("ASC NULLS LAST", (5, "p"), (5, "f")),
            ("ASC NULLS LAST", (5, "p"), (0, "c")),
            ("ASC NULLS LAST", (0, "c"), (5, "f")),
            ("ASC NULLS LAST", (0, "c"), (0, "c")),
            ("ASC NULLS FIRST", (5, "p"), (5, "f")),
            ("ASC NULLS FIRST", (0, "c"), (0, "c")),
            ("DESC NULLS LAST", (5, "p"), (5, "f")),
            ("DESC NULLS FIRST", (5, "p"), (5, "f"))]


def pw_bound(b):
    x, k = b
    return {"p": {"preceding": x}, "f": {"following": x},
            "c": "current_row"}[k]


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("ordering,start,end", PW_CASES)
def test_parallel_window_table(ctx, reg, ordering, start, end, nullable):
    """The table of the reference's client test parallel_window.rs:
    SUM(v) OVER (ORDER BY k <ordering> RANGE BETWEEN <frame>)."""
    ids = list(range(48))
    k = [None if nullable and i % 4 == 3 else i for i in ids]
    v = [10 * i for i in ids]
    name = f"pw{int(nullable)}"
    t = reg(name, pa.table({"id": pa.array(ids, pa.int64()),
                            "k": pa.array(k, pa.int64()),
                            "v": pa.array(v, pa.int64())}))
    desc, nf = ordering.startswith("DESC"), ordering.endswith("FIRST")
    schema, rows = run_window(
        t, name, [], [{"col": "k", "desc": desc, "nulls_first": nf}],
        [{"fn": "sum", "as": "w", "expr": {"col": "v"},
          "frame": {"units": "range", "start": pw_bound(start),
                    "end": pw_bound(end)}}])
    null_total = sum(v[i] for i in ids if k[i] is None)
    want = {}
    for i in ids:
        if k[i] is None:
            want[i] = null_total         # exactly the NULL run's total
            continue
        lo = k[i] - start[0] if not desc else k[i] - end[0]
        hi = k[i] + end[0] if not desc else k[i] + start[0]
        want[i] = sum(v[j] for j in ids
                      if k[j] is not None and lo <= k[j] <= hi)
    assert len(rows) == 48
    assert {r[0]: r[3] for r in rows} == want
    if nullable:
        assert all(r[3] == null_total for r in rows if r[1] is None)
    order = sorted(ids, key=lambda i: (sort_key(k[i], desc, nf), i))
    assert [r[0] for r in rows] == order


def test_reference_unit_vector_as_two_stages(ctx, reg):
    """partitioned_bounded_window_agg.rs's own vector, one stage per input
    partition as the wrapper runs it: sum(v) over (order by v range between
    2.0 preceding and current row)."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["partitions"]) == 2
    for pi, part in enumerate(golden["partitions"]):
        name = f"wgold{pi}"
        t = reg(name, pa.table({"v": pa.array(part["v"], pa.float64())}))
        schema, rows = run_window(
            t, name, [], [{"col": "v"}],
            [{"fn": "sum", "as": "w", "expr": {"col": "v"},
              "frame": {"units": "range", "start": {"preceding": 2.0},
                        "end": "current_row"}}])
        assert schema[-1] == {"name": "w", "dtype": "float64"}
        assert [r[1] for r in rows] == part["sum"]      # exact in binary64


def test_empty_input_keeps_the_full_schema(ctx, reg):
    t = reg("wempty", pa.table({"k": pa.array([1, 2, 3], pa.int64()),
                                "x": dec_array([1, 2, 3], 15, 2)}))
    pre = {"op": "filter",
           "predicates": [{"col": "k", "cmp": "gt", "lo": 100}],
           "input": scan_of(t, "wempty")}
    schema, rows = run_window(
        t, "wempty", ["k"], [],
        [{"fn": "rank", "as": "r"},
         {"fn": "avg", "as": "a", "expr": {"col": "x"},
          "frame": {"units": "rows", "start": "unbounded",
                    "end": "unbounded"}}], pre=pre)
    assert rows == []
    assert [f["name"] for f in schema] == ["k", "x", "r", "a"]
    assert schema[-1]["precision"] == 19 and schema[-1]["scale"] == 6


def test_unsupported_plan_fails_with_the_validation_message(ctx, reg):
    t = reg("wbad", pa.table({"k": pa.array([1, 2], pa.int64())}))
    node = {"op": "window", "partition_by": [], "order_by": [{"col": "k"}],
            "exprs": [{"fn": "min", "as": "m", "expr": {"col": "k"},
                       "frame": {"units": "rows", "start": {"preceding": 1},
                                 "end": "current_row"}}],
            "input": scan_of(t, "wbad")}
    msg = stage.validate_error(_doc(node))
    assert "window" in msg and "'m'" in msg and "1 preceding" in msg
    with pytest.raises(RuntimeError) as e:
        stage.execute(_doc(node))
    assert msg in str(e.value) and f"rc={BG_ERR_UNSUPPORTED}" in str(e.value)


def test_pool_returns_to_its_start(ctx, pool_start):
    """Runs last in this module: every call above gave its temporaries
    back."""
    gc.collect()
    assert ctx.pool_stats()[:2] == pool_start
