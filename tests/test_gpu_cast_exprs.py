"""CAST, Float64 arithmetic and Decimal128 division on the GPU: bg_cast,
bg_project_f64 and bg_div_dec128 at the C ABI, then q14-, q8-, q11- and
q17-shaped stages through one bg_execute_stage call each.  The checker is
plain Python (int, float, decimal); every comparison is bit-exact, Float64
included, because each result is a fixed sequence of correctly rounded
IEEE-754 operations.

Sizes 1/63/64/65/1000 are the word and tail edges of the 64-row validity
walk; each runs with and without a validity bitmap (about 1 row in 5 NULL,
the bitmap exactly ceil(n/8) bytes long).  Only valid rows are compared,
and the NULL rows carry the values that would fail a valid row: a fallible
call must not look at them."""
import ctypes
import decimal
import math
import struct

import numpy as np
import pyarrow as pa
import pytest

from datafusion_ballista_amd import gpu, stage

pytestmark = pytest.mark.gpu

BG_OK, BG_ERR_INVALID, BG_ERR_UNSUPPORTED = 0, -3, -4
SIZES = [1, 63, 64, 65, 1000]
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1
I128_MAX = 2**127 - 1
D = decimal.Decimal
CTX = decimal.Context(prec=400)      # every finite double is exact in it


@pytest.fixture(scope="module")
def ctx():
    c = gpu.GpuStageContext(0)
    yield c
    c.close()


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
# helpers
# ---------------------------------------------------------------------------
def make_valid(n, nulls, seed):
    if not nulls:
        return np.ones(n, dtype=bool)
    return np.random.default_rng(seed).random(n) >= 0.2


def bitmap(valid):
    """bool[n] -> Arrow LSB bitmap of exactly ceil(n/8) bytes."""
    return np.packbits(valid, bitorder="little")


def dec_raw(ints):
    return np.array([[x & M64, (x >> 64) & M64] for x in ints],
                    dtype=np.uint64).reshape(len(ints), 2)


def dec_col(ctx, ints, p, s, valid=None, nulls=False):
    col, _ = ctx.upload_column(dec_raw(ints), gpu.BG_DT_DECIMAL128,
                               validity=bitmap(valid) if nulls else None)
    col.precision, col.scale = p, s
    return col


def num_col(ctx, arr, dt, valid=None, nulls=False):
    col, _ = ctx.upload_column(arr, dt,
                               validity=bitmap(valid) if nulls else None)
    return col


def dec_ints(buf, n):
    raw = buf.download(np.uint64, 2 * n).reshape(n, 2)
    out = []
    for lo, hi in raw.tolist():
        v = lo | (hi << 64)
        out.append(v - (1 << 128) if v >> 127 else v)
    return out


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_bits(values):
    return np.array(values, dtype=np.float64).view(np.uint64)


def fixed_then_random(fixed, n, draw):
    """n values: the fixed edge cases first (all of them once n allows),
    random draws after."""
    vals = list(fixed[:n])
    while len(vals) < n:
        vals.append(draw())
    return vals


def raw_cast(ctx, col, to_dt, p, s, n, out):
    failed = ctypes.c_int64(-1)
    rc = ctx.L.bg_cast(ctypes.byref(col), to_dt, p, s, n, out.ptr,
                       ctypes.byref(failed))
    return rc, failed.value, ctx.L.bg_last_error().decode()


def raw_div(ctx, a, b, mul_pow, n, out):
    failed = ctypes.c_int64(-1)
    rc = ctx.L.bg_div_dec128(ctypes.byref(a), ctypes.byref(b), mul_pow, n,
                             out.ptr, ctypes.byref(failed))
    return rc, failed.value, ctx.L.bg_last_error().decode()


def assert_valid_equal(got, want, valid):
    for i, ok in enumerate(valid):
        if ok:
            assert got[i] == want[i], (i, got[i], want[i])


# ---------------------------------------------------------------------------
# bg_cast -> Float64
# ---------------------------------------------------------------------------
DEC_EDGES = [0, 1, -1, 2**53 + 1, -(2**53 + 1), 2**53 - 1, -(2**53 - 1),
             10**38 - 1, -(10**38 - 1), I64_MAX, I64_MIN,
             # round-to-even ties and their neighbours at 2^64 and 2^100
             (2**53 + 1) << 11, (2**53 + 3) << 11, ((2**53 + 1) << 11) + 1,
             ((2**53 + 1) << 11) - 1, (2**53 + 1) << 47, -((2**53 + 3) << 47),
             2**64, 2**64 - 1, 2**64 + 1]


@pytest.fixture(scope="module")
def dec_values():
    out = {}
    for n in SIZES:
        rng = np.random.default_rng(40 + n)

        def draw():
            mag = int.from_bytes(rng.bytes(15), "little")   # 120 bits
            return -mag if rng.random() < 0.5 else mag
        out[n] = fixed_then_random(DEC_EDGES, n, draw)
    return out


def test_edge_values_are_all_present(dec_values):
    assert len(DEC_EDGES) <= 63
    for n in SIZES[1:]:
        assert dec_values[n][:len(DEC_EDGES)] == DEC_EDGES


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_cast_decimal_to_float64(ctx, dec_values, n, nulls):
    ints = dec_values[n]
    valid = make_valid(n, nulls, 300 + n)
    for s in (0, 2, 15, 22, 38):
        col = dec_col(ctx, ints, 38, s, valid, nulls)
        got = ctx.cast(col, gpu.BG_DT_FLOAT64, n).download(np.uint64, n)
        want = f64_bits([float(x) / float(10**s) for x in ints])
        assert np.array_equal(got[valid], want[valid]), s


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_cast_integers_to_float64_and_int64(ctx, n, nulls):
    rng = np.random.default_rng(50 + n)
    valid = make_valid(n, nulls, 310 + n)
    v64 = fixed_then_random(
        [0, 1, -1, I64_MAX, I64_MIN, 2**53 + 1, -(2**53 + 1), 2**53 - 1,
         -(2**53 - 1), I64_MAX - 512, I64_MIN + 1025], n,
        lambda: int(rng.integers(I64_MIN, I64_MAX, endpoint=True)))
    v32 = fixed_then_random(
        [0, 1, -1, 2**31 - 1, -2**31], n,
        lambda: int(rng.integers(-2**31, 2**31 - 1, endpoint=True)))
    c64 = num_col(ctx, np.array(v64, dtype=np.int64), gpu.BG_DT_INT64, valid,
                  nulls)
    c32 = num_col(ctx, np.array(v32, dtype=np.int32), gpu.BG_DT_INT32, valid,
                  nulls)
    got = ctx.cast(c64, gpu.BG_DT_FLOAT64, n).download(np.uint64, n)
    assert np.array_equal(got[valid],
                          f64_bits([float(x) for x in v64])[valid])
    got = ctx.cast(c32, gpu.BG_DT_FLOAT64, n).download(np.uint64, n)
    assert np.array_equal(got[valid],
                          f64_bits([float(x) for x in v32])[valid])
    got = ctx.cast(c32, gpu.BG_DT_INT64, n).download(np.int64, n)
    assert np.array_equal(got[valid], np.array(v32, dtype=np.int64)[valid])


# ---------------------------------------------------------------------------
# bg_cast Float64 -> Decimal128
# ---------------------------------------------------------------------------
def ref_f64_to_dec(v, p, s):
    """round-half-away(v * 1e<s>) as an int, or None where the cast fails."""
    prod = v * float(10**s)
    if math.isnan(prod) or math.isinf(prod):
        return None
    r = int(D(prod).quantize(D(1), rounding=decimal.ROUND_HALF_UP,
                             context=CTX))
    return r if abs(r) < 10**p else None


F64_EDGES = [0.5, -2.5, 0.125, -0.125, 0.005, 1.005, 2.675, 0.0, -0.0, 1.5,
             -1.5, 0.2 * 25.5, 25.5, 1e-300, -1e-300, 5e-324,
             4503599627370495.5, -4503599627370497.0, 123456.789]
F64_POISON = [float("nan"), float("inf"), float("-inf"), 1e300, -1e300]


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_cast_float64_to_decimal(ctx, n, nulls):
    """Ties round away from zero; in the nulls run every NULL row holds NaN,
    an infinity or a value far out of precision, and the call succeeds."""
    rng = np.random.default_rng(60 + n)
    valid = make_valid(n, nulls, 320 + n)
    vals = fixed_then_random(F64_EDGES, n,
                             lambda: float(rng.uniform(-1e6, 1e6)))
    for i in range(n):
        if not valid[i]:
            vals[i] = F64_POISON[i % len(F64_POISON)]
    col = num_col(ctx, np.array(vals, dtype=np.float64), gpu.BG_DT_FLOAT64,
                  valid, nulls)
    for p, s in ((30, 2), (38, 15), (38, 0)):
        want = [ref_f64_to_dec(v, p, s) if valid[i] else None
                for i, v in enumerate(vals)]
        assert all(w is not None for w, ok in zip(want, valid) if ok)
        out = ctx.alloc(16 * n)
        rc, failed, msg = raw_cast(ctx, col, gpu.BG_DT_DECIMAL128, p, s, n,
                                   out)
        assert (rc, failed) == (BG_OK, 0), msg
        assert_valid_equal(dec_ints(out, n), want, valid)


def test_float64_tie_expectations_are_the_intended_ones():
    assert ref_f64_to_dec(0.5, 10, 0) == 1
    assert ref_f64_to_dec(-2.5, 10, 0) == -3
    assert ref_f64_to_dec(0.125, 10, 2) == 13
    assert ref_f64_to_dec(-0.125, 10, 2) == -13
    # 0.2 * 25.5 is the double 5.1000000000000005: the Float64 detour of
    # q17's threshold is visible in the last digit
    assert ref_f64_to_dec(0.2 * 25.5, 30, 15) == 5100000000000001
    assert ref_f64_to_dec(100.0, 4, 2) is None
    assert ref_f64_to_dec(99.99, 4, 2) == 9999


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_cast_float64_to_decimal_counts_failing_valid_rows(ctx, nulls):
    n = 1000
    rng = np.random.default_rng(61)
    valid = make_valid(n, nulls, 330)
    vals = [float(v) for v in rng.uniform(-99.0, 99.0, size=n)]
    edge = [99.99, -99.99, 99.994, 100.0, -100.0, 99.995, float("nan"),
            float("inf"), float("-inf"), 1e300, 1e25]
    for k, v in enumerate(edge * 3):        # spread over several words
        vals[7 + 29 * k] = v
    col = num_col(ctx, np.array(vals, dtype=np.float64), gpu.BG_DT_FLOAT64,
                  valid, nulls)
    want = [ref_f64_to_dec(v, 4, 2) for v in vals]
    nfail = sum(1 for w, ok in zip(want, valid) if ok and w is None)
    assert nfail >= 10
    out = ctx.alloc(16 * n)
    rc, failed, msg = raw_cast(ctx, col, gpu.BG_DT_DECIMAL128, 4, 2, n, out)
    assert (rc, failed) == (BG_ERR_INVALID, nfail), msg
    assert msg.startswith("cast:") and f"{nfail} of {n} rows" in msg \
        and "Decimal128(4,2)" in msg
    with pytest.raises(RuntimeError, match=f"cast: {nfail} of {n} rows"):
        ctx.cast(col, gpu.BG_DT_DECIMAL128, n, precision=4, scale=2)


# ---------------------------------------------------------------------------
# bg_cast Decimal128 / integers -> Decimal128
# ---------------------------------------------------------------------------
def ref_rescale(x, s1, s2, p2):
    """Python-int decimal-to-decimal cast, None where it overflows p2."""
    if s2 >= s1:
        r = x * 10**(s2 - s1)
    else:
        d = 10**(s1 - s2)
        r = (abs(x) + d // 2) // d
        r = -r if x < 0 else r
    return r if abs(r) < 10**p2 else None


def run_rescale(ctx, ints, p1, s1, p2, s2, valid, nulls, from_dt=None):
    """Cast and compare the valid rows; returns (rc, failed, msg, nfail)."""
    n = len(ints)
    if from_dt is None:
        col = dec_col(ctx, ints, p1, s1, valid, nulls)
    else:
        np_dt = np.int32 if from_dt == gpu.BG_DT_INT32 else np.int64
        col = num_col(ctx, np.array(ints, dtype=np_dt), from_dt, valid, nulls)
    want = [ref_rescale(x, s1, s2, p2) for x in ints]
    nfail = sum(1 for w, ok in zip(want, valid) if ok and w is None)
    out = ctx.alloc(16 * n)
    rc, failed, msg = raw_cast(ctx, col, gpu.BG_DT_DECIMAL128, p2, s2, n, out)
    if nfail == 0:
        assert (rc, failed) == (BG_OK, 0), msg
        assert_valid_equal(dec_ints(out, n), want, valid)
    else:
        assert (rc, failed) == (BG_ERR_INVALID, nfail), msg
        assert f"cast: {nfail} of {n} rows overflow Decimal128({p2},{s2})" \
            in msg
    return nfail


def poison_nulls(ints, valid, poison):
    return [x if ok else poison[i % len(poison)]
            for i, (x, ok) in enumerate(zip(ints, valid))]


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_cast_decimal_scale_up(ctx, n, nulls):
    rng = np.random.default_rng(70 + n)
    valid = make_valid(n, nulls, 340 + n)
    # q17: (15,2) -> (30,15), wide enough for every 15-digit input: the
    # unchecked path; the same values declared (38,2) take the checked one
    v15 = fixed_then_random(
        [0, 1, -1, 10**15 - 1, -(10**15 - 1), 5000, -5000], n,
        lambda: int(rng.integers(-10**15 + 1, 10**15)))
    assert run_rescale(ctx, v15, 15, 2, 30, 15, valid, nulls) == 0
    assert run_rescale(ctx, v15, 38, 2, 30, 15, valid, nulls) == 0
    # q11: (38,4) -> (38,15) fits below 10^27; NULL rows hold overflows
    v27 = fixed_then_random(
        [0, 10**27 - 1, -(10**27 - 1), 1, -1], n,
        lambda: int(rng.integers(-10**18, 10**18)) * 10**8 + 7)
    v27 = poison_nulls(v27, valid, [10**27, -10**27, 10**38 - 1, I128_MAX,
                                    -I128_MAX - 1])
    assert run_rescale(ctx, v27, 38, 4, 38, 15, valid, nulls) == 0


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_cast_decimal_scale_up_counts_overflowing_rows(ctx, nulls):
    n = 1000
    rng = np.random.default_rng(71)
    valid = make_valid(n, nulls, 350)
    vals = [int(v) for v in rng.integers(-10**18, 10**18, size=n)]
    edge = [10**27, -10**27, 10**27 - 1, -(10**27 - 1), 10**38 - 1,
            -(10**38 - 1), I128_MAX, -I128_MAX - 1, 10**27 + 1]
    for k, v in enumerate(edge * 3):
        vals[5 + 31 * k] = v
    nfail = run_rescale(ctx, vals, 38, 4, 38, 15, valid, nulls)
    assert nfail >= 12
    # a shift wider than the target precision: only zero survives
    small = [0, 1, -1, 0, 7]
    assert run_rescale(ctx, small, 38, 0, 3, 3, np.ones(5, dtype=bool),
                       False) == 3
    assert ref_rescale(1, 0, 3, 3) is None and ref_rescale(0, 0, 3, 3) == 0
    # (38,0) -> (2,4): the shift exceeds the precision, zero alone passes
    assert run_rescale(ctx, small, 38, 0, 4, 4, np.ones(5, dtype=bool),
                       False) == 3


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_cast_decimal_scale_down(ctx, n, nulls):
    """(19,6) -> (15,2): exact +-half ties round away from zero; the NULL
    rows hold values that round up into a 16th digit."""
    rng = np.random.default_rng(80 + n)
    valid = make_valid(n, nulls, 360 + n)
    fixed = [0, 5000, -5000, 4999, -4999, 5001, -5001, 15000, -15000, 25000,
             -25000, 1, -1, 9999, 10000, 10**19 - 5001, -(10**19 - 5001),
             123456785000, -123456785000, 123456784999]
    vals = fixed_then_random(fixed, n,
                             lambda: int(rng.integers(-10**18, 10**18)))
    vals = poison_nulls(vals, valid, [10**19 - 5000, -(10**19 - 5000),
                                      10**19 - 1, 10**30])
    assert run_rescale(ctx, vals, 19, 6, 15, 2, valid, nulls) == 0
    # (19,6) -> (38,2) cannot overflow: the unchecked path, same values
    assert run_rescale(ctx, vals, 19, 6, 38, 2, valid, nulls) == 0


def test_cast_decimal_scale_down_counts_overflowing_rows(ctx):
    vals = [10**19 - 5000, -(10**19 - 5000), 10**19 - 5001, 10**19 - 1,
            -(10**19 - 5001), 0, 10**25]
    valid = np.ones(len(vals), dtype=bool)
    assert run_rescale(ctx, vals, 19, 6, 15, 2, valid, False) == 4
    assert ref_rescale(10**19 - 5000, 6, 2, 15) is None      # rounds to 10^15
    assert ref_rescale(10**19 - 5001, 6, 2, 15) == 10**15 - 1
    assert ref_rescale(25000, 6, 2, 15) == 3
    assert ref_rescale(-25000, 6, 2, 15) == -3


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_cast_integers_to_decimal(ctx, n, nulls):
    rng = np.random.default_rng(90 + n)
    valid = make_valid(n, nulls, 370 + n)
    v32 = fixed_then_random(
        [0, 1, -1, 2**31 - 1, -2**31, 10**8 - 1, -(10**8 - 1)], n,
        lambda: int(rng.integers(-2**31, 2**31 - 1, endpoint=True)))
    # (12,2) holds every int32: unchecked
    assert run_rescale(ctx, v32, 10, 0, 12, 2, valid, nulls,
                       gpu.BG_DT_INT32) == 0
    # (10,2) holds |x| < 10^8: checked; NULL rows hold the int32 extremes
    s32 = [x % 10**8 if x >= 0 else -(-x % 10**8) for x in v32]
    s32 = poison_nulls(s32, valid, [2**31 - 1, -2**31, 10**8, -10**8])
    assert run_rescale(ctx, s32, 10, 0, 10, 2, valid, nulls,
                       gpu.BG_DT_INT32) == 0
    v64 = fixed_then_random(
        [0, 1, -1, 10**18 - 1, -(10**18 - 1), 2**53 + 1], n,
        lambda: int(rng.integers(-10**18 + 1, 10**18)))
    v64 = poison_nulls(v64, valid, [I64_MAX, I64_MIN, 10**18, -10**18])
    assert run_rescale(ctx, v64, 19, 0, 20, 2, valid, nulls,
                       gpu.BG_DT_INT64) == 0
    # (38,19) holds every int64: unchecked
    v64 = poison_nulls(v64, valid, [I64_MAX, I64_MIN])
    assert run_rescale(ctx, v64, 19, 0, 38, 19, valid, nulls,
                       gpu.BG_DT_INT64) == 0


def test_cast_integers_to_decimal_counts_overflowing_rows(ctx):
    v64 = [I64_MAX, I64_MIN, 10**18, -10**18, 10**18 - 1, -(10**18 - 1), 0]
    ones = np.ones(len(v64), dtype=bool)
    assert run_rescale(ctx, v64, 19, 0, 20, 2, ones, False,
                       gpu.BG_DT_INT64) == 4
    v32 = [2**31 - 1, -2**31, 10**8, -10**8, 10**8 - 1, 0]
    ones = np.ones(len(v32), dtype=bool)
    assert run_rescale(ctx, v32, 10, 0, 10, 2, ones, False,
                       gpu.BG_DT_INT32) == 4


def test_cast_refusals_allocate_nothing(ctx):
    n = 8
    out = ctx.alloc(16 * n)
    f = num_col(ctx, np.zeros(n, dtype=np.float64), gpu.BG_DT_FLOAT64)
    i64 = num_col(ctx, np.zeros(n, dtype=np.int64), gpu.BG_DT_INT64)
    d32 = num_col(ctx, np.zeros(n, dtype=np.int32), gpu.BG_DT_DATE32)
    u8 = num_col(ctx, np.zeros(n, dtype=np.uint8), gpu.BG_DT_DICT8)
    utf8 = ctx.upload_utf8_column([b"a"] * n)
    dec = dec_col(ctx, [0] * n, 15, 2)
    pairs = [(utf8, gpu.BG_DT_FLOAT64), (f, gpu.BG_DT_INT64),
             (f, gpu.BG_DT_FLOAT64), (d32, gpu.BG_DT_FLOAT64),
             (i64, gpu.BG_DT_INT32), (i64, gpu.BG_DT_INT64),
             (dec, gpu.BG_DT_INT64), (u8, gpu.BG_DT_DECIMAL128),
             (dec, gpu.BG_DT_UTF8)]
    before = ctx.pool_stats()
    for col, to in pairs:
        rc, _, msg = raw_cast(ctx, col, to, 10, 2, n, out)
        assert rc == BG_ERR_UNSUPPORTED, (col.dtype, to, msg)
        assert "bg_cast" in msg
    assert ctx.pool_stats()[:2] == before[:2]
    for p, s in ((0, 0), (39, 0), (10, 11), (10, -1)):
        rc, _, msg = raw_cast(ctx, dec, gpu.BG_DT_DECIMAL128, p, s, n, out)
        assert rc == BG_ERR_INVALID and "precision" in msg
    assert ctx.pool_stats()[:2] == before[:2]


# ---------------------------------------------------------------------------
# bg_project_f64
# ---------------------------------------------------------------------------
F64_OPS = [
    (gpu.BG_F64_MUL, lambda a, b, lit: np.multiply(a, b)),
    (gpu.BG_F64_ADD, lambda a, b, lit: np.add(a, b)),
    (gpu.BG_F64_SUB, lambda a, b, lit: np.subtract(a, b)),
    (gpu.BG_F64_DIV, lambda a, b, lit: np.divide(a, b)),
    (gpu.BG_F64_MUL_LIT, lambda a, b, lit: np.multiply(a, lit)),
    (gpu.BG_F64_ADD_LIT, lambda a, b, lit: np.add(a, lit)),
    (gpu.BG_F64_LIT_SUB, lambda a, b, lit: np.subtract(lit, a)),
    (gpu.BG_F64_DIV_LIT, lambda a, b, lit: np.divide(a, lit)),
    (gpu.BG_F64_LIT_DIV, lambda a, b, lit: np.divide(lit, a)),
]
TINY = 2.2250738585072014e-308          # smallest normal
F64_A = [0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, TINY, TINY / 4, 0.0, -0.0,
         0.1, 0.2, 1e308, 3.0, 1e-200, 7.0, 0.0, 1.0]
F64_B = [0.0, 0.0, 0.0, -0.0, 3.0, 0.5, 0.5, 3.0, -0.0, 5.0,
         0.2, 0.1, 10.0, 1e-320, 1e-200, 3.0, 5e-324, 5e-324]


@pytest.mark.parametrize("n", SIZES)
def test_project_f64_matches_numpy_bitwise(ctx, n):
    """Zero divisors (x/0 = +-inf, 0/0 = NaN), subnormal inputs and results,
    signed zeros; NaN and inf results are compared by their bits too."""
    rng = np.random.default_rng(100 + n)

    def draw():
        return float(rng.standard_normal() * 10.0 ** int(rng.integers(-8, 9)))
    a = np.array(fixed_then_random(F64_A, n, draw), dtype=np.float64)
    b = np.array(fixed_then_random(F64_B, n, draw), dtype=np.float64)
    ca = num_col(ctx, a, gpu.BG_DT_FLOAT64)
    cb = num_col(ctx, b, gpu.BG_DT_FLOAT64)
    for op, fn in F64_OPS:
        lits = [0.2, -7.0, 1e-310]
        if op in (gpu.BG_F64_DIV_LIT, gpu.BG_F64_LIT_DIV):
            lits += [0.0, -0.0]
        for lit in lits if op >= gpu.BG_F64_MUL_LIT else [0.0]:
            with np.errstate(all="ignore"):
                want = fn(a, b, np.float64(lit)).view(np.uint64)
            got = ctx.project_f64(
                op, ca, cb if op <= gpu.BG_F64_DIV else None, lit,
                n).download(np.uint64, n)
            assert np.array_equal(got, want), (op, lit)


def test_project_f64_unaligned_pointers_take_the_scalar_path(ctx):
    n = 65
    a = np.arange(1, n + 2, dtype=np.float64) / 7.0
    buf = ctx.upload(a)
    col = gpu.BgColumn(gpu.BG_DT_FLOAT64, 0, 0, 0, buf.at(8), None, None, n)
    got = ctx.project_f64(gpu.BG_F64_DIV, col, col, 0.0, n).download(
        np.float64, n)
    assert np.array_equal(got, np.ones(n))
    got = ctx.project_f64(gpu.BG_F64_MUL_LIT, col, None, 0.2, n).download(
        np.uint64, n)
    assert np.array_equal(got, (a[1:] * 0.2).view(np.uint64))


def test_project_f64_refusals(ctx):
    f = num_col(ctx, np.zeros(4, dtype=np.float64), gpu.BG_DT_FLOAT64)
    i64 = num_col(ctx, np.zeros(4, dtype=np.int64), gpu.BG_DT_INT64)
    dec = dec_col(ctx, [0] * 4, 15, 2)
    out = ctx.alloc(64)
    L = ctx.L
    for a, b, op in ((i64, f, gpu.BG_F64_MUL), (f, dec, gpu.BG_F64_DIV),
                     (dec, None, gpu.BG_F64_MUL_LIT), (f, None, gpu.BG_F64_ADD),
                     (f, f, 9), (f, f, -1)):
        rc = L.bg_project_f64(op, ctypes.byref(a),
                              ctypes.byref(b) if b is not None else None,
                              1.0, 4, out.ptr)
        assert rc == BG_ERR_INVALID, (op, L.bg_last_error())
        assert b"bg_project_f64" in L.bg_last_error()


# ---------------------------------------------------------------------------
# bg_div_dec128
# ---------------------------------------------------------------------------
def ref_div(a, b, mul_pow):
    """arrow-rs decimal div: truncating i128 division after scale alignment;
    "zero" / "wide" where the row fails."""
    if b == 0:
        return "zero"
    if mul_pow >= 0:
        a *= 10**mul_pow
        if abs(a) > I128_MAX:
            return "wide"
    else:
        b *= 10**(-mul_pow)
        if abs(b) > I128_MAX:
            return "wide"
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_div_dec128(ctx, n, nulls):
    """mul_pow > 0, == 0 and < 0, all four sign combinations (truncation
    toward zero, not floor).  In the nulls run a and b carry DIFFERENT
    bitmaps, and every row NULL on either side has a zero divisor."""
    rng = np.random.default_rng(110 + n)
    va = make_valid(n, nulls, 380 + n)
    vb = make_valid(n, nulls, 390 + n)
    both = va & vb
    a = fixed_then_random(
        [7, -7, 7, -7, 0, 1, -1, 10**30, -(10**30), 999999, -999999], n,
        lambda: int(rng.integers(-10**17, 10**17)))
    b = fixed_then_random(
        [2, 2, -2, -2, 5, 3, 3, 7, 7, 1000, 1000], n,
        lambda: int(rng.integers(1, 10**9)) * (1 if rng.random() < .5 else -1))
    b = [y if ok else 0 for y, ok in zip(b, both)]
    ca = dec_col(ctx, a, 38, 4, va, nulls)
    cb = dec_col(ctx, b, 38, 4, vb, nulls)
    for mul_pow in (4, 0, -3, 8):
        want = [ref_div(x, y, mul_pow) if ok else None
                for x, y, ok in zip(a, b, both)]
        out = ctx.alloc(16 * n)
        rc, failed, msg = raw_div(ctx, ca, cb, mul_pow, n, out)
        assert (rc, failed) == (BG_OK, 0), msg
        assert_valid_equal(dec_ints(out, n), want, both)


def test_div_truncates_toward_zero_in_the_reference():
    assert [ref_div(7, 2, 0), ref_div(-7, 2, 0), ref_div(7, -2, 0),
            ref_div(-7, -2, 0)] == [3, -3, -3, 3]
    assert ref_div(1, 3, 4) == 3333 and ref_div(-1, 3, 4) == -3333
    assert ref_div(10**6, 3, -3) == 333 and ref_div(-10**6, 3, -3) == -333


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_div_counts_zero_divisors_on_valid_rows(ctx, nulls):
    n = 1000
    rng = np.random.default_rng(120)
    va = make_valid(n, nulls, 400)
    vb = make_valid(n, nulls, 401)
    both = va & vb
    a = [int(v) for v in rng.integers(-10**12, 10**12, size=n)]
    b = [int(v) for v in rng.integers(1, 10**6, size=n)]
    for i in range(0, n, 37):
        b[i] = 0
    nzero = sum(1 for y, ok in zip(b, both) if ok and y == 0)
    assert nzero >= 10
    out = ctx.alloc(16 * n)
    ca, cb = dec_col(ctx, a, 38, 4, va, nulls), dec_col(ctx, b, 38, 4, vb,
                                                        nulls)
    rc, failed, msg = raw_div(ctx, ca, cb, 4, n, out)
    assert (rc, failed) == (BG_ERR_INVALID, nzero), msg
    assert msg == f"div: division by zero in {nzero} rows"
    with pytest.raises(RuntimeError, match="div: division by zero"):
        ctx.div_dec128(ca, cb, 4, n)
    one = [1] * n
    one[64] = 0
    rc, failed, msg = raw_div(ctx, dec_col(ctx, a, 38, 4),
                              dec_col(ctx, one, 38, 4), 0, n, out)
    assert (rc, failed) == (BG_ERR_INVALID, 1)
    assert msg == "div: division by zero in 1 row"


@pytest.mark.parametrize("mul_pow", [4, -4, 38, 0])
def test_div_scaled_operand_overflow_boundary(ctx, mul_pow):
    """The largest operand that still fits i128 after scaling passes, the
    next one fails, on either sign."""
    fit = I128_MAX // 10**abs(mul_pow)
    edge = [fit, -fit, fit + 1, -(fit + 1), fit - 1, 1]
    other = [3, -3, 3, 3, 7, 1]
    if mul_pow == 0:
        edge = [fit, -fit, -(fit + 1), fit - 1, 1]     # fit + 1 is not i128
        other = [3, -3, 3, 7, 1]
    n = len(edge)
    a, b = (edge, other) if mul_pow >= 0 else (other, edge)
    want = [ref_div(x, y, mul_pow) for x, y in zip(a, b)]
    nwide = want.count("wide")
    assert nwide == (2 if mul_pow else 1)
    out = ctx.alloc(16 * n)
    ca, cb = dec_col(ctx, a, 38, 0), dec_col(ctx, b, 38, 0)
    rc, failed, msg = raw_div(ctx, ca, cb, mul_pow, n, out)
    assert (rc, failed) == (BG_ERR_INVALID, nwide), msg
    assert "overflows i128" in msg and "zero" not in msg
    # the same rows minus the overflowing ones pass
    keep = [i for i, w in enumerate(want) if w != "wide"]
    ca = dec_col(ctx, [a[i] for i in keep], 38, 0)
    cb = dec_col(ctx, [b[i] for i in keep], 38, 0)
    rc, failed, msg = raw_div(ctx, ca, cb, mul_pow, len(keep), out)
    assert (rc, failed) == (BG_OK, 0), msg
    assert dec_ints(out, len(keep)) == [want[i] for i in keep]


def test_div_refusals(ctx):
    dec = dec_col(ctx, [1] * 4, 38, 4)
    i64 = num_col(ctx, np.ones(4, dtype=np.int64), gpu.BG_DT_INT64)
    out = ctx.alloc(64)
    for a, b, mp in ((dec, i64, 0), (i64, dec, 0), (dec, dec, 39),
                     (dec, dec, -39)):
        rc, _, msg = raw_div(ctx, a, b, mp, 4, out)
        assert rc == BG_ERR_INVALID and "bg_div_dec128" in msg


# ---------------------------------------------------------------------------
# plan-driven stages
# ---------------------------------------------------------------------------
def _doc(plan):
    return {"job_id": "ce", "stage_id": 1, "task_id": 0,
            "work_dir": "/tmp/cast_exprs", "plan": plan}


def scan_of(table, name):
    return {"op": "scan", "schema": stage.schema_json(table.schema),
            "source": {"kind": "device", "table": name}}


def dec_array(unscaled, p, s, mask=None):
    vals = [None if mask is not None and mask[i]
            else D(int(v)).scaleb(-s, context=CTX)
            for i, v in enumerate(unscaled)]
    return pa.array(vals, type=pa.decimal128(p, s))


def cast(arg, dtype, p=None, s=None):
    to = {"dtype": dtype}
    if p is not None:
        to.update(precision=p, scale=s)
    return {"cast": {"arg": arg, "to": to}}


def col(name):
    return {"col": name}


def schema_types(res):
    return [(f["dtype"], f.get("precision"), f.get("scale"))
            if f["dtype"] == "decimal128" else (f["dtype"], None, None)
            for f in res["schema"]]


def test_stage_q14_final_projection(ctx, reg):
    """q14.txt:22: 100 * CAST(sum(..) AS Float64) / CAST(sum(..) AS
    Float64) over a 3-row aggregate output."""
    a = [164712983456, 0, -5]
    b = [1003478129951, 7, 3]
    t = reg("ce_q14", pa.table({"promo": dec_array(a, 38, 4),
                                "total": dec_array(b, 38, 4)}))
    res = stage.execute(_doc({"op": "collect", "input": {
        "op": "project", "input": scan_of(t, "ce_q14"), "exprs": [
            {"as": "promo_revenue", "expr": {"div": [
                {"mul": [{"lit_f64": 100}, cast(col("promo"), "float64")]},
                cast(col("total"), "float64")]}}]}}))
    assert schema_types(res) == [("float64", None, None)]
    want = [100.0 * (float(x) / 1e4) / (float(y) / 1e4) for x, y in zip(a, b)]
    assert [bits(r[0]) for r in res["rows"]] == [bits(w) for w in want]


def test_stage_q8_mkt_share(ctx, reg):
    """q8.txt:103: sum(case..) / sum(volume) per o_year, both (38,4): the
    output is decimal128(38,8), truncated."""
    rng = np.random.default_rng(130)
    n = 600
    years = rng.integers(1995, 1997, size=n, endpoint=True).astype(np.int32)
    volume = rng.integers(1, 10**10, size=n)
    brazil = np.where(rng.random(n) < 0.3, volume, 0)
    t = reg("ce_q8", pa.table({"o_year": pa.array(years),
                               "brazil": dec_array(brazil, 38, 4),
                               "volume": dec_array(volume, 38, 4)}))
    res = stage.execute(_doc({"op": "collect", "input": {
        "op": "project", "exprs": [
            {"as": "o_year", "expr": col("o_year")},
            {"as": "mkt_share", "expr": {"div": [col("sb"), col("sv")]}}],
        "input": {
            "op": "hash_aggregate", "mode": "single", "group_by": ["o_year"],
            "aggs": [{"fn": "sum", "as": "sb", "expr": col("brazil")},
                     {"fn": "sum", "as": "sv", "expr": col("volume")}],
            "input": scan_of(t, "ce_q8")}}}))
    assert schema_types(res) == [("int32", None, None),
                                 ("decimal128", 38, 8)]
    want = {}
    for y in (1995, 1996, 1997):
        sb = int(brazil[years == y].sum())
        sv = int(volume[years == y].sum())
        want[y] = sb * 10**8 // sv      # S - s1 + s2 = 8 - 4 + 4
    assert {r[0]: int(r[1]) for r in res["rows"]} == want
    assert len(res["rows"]) == 3 and all(0 < v < 10**8 for v in want.values())


def test_stage_q11_casts(ctx, reg):
    """q11.txt:70: CAST(CAST(sum AS Float64) * 0.0001 AS Decimal128(38,15));
    q11.txt:74: CAST(sum AS Decimal128(38,15))."""
    rng = np.random.default_rng(131)
    n = 200
    sums = [int(v) for v in rng.integers(0, 10**16, size=n)]
    sums[:4] = [0, 1, 10**16, 123456789012345]
    mask = rng.random(n) < 0.1
    t = reg("ce_q11", pa.table({"value": dec_array(sums, 25, 2, mask)}))
    res = stage.execute(_doc({"op": "collect", "input": {
        "op": "project", "input": scan_of(t, "ce_q11"), "exprs": [
            {"as": "threshold", "expr": cast(
                {"mul": [cast(col("value"), "float64"), {"lit_f64": 0.0001}]},
                "decimal128", 38, 15)},
            {"as": "value", "expr": cast(col("value"), "decimal128", 38,
                                         15)}]}}))
    assert schema_types(res) == [("decimal128", 38, 15)] * 2
    assert len(res["rows"]) == n
    for x, m, r in zip(sums, mask, res["rows"]):
        if m:
            assert r == [None, None]
            continue
        thr = ref_f64_to_dec((float(x) / 1e2) * 0.0001, 38, 15)
        assert [int(r[0]), int(r[1])] == [thr, x * 10**13]


def test_stage_q17_shape(ctx, reg):
    """q17 stage 4: lineitem JOIN part, then LeftSemi against the per-part
    threshold CAST(0.2 * CAST(avg AS Float64) AS Decimal128(30,15)) with
    filter CAST(l_quantity AS Decimal128(30,15)) < threshold, then
    sum(l_extendedprice)."""
    rng = np.random.default_rng(132)
    n, nparts, nkeys = 2000, 50, 80
    lkey = rng.integers(0, nkeys, size=n).astype(np.int64)
    qty = rng.integers(100, 5100, size=n)             # 1.00 .. 50.99
    qmask = rng.random(n) < 0.05
    price = rng.integers(90000, 10_000_000, size=n)
    parts = np.sort(rng.choice(nkeys, size=nparts, replace=False)).astype(
        np.int64)
    avg = rng.integers(5_000_000, 45_000_000, size=nkeys)   # (19,6)
    avg[:3] = [25_500_000, 10_000_000, 12_345_678]
    li = reg("ce_q17_li", pa.table({
        "l_partkey": pa.array(lkey),
        "l_quantity": dec_array(qty, 15, 2, qmask),
        "l_extendedprice": dec_array(price, 15, 2)}))
    pt = reg("ce_q17_part", pa.table({"p_partkey": pa.array(parts)}))
    av = reg("ce_q17_avg", pa.table({
        "l_partkey": pa.array(np.arange(nkeys, dtype=np.int64)),
        "avg_qty": dec_array(avg, 19, 6)}))
    joined = {"op": "hash_join", "join_type": "inner",
              "build": scan_of(pt, "ce_q17_part"),
              "probe": scan_of(li, "ce_q17_li"),
              "build_keys": ["p_partkey"], "probe_keys": ["l_partkey"],
              "output": [{"side": "probe", "col": "l_quantity"},
                         {"side": "probe", "col": "l_extendedprice"},
                         {"side": "build", "col": "p_partkey"}]}
    left = {"op": "project", "input": joined, "exprs": [
        {"as": "q30", "expr": cast(col("l_quantity"), "decimal128", 30, 15)},
        {"as": "l_extendedprice", "expr": col("l_extendedprice")},
        {"as": "p_partkey", "expr": col("p_partkey")}]}
    right = {"op": "project", "input": scan_of(av, "ce_q17_avg"), "exprs": [
        {"as": "thr", "expr": cast(
            {"mul": [{"lit_f64": 0.2}, cast(col("avg_qty"), "float64")]},
            "decimal128", 30, 15)},
        {"as": "l_partkey", "expr": col("l_partkey")}]}
    res = stage.execute(_doc({"op": "collect", "input": {
        "op": "hash_aggregate", "mode": "single", "group_by": [],
        "aggs": [{"fn": "sum", "as": "s", "expr": col("l_extendedprice")},
                 {"fn": "count", "as": "c"}],
        "input": {"op": "hash_join", "join_type": "semi_build",
                  "build": left, "probe": right,
                  "build_keys": ["p_partkey"], "probe_keys": ["l_partkey"],
                  "filter": {"any": [{"cross": [
                      {"build": "q30", "cmp": "lt", "probe": "thr"}]}]},
                  "output": [{"side": "build",
                              "col": "l_extendedprice"}]}}}))
    thr = [ref_f64_to_dec(0.2 * (float(int(a)) / 1e6), 30, 15) for a in avg]
    assert thr[0] == 5100000000000001     # 0.2 * 25.5 in binary64
    in_part = set(parts.tolist())
    total = cnt = 0
    for k, q, m, p in zip(lkey.tolist(), qty.tolist(), qmask.tolist(),
                          price.tolist()):
        if k in in_part and not m and q * 10**13 < thr[k]:
            total += p
            cnt += 1
    assert 50 < cnt < n // 2
    assert (int(res["rows"][0][0]), res["rows"][0][1]) == (total, cnt)


def two_nullable_table(n, seed, zero_on_valid_row):
    rng = np.random.default_rng(seed)
    a = rng.integers(-10**12, 10**12, size=n)
    b = rng.integers(1, 10**6, size=n)
    am, bm = rng.random(n) < 0.2, rng.random(n) < 0.2
    b[am | bm] = 0                       # zero divisors under every NULL row
    assert (am & ~bm).any() and (bm & ~am).any() and (am & bm).any()
    if zero_on_valid_row:
        b[np.flatnonzero(~am & ~bm)[5]] = 0
    return a, b, am, bm


def div_plan(t, name):
    return _doc({"op": "collect", "input": {
        "op": "project", "input": scan_of(t, name), "exprs": [
            {"as": "r", "expr": {"div": [col("a"), col("b")], "scale": 6}}]}})


def test_stage_div_of_two_nullable_inputs(ctx, reg):
    n = 500
    a, b, am, bm = two_nullable_table(n, 133, False)
    t = reg("ce_div2", pa.table({"a": dec_array(a, 38, 4, am),
                                 "b": dec_array(b, 38, 2, bm)}))
    res = stage.execute(div_plan(t, "ce_div2"))
    assert schema_types(res) == [("decimal128", 38, 6)]
    got = [r[0] for r in res["rows"]]
    assert [g is None for g in got] == (am | bm).tolist()
    for g, x, y, null in zip(got, a.tolist(), b.tolist(), (am | bm).tolist()):
        if not null:
            assert int(g) == ref_div(x, y, 6 - 4 + 2)


def test_stage_div_by_zero_raises_and_releases(ctx, reg):
    n = 500
    a, b, am, bm = two_nullable_table(n, 134, True)
    t = reg("ce_div0", pa.table({"a": dec_array(a, 38, 4, am),
                                 "b": dec_array(b, 38, 2, bm)}))
    before = ctx.pool_stats()
    with pytest.raises(RuntimeError, match="div: division by zero in 1 row"):
        stage.execute(div_plan(t, "ce_div0"))
    assert ctx.pool_stats()[:2] == before[:2]
