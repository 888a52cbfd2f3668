"""Scalar expressions on the GPU: bg_date_part, bg_substr,
bg_eval_compare_cols and bg_eval_in_utf8 at the C ABI, then q12-, q9- and
q22-shaped stages through one bg_execute_stage call each.  The checker is
pyarrow compute plus a few lines of plain Python; every comparison is exact.

Sizes 1/63/64/65/1000 are the word and tail edges of the ballot kernels and
of the four-rows-per-lane date_part path; each runs with and without a
validity bitmap (about 1 row in 5 NULL).  NULL rows are compared only where
the library defines them: predicates are false, substr emits zero bytes,
date_part's value bytes are unspecified (skipped)."""
import ctypes
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from datafusion_ballista_amd import gpu, stage

pytestmark = pytest.mark.gpu

BG_OK, BG_ERR_INVALID, BG_ERR_UNSUPPORTED = 0, -3, -4
SIZES = [1, 63, 64, 65, 1000]
I64 = ctypes.c_int64

DAY_LO, DAY_HI = -719162, 2932896          # 0001-01-01 .. 9999-12-31
FIXED_DAYS = [-719162, -25509, -25508, -1, 0, 3, 10956, 11016, 11017,
              2932896]
PARTS = {
    gpu.BG_DATE_PART_YEAR: pc.year,
    gpu.BG_DATE_PART_QUARTER: pc.quarter,
    gpu.BG_DATE_PART_MONTH: pc.month,
    gpu.BG_DATE_PART_DAY: pc.day,
    gpu.BG_DATE_PART_DOY: pc.day_of_year,
    gpu.BG_DATE_PART_DOW: lambda a: pc.day_of_week(
        a, count_from_zero=True, week_start=7),
}


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


def bitmap_bytes(bits):
    """bool[n] -> Arrow LSB bitmap, whole words plus one spare."""
    n = len(bits)
    out = np.zeros((n + 63) // 64 * 8 + 8, dtype=np.uint8)
    out[:(n + 7) // 8] = np.packbits(bits, bitorder="little")
    return out


def make_valid(n, nulls, seed):
    if not nulls:
        return np.ones(n, dtype=bool)
    return np.random.default_rng(seed).random(n) >= 0.2


def start_mask(n, seed):
    """A starting mask that is not all ones: about half the bits, whole
    zero words where there is more than one word, and every bit at or
    beyond n SET, so a kernel that leaves the tail alone is caught."""
    rng = np.random.default_rng(seed)
    nwords = (n + 63) // 64
    bits = rng.random(nwords * 64) < 0.5
    bits[0] = True
    for w in range(1, nwords, 3):
        bits[w * 64:(w + 1) * 64] = False
    bits[n:] = True
    return bits


def run_mask(ctx, n, start_bits, call):
    """Upload the start mask, run call(mask buffer), return bool[nwords*64]."""
    nwords = (n + 63) // 64
    raw = np.zeros(nwords * 8 + 8, dtype=np.uint8)
    raw[:nwords * 8] = np.packbits(start_bits, bitorder="little")
    mask = ctx.upload(raw)
    call(mask)
    ctx.synchronize()
    got = mask.download(np.uint8, nwords * 8)
    return np.unpackbits(got, bitorder="little").astype(bool)


def check_mask(got, start_bits, expected, n):
    want = np.zeros(len(start_bits), dtype=bool)
    want[:n] = start_bits[:n] & expected
    assert np.array_equal(got, want)     # includes: bits >= n are 0


# ---------------------------------------------------------------------------
# bg_date_part
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def days_by_size():
    rng = np.random.default_rng(11)
    out = {}
    for n in SIZES:
        d = rng.integers(DAY_LO, DAY_HI + 1, size=n).astype(np.int32)
        k = min(n, len(FIXED_DAYS))
        d[:k] = FIXED_DAYS[:k]
        arr = pa.array(d, type=pa.int32()).cast(pa.date32())
        want = {p: np.asarray(fn(arr).cast(pa.int32())) for p, fn in
                PARTS.items()}
        out[n] = (d, want)
    return out


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_date_part_matches_pyarrow(ctx, days_by_size, n, nulls):
    days, want = days_by_size[n]
    valid = make_valid(n, nulls, 100 + n)
    col, _ = ctx.upload_column(days, gpu.BG_DT_DATE32,
                               validity=bitmap_bytes(valid) if nulls else None)
    for part in PARTS:
        got = ctx.date_part(col, part, n).download(np.int32, n)
        assert np.array_equal(got[valid], want[part][valid]), part


def test_date_part_fixed_dates(ctx):
    """The calendar edges: 0001-01-01, 1900-02-28/03-01 (no leap day),
    1969-12-31/1970-01-01, the first Sunday, 1999-12-31, 2000-02-29/03-01,
    9999-12-31."""
    days = np.array(FIXED_DAYS, dtype=np.int32)
    n = len(days)
    col, _ = ctx.upload_column(days, gpu.BG_DT_DATE32)
    want = {
        gpu.BG_DATE_PART_YEAR:
            [1, 1900, 1900, 1969, 1970, 1970, 1999, 2000, 2000, 9999],
        gpu.BG_DATE_PART_QUARTER: [1, 1, 1, 4, 1, 1, 4, 1, 1, 4],
        gpu.BG_DATE_PART_MONTH: [1, 2, 3, 12, 1, 1, 12, 2, 3, 12],
        gpu.BG_DATE_PART_DAY: [1, 28, 1, 31, 1, 4, 31, 29, 1, 31],
        gpu.BG_DATE_PART_DOY: [1, 59, 60, 365, 1, 4, 365, 60, 61, 365],
        gpu.BG_DATE_PART_DOW: [1, 3, 4, 3, 4, 0, 5, 2, 3, 5],
    }
    arr = pa.array(days, type=pa.int32()).cast(pa.date32())
    for part, fn in PARTS.items():
        assert fn(arr).to_pylist() == want[part]
        got = ctx.date_part(col, part, n).download(np.int32, n)
        assert got.tolist() == want[part], part


def _civil(z):
    """Proleptic-Gregorian (year, month, day, doy, dow) in Python ints."""
    z2 = z + 719468
    era, doe = divmod(z2, 146097)
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = mp + 3 if mp < 10 else mp - 9
    y = yoe + era * 400 + (1 if m <= 2 else 0)
    leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
    cum = [0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334]
    jdoy = cum[m - 1] + d + (1 if leap and m > 2 else 0)
    return y, (m + 2) // 3, m, d, jdoy, (z + 4) % 7


def test_date_part_every_int32_is_defined(ctx):
    """Beyond pyarrow's calendar: the int32 extremes and the era seam of
    the 32-bit chain, against floor-division civil-from-days in Python
    ints; through an unaligned pointer too (the all-scalar path)."""
    lo = -2**31
    days = np.array([lo, lo + 1, lo + 14861, lo + 14862, lo + 14863,
                     -146097 - 719468, -719468 - 1, -719468, -719163,
                     2932897, 2**31 - 2, 2**31 - 1, 0], dtype=np.int32)
    n = len(days)
    buf = ctx.upload(np.concatenate([np.zeros(1, np.int32), days]))
    whole, _ = ctx.upload_column(days, gpu.BG_DT_DATE32)
    shifted = gpu.BgColumn(gpu.BG_DT_DATE32, 0, 0, 0, buf.at(4), None, None,
                           n)
    order = [gpu.BG_DATE_PART_YEAR, gpu.BG_DATE_PART_QUARTER,
             gpu.BG_DATE_PART_MONTH, gpu.BG_DATE_PART_DAY,
             gpu.BG_DATE_PART_DOY, gpu.BG_DATE_PART_DOW]
    want = [_civil(int(z)) for z in days]
    for col in (whole, shifted):
        for k, part in enumerate(order):
            got = ctx.date_part(col, part, n).download(np.int32, n)
            assert got.tolist() == [w[k] for w in want], part


def test_date_part_refusals(ctx):
    days = np.arange(8, dtype=np.int32)
    dcol, _ = ctx.upload_column(days, gpu.BG_DT_DATE32)
    icol, _ = ctx.upload_column(days, gpu.BG_DT_INT32)
    out = ctx.alloc(64)
    L = ctx.L
    for part in (-1, 6, 99):
        assert L.bg_date_part(ctypes.byref(dcol), part, 8, out.ptr) == \
            BG_ERR_UNSUPPORTED
    assert L.bg_date_part(ctypes.byref(icol), 0, 8, out.ptr) == BG_ERR_INVALID
    assert b"Date32" in L.bg_last_error()


# ---------------------------------------------------------------------------
# bg_substr
# ---------------------------------------------------------------------------
POOL = ["", "a", "13-555", "héllo𝄞x", "日本語テキスト", "𝄞𝄞", "xé",
        "0123456789abcdef", "é", "ab€cd"]
SUBSTR_ARGS = [(1, 2), (2, 4), (0, 2), (-1, 3), (-5, 2), (4, 2), (2, None),
               (3, 0), (1, 10**9)]


def py_substr(s, start, count):
    cps = list(s)
    ln = len(cps)
    lo = start - 1
    hi = ln if count is None else lo + count
    lo, hi = min(max(lo, 0), ln), min(max(hi, 0), ln)
    return "".join(cps[lo:hi]) if hi > lo else ""


def strings_for(n, seed):
    rng = np.random.default_rng(seed)
    return [POOL[i % len(POOL)] if i < 2 * len(POOL)
            else POOL[int(rng.integers(len(POOL)))] * int(rng.integers(1, 3))
            for i in range(n)]


def utf8_col(ctx, strs, valid=None):
    col = ctx.upload_utf8_column([s.encode() for s in strs])
    if valid is not None:
        vbuf = ctx.upload(bitmap_bytes(valid))
        col.d_validity = vbuf.ptr
        col._keep = col._keep + (vbuf,)
    return col


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_substr_matches_code_point_rule(ctx, n, nulls):
    strs = strings_for(n, 200 + n)
    valid = make_valid(n, nulls, 300 + n)
    col = utf8_col(ctx, strs, valid if nulls else None)
    for start, count in SUBSTR_ARGS:
        want = [py_substr(s, start, count).encode() if v else b""
                for s, v in zip(strs, valid)]
        want_offs = np.concatenate(
            [[0], np.cumsum([len(w) for w in want])]).astype(np.int32)
        # the sizing call alone
        sized = I64(-1)
        scratch = ctx.alloc(4 * (n + 1))
        has, cnt = (0, 0) if count is None else (1, count)
        assert ctx.L.bg_substr(ctypes.byref(col), start, has, cnt, n,
                               scratch.ptr, None, 0,
                               ctypes.byref(sized)) == BG_OK
        offs, data, total = ctx.substr(col, start, count, n)
        assert sized.value == total == int(want_offs[-1]), (start, count)
        assert np.array_equal(offs.download(np.int32, n + 1), want_offs)
        assert bytes(data.download(np.uint8, total)) == b"".join(want)
        if (start, count) == (3, 0):
            assert total == 0


def test_substr_refusals(ctx):
    col = utf8_col(ctx, ["abc", "de"])
    icol, _ = ctx.upload_column(np.arange(2, dtype=np.int32), gpu.BG_DT_INT32)
    offs = ctx.alloc(16)
    total = I64()
    L = ctx.L
    assert L.bg_substr(ctypes.byref(col), 1, 1, -1, 2, offs.ptr, None, 0,
                       ctypes.byref(total)) == BG_ERR_INVALID
    assert b"negative substring length not allowed" in L.bg_last_error()
    assert L.bg_substr(ctypes.byref(icol), 1, 1, 2, 2, offs.ptr, None, 0,
                       ctypes.byref(total)) == BG_ERR_INVALID
    # a negative count is only looked at when has_count is set
    assert L.bg_substr(ctypes.byref(col), 2, 0, -1, 2, offs.ptr, None, 0,
                       ctypes.byref(total)) == BG_OK
    assert total.value == 3


# ---------------------------------------------------------------------------
# bg_eval_compare_cols
# ---------------------------------------------------------------------------
CMPS = {gpu.BG_CMP_LT: lambda a, b: a < b, gpu.BG_CMP_LE: lambda a, b: a <= b,
        gpu.BG_CMP_GT: lambda a, b: a > b, gpu.BG_CMP_GE: lambda a, b: a >= b,
        gpu.BG_CMP_EQ: lambda a, b: a == b, gpu.BG_CMP_NE: lambda a, b: a != b}

_HI = 1 << 64
DEC_EDGES = [  # (a, b) as Python ints
    (-1, 0), (0, -1), (-5, -5), (-(1 << 100), 1 << 100),
    # differ only in the high word; low word >= 2^63
    ((3 << 64) | (1 << 63), (4 << 64) | (1 << 63)),
    ((-2 * _HI) | ((1 << 63) + 7), (-3 * _HI) | ((1 << 63) + 7)),
    # differ only in the low word, on both sides of 2^63
    ((5 << 64) | ((1 << 63) + 1), (5 << 64) | ((1 << 63) - 1)),
    ((-7 * _HI) | (_HI - 1), (-7 * _HI) | (1 << 63)),
    ((1 << 63), (1 << 63) - 1), (-(1 << 63), (1 << 63)),
]


def dec_bytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(16, "little", signed=True)
                                  for v in vals), dtype=np.uint8)


def compare_inputs(kind, n, seed):
    """-> (BG dtype, upload array a, upload array b, python-comparable a, b);
    small domains so that equal pairs are common."""
    rng = np.random.default_rng(seed)
    if kind == "decimal128":
        pool = [v for pair in DEC_EDGES for v in pair]
        a = [DEC_EDGES[i][0] if i < len(DEC_EDGES)
             else pool[int(rng.integers(len(pool)))] for i in range(n)]
        b = [DEC_EDGES[i][1] if i < len(DEC_EDGES)
             else pool[int(rng.integers(len(pool)))] for i in range(n)]
        return (gpu.BG_DT_DECIMAL128, dec_bytes(a), dec_bytes(b),
                np.array(a, dtype=object), np.array(b, dtype=object))
    np_t, dt, lo, hi = {
        "int32": (np.int32, gpu.BG_DT_INT32, -2**31, 2**31),
        "date32": (np.int32, gpu.BG_DT_DATE32, 8000, 8012),
        "int64": (np.int64, gpu.BG_DT_INT64, -2**63, 2**63),
        "dict8": (np.uint8, gpu.BG_DT_DICT8, 0, 256),
    }[kind]
    a = rng.integers(lo, hi, size=n, dtype=np_t)
    b = rng.integers(lo, hi, size=n, dtype=np_t)
    same = rng.random(n) < 0.3
    b[same] = a[same]
    if n > 2 and kind in ("int32", "int64"):  # sign edges
        a[0], b[0] = lo, hi - 1
        a[1], b[1] = -1, 0
    return dt, a, b, a, b


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["int32", "date32", "int64", "dict8",
                                  "decimal128"])
def test_compare_cols(ctx, kind, n, nulls):
    dt, ua, ub, pa_, pb = compare_inputs(kind, n, 400 + n)
    va, vb = make_valid(n, nulls, 500 + n), make_valid(n, nulls, 600 + n)
    ca, _ = ctx.upload_column(ua, dt, validity=bitmap_bytes(va) if nulls
                              else None)
    cb, _ = ctx.upload_column(ub, dt, validity=bitmap_bytes(vb) if nulls
                              else None)
    if kind == "decimal128":
        ca.precision = cb.precision = 38
        ca.scale = cb.scale = 2
    start = start_mask(n, 700 + n)
    for cmp, fn in CMPS.items():
        expected = np.asarray(fn(pa_, pb), dtype=bool) & va & vb
        got = run_mask(ctx, n, start,
                       lambda m: ctx.compare_cols(ca, cb, cmp, n, m))
        check_mask(got, start, expected, n)


def test_compare_cols_all_zero_mask_stays_zero(ctx):
    n = 300
    a, _ = ctx.upload_column(np.arange(n, dtype=np.int32), gpu.BG_DT_DATE32)
    start = np.zeros((n + 63) // 64 * 64, dtype=bool)
    got = run_mask(ctx, n, start,
                   lambda m: ctx.compare_cols(a, a, gpu.BG_CMP_EQ, n, m))
    assert not got.any()


def test_compare_cols_refusals(ctx):
    n = 8
    i32, _ = ctx.upload_column(np.arange(n, dtype=np.int32), gpu.BG_DT_INT32)
    d32, _ = ctx.upload_column(np.arange(n, dtype=np.int32), gpu.BG_DT_DATE32)
    f64, _ = ctx.upload_column(np.arange(n, dtype=np.float64))
    dec2, _ = ctx.upload_column(dec_bytes(range(n)), gpu.BG_DT_DECIMAL128)
    dec4, _ = ctx.upload_column(dec_bytes(range(n)), gpu.BG_DT_DECIMAL128)
    dec2.scale, dec4.scale = 2, 4
    s = utf8_col(ctx, ["a"] * n)
    mask = ctx.upload(np.full(16, 0xFF, dtype=np.uint8))
    L = ctx.L

    def rc(a, b, cmp=gpu.BG_CMP_LT):
        return L.bg_eval_compare_cols(ctypes.byref(a), ctypes.byref(b), cmp,
                                      n, mask.ptr)

    assert rc(i32, d32) == BG_ERR_INVALID
    assert b"dtype mismatch" in L.bg_last_error()
    assert rc(dec2, dec4) == BG_ERR_INVALID
    assert b"scale" in L.bg_last_error()
    assert rc(f64, f64) == BG_ERR_UNSUPPORTED
    assert rc(s, s) == BG_ERR_UNSUPPORTED
    assert rc(i32, i32, 6) == BG_ERR_INVALID
    assert rc(i32, i32, -1) == BG_ERR_INVALID
    ctx.synchronize()
    assert mask.download(np.uint8, 8).tolist() == [0xFF] * 8  # untouched


# ---------------------------------------------------------------------------
# bg_eval_in_utf8
# ---------------------------------------------------------------------------
IN_LITERALS = ["13", "31", "23", "29", "30", "18", "17", "13-5", "héllo",
               "x" * 64, "a", "ab", "abc", "𝄞", "日本", "0"]
IN_ROWS = ["13", "1", "13-", "13-5", "13-55", "31", "", "héllo", "héll",
           "héllo𝄞", "x" * 64, "x" * 63, "x" * 65, "abc", "abcd", "𝄞", "日",
           "日本", "00", "0", "17", "71"]


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_in_utf8(ctx, n, nulls):
    rng = np.random.default_rng(800 + n)
    strs = [IN_ROWS[i] if i < len(IN_ROWS)
            else IN_ROWS[int(rng.integers(len(IN_ROWS)))] for i in range(n)]
    valid = make_valid(n, nulls, 900 + n)
    col = utf8_col(ctx, strs, valid if nulls else None)
    start = start_mask(n, 1000 + n)
    for nvals in (1, 7, 16):
        lits = IN_LITERALS[:nvals]
        expected = np.array([s in lits for s in strs], dtype=bool) & valid
        got = run_mask(ctx, n, start, lambda m: ctx.in_utf8(
            col, [v.encode() for v in lits], n, m))
        check_mask(got, start, expected, n)


def test_in_utf8_prefix_cases_are_present():
    """The literal/row lists hold a literal that is a strict prefix of a row
    and a row that is a strict prefix of a literal, for every list size."""
    for nvals in (1, 7, 16):
        lits = IN_LITERALS[:nvals]
        assert any(r != v and r.startswith(v) for r in IN_ROWS for v in lits)
        assert any(r != v and v.startswith(r) and r for r in IN_ROWS
                   for v in lits)


def test_in_utf8_refusals(ctx):
    col = utf8_col(ctx, ["a", "b"])
    icol, _ = ctx.upload_column(np.arange(2, dtype=np.int32), gpu.BG_DT_INT32)
    mask = ctx.upload(np.full(16, 0xFF, dtype=np.uint8))
    for bad in ([], [b"x"] * 17, [b""], [b"y" * 65]):
        with pytest.raises(RuntimeError, match="bg_eval_in_utf8"):
            ctx.in_utf8(col, bad, 2, mask)
    with pytest.raises(RuntimeError, match="Utf8 column required"):
        ctx.in_utf8(icol, [b"a"], 2, mask)


# ---------------------------------------------------------------------------
# plan-driven stages
# ---------------------------------------------------------------------------
def _doc(plan):
    return {"job_id": "se", "stage_id": 1, "task_id": 0,
            "work_dir": "/tmp/scalar_exprs", "plan": plan}


def scan_of(table, name):
    return {"op": "scan", "schema": stage.schema_json(table.schema),
            "source": {"kind": "device", "table": name}}


def dec_array(unscaled, mask=None, scale=2):
    vals = [None if mask is not None and mask[i]
            else decimal.Decimal(int(v)).scaleb(-scale)
            for i, v in enumerate(unscaled)]
    return pa.array(vals, type=pa.decimal128(15, scale))


def unscaled(d, scale):
    return None if d is None else int(d.scaleb(scale))


N_STAGE = 3000


def test_stage_q12_shape(ctx, reg):
    """(mode = MAIL OR mode = SHIP) AND receipt > commit AND ship < commit
    AND receipt in [1994-01-01, 1995-01-01): row set and order."""
    rng = np.random.default_rng(21)
    n = N_STAGE
    base = rng.integers(8700, 9200, size=n).astype(np.int32)
    ship = base + rng.integers(-20, 20, size=n).astype(np.int32)
    commit = base + rng.integers(-20, 20, size=n).astype(np.int32)
    receipt = base + rng.integers(-20, 20, size=n).astype(np.int32)
    t = reg("se_q12", pa.table({
        "l_orderkey": pa.array(np.arange(n, dtype=np.int64)),
        "l_shipmode": pa.array(rng.integers(0, 7, size=n).astype(np.uint8)),
        "l_shipdate": pa.array(ship, type=pa.date32(),
                               mask=rng.random(n) < 0.1),
        "l_commitdate": pa.array(commit, type=pa.date32(),
                                 mask=rng.random(n) < 0.1),
        "l_receiptdate": pa.array(receipt, type=pa.date32(),
                                  mask=rng.random(n) < 0.1),
    }))
    lo, hi = 8766, 9131  # 1994-01-01, 1995-01-01
    rest = [
        {"col": "l_receiptdate", "cmp": "gt", "rhs": {"col": "l_commitdate"}},
        {"col": "l_shipdate", "cmp": "lt", "rhs": {"col": "l_commitdate"}},
        {"col": "l_receiptdate", "cmp": "ge_lt", "lo": lo, "hi": hi}]
    res = stage.execute(_doc({"op": "collect", "input": {
        "op": "filter", "input": scan_of(t, "se_q12"), "any": [
            [{"col": "l_shipmode", "cmp": "eq", "lo": 2}] + rest,
            [{"col": "l_shipmode", "cmp": "eq", "lo": 5}] + rest]}}))
    i32 = pa.int32()
    keep = pc.and_(
        pc.is_in(t["l_shipmode"], value_set=pa.array([2, 5], pa.uint8())),
        pc.and_(pc.greater(t["l_receiptdate"], t["l_commitdate"]),
                pc.and_(pc.less(t["l_shipdate"], t["l_commitdate"]),
                        pc.and_(pc.greater_equal(
                            t["l_receiptdate"].cast(i32), lo),
                            pc.less(t["l_receiptdate"].cast(i32), hi)))))
    want = t.filter(pc.fill_null(keep, False))
    assert 50 < want.num_rows < n
    got = res["rows"]
    assert [r[0] for r in got] == want["l_orderkey"].to_pylist()
    assert [r[1] for r in got] == want["l_shipmode"].to_pylist()
    assert [r[4] for r in got] == want["l_receiptdate"].cast(i32).to_pylist()


def test_stage_q9_shape(ctx, reg):
    """project date_part(year, o_orderdate), price * discount; GROUP BY the
    year (NULL dates form one NULL group); SUM."""
    rng = np.random.default_rng(22)
    n = N_STAGE
    t = reg("se_q9", pa.table({
        "o_orderdate": pa.array(
            rng.integers(8035, 10592, size=n).astype(np.int32),
            type=pa.date32(), mask=rng.random(n) < 0.05),
        "l_extendedprice": dec_array(rng.integers(90000, 10_000_000, size=n)),
        "l_discount": dec_array(rng.integers(0, 11, size=n)),
    }))
    res = stage.execute(_doc({"op": "collect", "input": {
        "op": "hash_aggregate", "mode": "single", "group_by": ["o_year"],
        "aggs": [{"fn": "sum", "as": "amount", "expr": {"col": "amount"}},
                 {"fn": "count", "as": "cnt"}],
        "input": {"op": "project", "input": scan_of(t, "se_q9"), "exprs": [
            {"as": "o_year", "expr": {"date_part": {
                "part": "year", "arg": {"col": "o_orderdate"}}}},
            {"as": "amount", "expr": {"mul": [{"col": "l_extendedprice"},
                                              {"col": "l_discount"}]}}]}}}))
    want_t = pa.table({
        "o_year": pc.year(t["o_orderdate"]).cast(pa.int32()),
        "amount": pc.multiply(t["l_extendedprice"], t["l_discount"]),
    }).group_by("o_year").aggregate([("amount", "sum"), ("amount", "count")])
    want = sorted(((y, unscaled(s, 4), c) for y, s, c in zip(
        want_t["o_year"].to_pylist(), want_t["amount_sum"].to_pylist(),
        want_t["amount_count"].to_pylist())),
        key=lambda r: (r[0] is None, r[0]))
    got = sorted(((r[0], int(r[1]), r[2]) for r in res["rows"]),
                 key=lambda r: (r[0] is None, r[0]))
    assert len(want) == 8 and want[-1][0] is None   # 1992..1998 + NULL
    assert got == want


Q22_CODES = ["13", "31", "23", "29", "30", "18", "17"]


def test_stage_q22_shape(ctx, reg):
    """acctbal > 0 AND substr(phone,1,2) IN (7 codes); project the code as
    cntrycode; GROUP BY it with COUNT and SUM."""
    rng = np.random.default_rng(23)
    n = N_STAGE
    phones = [f"{int(c):02d}-{int(a):03d}-{int(b):03d}-{int(d):04d}"
              for c, a, b, d in zip(rng.integers(10, 35, size=n),
                                    rng.integers(0, 1000, size=n),
                                    rng.integers(0, 1000, size=n),
                                    rng.integers(0, 10000, size=n))]
    pmask = rng.random(n) < 0.05
    t = reg("se_q22", pa.table({
        "c_phone": pa.array([None if m else p for p, m in
                             zip(phones, pmask)], type=pa.string()),
        "c_acctbal": dec_array(rng.integers(-99999, 999999, size=n),
                               mask=rng.random(n) < 0.05),
    }))
    code = {"substr": {"arg": {"col": "c_phone"}, "start": 1, "count": 2}}
    res = stage.execute(_doc({"op": "collect", "input": {
        "op": "hash_aggregate", "mode": "single", "group_by": ["cntrycode"],
        "aggs": [{"fn": "count", "as": "numcust"},
                 {"fn": "sum", "as": "totacctbal",
                  "expr": {"col": "c_acctbal"}}],
        "input": {"op": "project", "exprs": [
            {"as": "cntrycode", "expr": code},
            {"as": "c_acctbal", "expr": {"col": "c_acctbal"}}],
            "input": {"op": "filter", "input": scan_of(t, "se_q22"),
                      "predicates": [
                          {"col": "c_acctbal", "cmp": "gt", "lo": 0},
                          {"expr": code, "in": Q22_CODES}]}}}}))
    codes = pc.utf8_slice_codeunits(t["c_phone"], 0, 2)
    keep = pc.and_(pc.greater(t["c_acctbal"], decimal.Decimal("0.00")),
                   pc.is_in(codes, value_set=pa.array(Q22_CODES)))
    kept = pa.table({"cntrycode": codes, "c_acctbal": t["c_acctbal"]}).filter(
        pc.fill_null(keep, False))
    want_t = kept.group_by("cntrycode").aggregate(
        [("c_acctbal", "count"), ("c_acctbal", "sum")])
    want = sorted(zip(want_t["cntrycode"].to_pylist(),
                      want_t["c_acctbal_count"].to_pylist(),
                      (unscaled(s, 2) for s in
                       want_t["c_acctbal_sum"].to_pylist())))
    got = sorted((r[0], r[1], int(r[2])) for r in res["rows"])
    assert [w[0] for w in want] == sorted(Q22_CODES)
    assert got == want
