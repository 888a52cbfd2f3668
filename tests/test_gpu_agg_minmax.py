"""GPU tests of MIN/MAX over Decimal128, Utf8, Int32 and Date32.

Decimal128 and Utf8 run the row-index accumulators (BG_AGG_OP_MIN_ROW /
MAX_ROW: word 0 of the record is the winning input row + 1), Int32 and
Date32 the 32-bit pair of the order-preserving encoding.  Every value is
checked by exact equality against pyarrow's group_by min/max (Arrow's
orders: signed i128, bytewise unsigned strings), the raw ops against a
Python dict of min/max over int / bytes.

k_hashagg_lds is attempted from n = 65536 rows; below that the global
table runs.  A block of the LDS attempt sees at most 256 rows while the
grid is not capped (n <= 2048 * 256), so its table only overflows when it
holds fewer than 256 slots: that is the 8-aggregate record (128 slots),
which the overflow test therefore uses."""
import ctypes
import decimal

import numpy as np
import pyarrow as pa
import pytest

from datafusion_ballista_amd import gpu, stage

pytestmark = pytest.mark.gpu

BG_ERR_INVALID, BG_ERR_UNSUPPORTED = -3, -4
DEC_MAX = 10**38 - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1


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


# ---- helpers -------------------------------------------------------------

def dec(v, scale):
    """int -> Decimal at `scale`, exact at any width (no context rounding)."""
    return decimal.Decimal((1 if v < 0 else 0,
                            tuple(int(c) for c in str(abs(v))), -scale))


def dec_int(d):
    """Decimal -> its unscaled integer, exact at any width."""
    sign, digits, _ = d.as_tuple()
    v = int("".join(map(str, digits)))
    return -v if sign else v


def dec_array(ints, mask, precision, scale):
    return pa.array([None if m else dec(int(v), scale)
                     for v, m in zip(ints, mask)],
                    type=pa.decimal128(precision, scale))


def str_array(strs, mask):
    return pa.array([None if m else s for s, m in zip(strs, mask)],
                    type=pa.string())


def date_array(days, mask):
    return pa.array(np.asarray(days, dtype=np.int32), mask=np.asarray(mask),
                    type=pa.int32()).cast(pa.date32())


def plain(arr):
    """A pyarrow column as the collect root spells its cells: Decimal128 as
    the unscaled int, Date32 as days, everything else as is."""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    if pa.types.is_decimal(arr.type):
        return [None if d is None else dec_int(d) for d in arr.to_pylist()]
    if pa.types.is_date32(arr.type):
        return arr.cast(pa.int32()).to_pylist()
    return arr.to_pylist()


def got_columns(res):
    """Result JSON -> {name: cells}, Decimal128 strings turned into ints."""
    out = {}
    for c, f in enumerate(res["schema"]):
        cells = [r[c] for r in res["rows"]]
        if f["dtype"] == "decimal128":
            cells = [None if x is None else int(x) for x in cells]
        out[f["name"]] = cells
    return out


def result_table(res):
    """Result JSON -> pyarrow table of the same schema (partial outputs are
    registered again as the final stage's input)."""
    cols = got_columns(res)
    arrays, names = [], []
    for f in res["schema"]:
        cells = cols[f["name"]]
        if f["dtype"] == "decimal128":
            a = pa.array([None if x is None else dec(x, f["scale"])
                          for x in cells],
                         type=pa.decimal128(f["precision"], f["scale"]))
        elif f["dtype"] == "date32":
            a = pa.array(cells, type=pa.int32()).cast(pa.date32())
        elif f["dtype"] == "utf8":
            a = pa.array(cells, type=pa.string())
        else:
            a = pa.array(cells, type={"int64": pa.int64(),
                                      "int32": pa.int32()}[f["dtype"]])
        arrays.append(a)
        names.append(f["name"])
    return pa.table(arrays, names=names)


def scan_of(table, name):
    return {"op": "scan", "schema": stage.schema_json(table.schema),
            "source": {"kind": "device", "table": name}}


def run(plan):
    """Validate, then execute: the two must give the same verdict."""
    doc = {"job_id": "job-mm", "stage_id": 1, "task_id": 0,
           "work_dir": "/tmp/stage-tests",
           "plan": {"op": "collect", "input": plan}}
    assert stage.validate(doc)["ok"] is True
    return stage.execute(doc)


def minmax_aggs(cols, fns=("min", "max")):
    return [{"fn": fn, "as": f"{c}_{fn}", "expr": {"col": c}}
            for c in cols for fn in fns]


def agg_plan(inp, group_by, aggs, mode="single"):
    return {"op": "hash_aggregate", "mode": mode, "group_by": group_by,
            "aggs": aggs, "input": inp}


def want_by_key(t, key, cols, fns=("min", "max")):
    """pyarrow reference: {key: {"c_min": v, ...}} with plain() cells."""
    ref = t.group_by(key).aggregate([(c, fn) for c in cols for fn in fns])
    names = [f"{c}_{fn}" for c in cols for fn in fns]
    data = {nm: plain(ref[nm]) for nm in names}
    return {k: {nm: data[nm][i] for nm in names}
            for i, k in enumerate(ref[key].to_pylist())}


def check_grouped(res, t, key, cols, fns=("min", "max")):
    want = want_by_key(t, key, cols, fns)
    got = got_columns(res)
    assert sorted(got[key]) == sorted(want)
    for i, k in enumerate(got[key]):
        for nm, w in want[k].items():
            assert got[nm][i] == w, (k, nm, got[nm][i], w)
    return got


def check_one_group(res, t, cols, fns=("min", "max")):
    """No group_by: one output row; the reference groups by a constant."""
    ref = t.append_column("one$", pa.array(np.zeros(t.num_rows, np.int64)))
    want = want_by_key(ref, "one$", cols, fns)[0]
    got = got_columns(res)
    assert len(res["rows"]) == 1
    for nm, w in want.items():
        assert got[nm][0] == w, (nm, got[nm][0], w)


def out_dtypes(res):
    return {f["name"]: f for f in res["schema"]}


# pairs that tell a correct i128 compare from a wrong one
DEC_PAIRS = [
    (5 + (3 << 64), 5 + (4 << 64)),      # differ only in the high limb
    (1 << 63, 1),                        # low limb, top bit set on one side
    ((7 << 64) + (1 << 63), (7 << 64) + 1),
    (-(1 << 63), -1),
    (12345, -12345),                     # differ only in sign
    (DEC_MAX, -DEC_MAX),
    (DEC_MAX, DEC_MAX - 1),
    (-DEC_MAX, -DEC_MAX + 1),
]


def edge_decimals(rng, keys):
    """Decimal(38,x) unscaled ints: group p < len(DEC_PAIRS) draws only from
    pair p, every other group from a wide mixture incl. the pair values."""
    pool = [v for p in DEC_PAIRS for v in p]
    out = []
    for k in keys:
        if k < len(DEC_PAIRS):
            out.append(DEC_PAIRS[k][int(rng.integers(0, 2))])
            continue
        kind = int(rng.integers(0, 4))
        if kind == 0:
            out.append(pool[int(rng.integers(0, len(pool)))])
        elif kind == 1:
            out.append(int(rng.integers(-10**6, 10**6)))
        else:
            mag = int(rng.integers(0, 2**62)) * int(rng.integers(0, 2**62))
            out.append(min(mag, DEC_MAX) * (1 if kind == 2 else -1))
    return out


LONG = "abc" * 100  # 300 bytes
STR_PAIRS = [
    ("ab", "abc"),       # a proper prefix is smaller
    ("é", "z"),     # 0xC3 0xA9 > 0x7A only in an unsigned compare
    ("", "a"),
    ("", ""),            # "" alone is a value
    (LONG, LONG + "d"),
    (LONG, "abd"),
]


def edge_strings(rng, keys):
    pool = [s for p in STR_PAIRS for s in p] + ["zz", "a", "Z", "éa"]
    out = []
    for k in keys:
        if k < len(STR_PAIRS):
            out.append(STR_PAIRS[k][int(rng.integers(0, 2))])
        elif rng.random() < 0.5:
            out.append(pool[int(rng.integers(0, len(pool)))])  # duplicates
        else:
            out.append("s%05d" % int(rng.integers(0, 3000)))
    return out


def nulls(rng, n, frac=0.25):
    return rng.random(n) < frac


# ---- 1-3: the global-table path, per dtype ---------------------------------

def test_decimal128_limbs_global_path(ctx, reg):
    rng = np.random.default_rng(101)
    n = 4096
    keys = rng.integers(0, 200, size=n, dtype=np.int64)
    t = pa.table({"k": pa.array(keys),
                  "d": dec_array(edge_decimals(rng, keys), nulls(rng, n),
                                 38, 2)})
    reg("mm1", t)
    res = run(agg_plan(scan_of(t, "mm1"), ["k"], minmax_aggs(["d"])))
    check_grouped(res, t, "k", ["d"])
    for nm in ("d_min", "d_max"):
        f = out_dtypes(res)[nm]
        assert (f["dtype"], f["precision"], f["scale"]) == ("decimal128",
                                                            38, 2)


def test_utf8_global_path(ctx, reg):
    rng = np.random.default_rng(102)
    n = 4096
    keys = rng.integers(0, 200, size=n, dtype=np.int64)
    mask = nulls(rng, n)
    mask[np.flatnonzero(keys == 3)[0]] = False  # group 3: "" and NULLs only
    t = pa.table({"k": pa.array(keys),
                  "s": str_array(edge_strings(rng, keys), mask)})
    reg("mm2", t)
    res = run(agg_plan(scan_of(t, "mm2"), ["k"], minmax_aggs(["s"])))
    got = check_grouped(res, t, "k", ["s"])
    i3 = got["k"].index(3)
    assert got["s_min"][i3] == "" and got["s_max"][i3] == ""
    i1 = got["k"].index(1)  # both present with overwhelming probability
    assert (got["s_min"][i1], got["s_max"][i1]) == ("z", "é")
    assert out_dtypes(res)["s_min"]["dtype"] == "utf8"


def test_int32_and_date32(ctx, reg):
    rng = np.random.default_rng(103)
    n = 4096
    keys = rng.integers(0, 200, size=n, dtype=np.int64)
    edge = np.array([I32_MIN, I32_MAX, -1, 0], dtype=np.int64)

    def values():
        v = rng.integers(-10**5, 10**5, size=n)
        pick = rng.random(n) < 0.3
        v[pick] = edge[rng.integers(0, 4, size=int(pick.sum()))]
        return v.astype(np.int32)

    t = pa.table({"k": pa.array(keys),
                  "i": pa.array(values(), mask=nulls(rng, n)),
                  "dt": date_array(values(), nulls(rng, n))})
    reg("mm3", t)
    res = run(agg_plan(scan_of(t, "mm3"), ["k"], minmax_aggs(["i", "dt"])))
    check_grouped(res, t, "k", ["i", "dt"])
    dts = out_dtypes(res)
    assert [dts[c]["dtype"] for c in ("i_min", "i_max", "dt_min",
                                      "dt_max")] == ["int32", "int32",
                                                     "date32", "date32"]
    got = got_columns(res)
    assert I32_MIN in got["i_min"] and I32_MAX in got["i_max"]
    assert I32_MIN in got["dt_min"] and I32_MAX in got["dt_max"]


# ---- 4-5: the LDS path and its overflow fallback ---------------------------

@pytest.fixture(scope="module")
def big_cols():
    """n = 70000 value columns shared by the LDS tests (25 % NULL each)."""
    rng = np.random.default_rng(104)
    n = 70_000
    k50 = rng.integers(0, 50, size=n, dtype=np.int64)
    return {
        "n": n, "k50": k50,
        "k20k": rng.integers(0, 20_000, size=n, dtype=np.int64),
        "d": dec_array(edge_decimals(rng, k50), nulls(rng, n), 38, 2),
        "s": str_array(edge_strings(rng, k50), nulls(rng, n)),
        "dt": date_array(rng.integers(-40000, 40000, size=n), nulls(rng, n)),
        "v": pa.array(rng.integers(-10**9, 10**9, size=n, dtype=np.int64),
                      mask=nulls(rng, n)),
    }


def test_lds_path_mixed_record(ctx, reg, big_cols):
    b = big_cols
    t = pa.table({"k": pa.array(b["k50"]), "d": b["d"], "s": b["s"],
                  "dt": b["dt"], "v": b["v"]})
    reg("mm4", t)
    aggs = minmax_aggs(["d", "s", "dt"]) + [
        {"fn": "sum", "as": "v_sum", "expr": {"col": "v"}},
        {"fn": "count", "as": "k_count"}]
    res = run(agg_plan(scan_of(t, "mm4"), ["k"], aggs))
    got = check_grouped(res, t, "k", ["d", "s", "dt"])
    ref = t.group_by("k").aggregate([("v", "sum"), ("k", "count")])
    want = {k: (s, c) for k, s, c in zip(ref["k"].to_pylist(),
                                         ref["v_sum"].to_pylist(),
                                         ref["k_count"].to_pylist())}
    for i, k in enumerate(got["k"]):
        assert (got["v_sum"][i], got["k_count"][i]) == want[k]


def test_lds_overflow_fallback(ctx, reg, big_cols):
    """20000 groups over 70000 rows with an 8-aggregate record: the LDS
    table of a block holds 128 slots, every block meets about 250 groups,
    so the LDS attempt aborts and the global table runs on a zeroed
    table."""
    b = big_cols
    t = pa.table({"k": pa.array(b["k20k"]), "d": b["d"], "s": b["s"],
                  "dt": b["dt"], "v": b["v"]})
    reg("mm5", t)
    aggs = minmax_aggs(["d", "s", "dt"]) + [
        {"fn": "sum", "as": "v_sum", "expr": {"col": "v"}},
        {"fn": "avg", "as": "v_avg", "expr": {"col": "v"}}]
    assert len(aggs) == 8
    res = run(agg_plan(scan_of(t, "mm5"), ["k"], aggs))
    check_grouped(res, t, "k", ["d", "s", "dt"])


# ---- 6: one group, every row an improvement --------------------------------

@pytest.mark.parametrize("n", [70_000, 3_000])
def test_one_group_under_contention(ctx, reg, n):
    asc = [(i - n // 2) * ((1 << 64) + 1) for i in range(n)]  # both limbs
    none = np.zeros(n, dtype=bool)
    sasc = ["r%07d" % i for i in range(n)]
    t = pa.table({"d_desc": dec_array(asc[::-1], none, 38, 0),
                  "d_asc": dec_array(asc, none, 38, 0),
                  "s_desc": str_array(sasc[::-1], none),
                  "s_asc": str_array(sasc, none)})
    name = f"mm6_{n}"
    reg(name, t)
    # min over descending and max over ascending input: each row beats
    # every row before it
    res = run(agg_plan(scan_of(t, name), [], [
        {"fn": "min", "as": "d_desc_min", "expr": {"col": "d_desc"}},
        {"fn": "max", "as": "d_asc_max", "expr": {"col": "d_asc"}}]))
    got = got_columns(res)
    assert len(res["rows"]) == 1
    assert got["d_desc_min"][0] == asc[0] and got["d_asc_max"][0] == asc[-1]
    res = run(agg_plan(scan_of(t, name), [], [
        {"fn": "min", "as": "s_desc_min", "expr": {"col": "s_desc"}},
        {"fn": "max", "as": "s_asc_max", "expr": {"col": "s_asc"}}]))
    got = got_columns(res)
    assert len(res["rows"]) == 1
    assert got["s_desc_min"][0] == sasc[0] and got["s_asc_max"][0] == sasc[-1]
    check_one_group(run(agg_plan(scan_of(t, name), [],
                                 minmax_aggs(["d_desc", "s_asc"]))),
                    t, ["d_desc", "s_asc"])


# ---- 7: row encoding edges -------------------------------------------------

def test_row_encoding_edges(ctx, reg):
    """row + 1 encoding: a winner at row 0 and at row n-1; an all-NULL group
    gives NULL; a fused filter removes one key entirely and the extremum
    row of another, whose runner-up must win."""
    n = 1000
    keys = np.array([i % 5 for i in range(n)], dtype=np.int64)
    keys[0], keys[n - 1] = 0, 1
    vals = [1000 + i for i in range(n)]
    vals[0] = -DEC_MAX            # min of key 0 at row 0
    vals[n - 1] = DEC_MAX         # max of key 1 at row n-1
    strs = ["m%04d" % i for i in range(n)]
    strs[0], strs[n - 1] = "", "é"
    mask = keys == 2              # key 2: every value NULL
    f = np.full(n, 5, dtype=np.int64)
    f[keys == 3] = 100            # key 3: every row filtered out
    k4 = np.flatnonzero(keys == 4)
    vals[k4[7]] = -5              # key 4: its min row is filtered out ...
    strs[k4[7]] = "!"
    f[k4[7]] = 100
    vals[k4[9]] = -3              # ... so this runner-up wins
    strs[k4[9]] = "#"
    t = pa.table({"k": pa.array(keys), "f": pa.array(f),
                  "d": dec_array(vals, mask, 38, 2),
                  "s": str_array(strs, mask)})
    reg("mm7", t)
    flt = {"op": "filter", "predicates": [
        {"col": "f", "cmp": "ge_lt", "lo": 0, "hi": 10}],
        "input": scan_of(t, "mm7")}
    res = run(agg_plan(flt, ["k"], minmax_aggs(["d", "s"])))
    kept = t.filter(pa.array(f < 10))
    got = check_grouped(res, kept, "k", ["d", "s"])
    assert sorted(got["k"]) == [0, 1, 2, 4]
    row = {k: i for i, k in enumerate(got["k"])}
    assert got["d_min"][row[0]] == -DEC_MAX and got["s_min"][row[0]] == ""
    assert got["d_max"][row[1]] == DEC_MAX
    assert got["s_max"][row[1]] == "é"
    for nm in ("d_min", "d_max", "s_min", "s_max"):
        assert got[nm][row[2]] is None
    assert got["d_min"][row[4]] == -3 and got["s_min"][row[4]] == "#"


# ---- 8: partial, then final --------------------------------------------------

def test_partial_then_final(ctx, reg):
    rng = np.random.default_rng(108)
    n, half = 20_000, 10_000
    keys = rng.integers(0, 300, size=n, dtype=np.int64)
    mask_d, mask_s, mask_t = (nulls(rng, n) for _ in range(3))
    first = np.arange(n) < half
    for m in (mask_d, mask_s, mask_t):
        m[(keys == 7) & first] = True   # all NULL in the first half only
        m[keys == 9] = True             # all NULL in both halves
    t = pa.table({
        "k": pa.array(keys),
        "d": dec_array(edge_decimals(rng, keys + 100), mask_d, 38, 4),
        "s": str_array(edge_strings(rng, keys + 100), mask_s),
        "dt": date_array(rng.integers(-30000, 30000, size=n), mask_t)})
    cols = ["d", "s", "dt"]
    aggs = minmax_aggs(cols)
    parts = []
    for i, part in enumerate((t.slice(0, half), t.slice(half))):
        reg(f"mm8_{i}", part)
        res = run(agg_plan(scan_of(part, f"mm8_{i}"), ["k"], aggs,
                           mode="partial"))
        dts = out_dtypes(res)
        assert (dts["d_min"]["precision"], dts["d_min"]["scale"]) == (38, 4)
        assert dts["s_max"]["dtype"] == "utf8"
        assert dts["dt_min"]["dtype"] == "date32"
        assert dts["d_min$n"]["dtype"] == "int64"
        parts.append(result_table(res))
    # key 7's partial value is NULL with a zero count in the first half
    p0 = parts[0].to_pydict()
    i7 = p0["k"].index(7)
    assert p0["d_min"][i7] is None and p0["d_min$n"][i7] == 0
    merged = pa.concat_tables(parts)
    reg("mm8_p", merged)
    reg("mm8_all", t)
    # a final aggregate spends two kernel slots per aggregate (the value
    # and its "$n" sum) and the kernel has eight: mins and maxes apart
    for fn in ("min", "max"):
        faggs = minmax_aggs(cols, (fn,))
        fin = run(agg_plan(scan_of(merged, "mm8_p"), ["k"],
                           [{"fn": fn, "as": a["as"]} for a in faggs],
                           mode="final"))
        got = check_grouped(fin, t, "k", cols, (fn,))
        i9 = got["k"].index(9)
        assert all(got[a["as"]][i9] is None for a in faggs)
        assert got[f"d_{fn}"][got["k"].index(7)] is not None
        single = run(agg_plan(scan_of(t, "mm8_all"), ["k"], faggs))
        gs = got_columns(single)
        order_s = {k: i for i, k in enumerate(gs["k"])}
        for i, k in enumerate(got["k"]):
            for a in faggs:
                assert got[a["as"]][i] == gs[a["as"]][order_s[k]]
        assert fin["schema"] == single["schema"]


# ---- 9: the q2 and q15 shapes -------------------------------------------------

def test_q2_shape_min_decimal_over_filtered_join(ctx, reg):
    """min(ps_supplycost) Decimal(15,2) by ps_partkey over a filtered join
    output (build 500 suppliers, probe 5000 partsupp rows)."""
    rng = np.random.default_rng(109)
    nb, npr = 500, 5000
    supp = pa.table({"s_suppkey": pa.array(np.arange(nb, dtype=np.int64)),
                     "s_region": pa.array(rng.integers(0, 5, size=nb,
                                                       dtype=np.int64))})
    cost = rng.integers(100, 100_000, size=npr)
    ps = pa.table({
        "ps_partkey": pa.array(rng.integers(0, 800, size=npr,
                                            dtype=np.int64)),
        "ps_suppkey": pa.array(rng.integers(0, nb + 50, size=npr,
                                            dtype=np.int64)),
        "ps_supplycost": dec_array(cost, nulls(rng, npr, 0.1), 15, 2)})
    reg("mm9s", supp)
    reg("mm9p", ps)
    join = {"op": "hash_join", "build": scan_of(supp, "mm9s"),
            "probe": scan_of(ps, "mm9p"),
            "build_keys": ["s_suppkey"], "probe_keys": ["ps_suppkey"],
            "join_type": "inner",
            "output": [{"side": "probe", "col": "ps_partkey"},
                       {"side": "probe", "col": "ps_supplycost"},
                       {"side": "build", "col": "s_region"}]}
    flt = {"op": "filter", "input": join, "predicates": [
        {"col": "s_region", "cmp": "eq", "lo": 2}]}
    res = run(agg_plan(flt, ["ps_partkey"], [
        {"fn": "min", "as": "ps_supplycost_min",
         "expr": {"col": "ps_supplycost"}}]))
    region = np.asarray(supp["s_region"])
    sk = np.asarray(ps["ps_suppkey"])
    keep = (sk < nb) & (region[np.minimum(sk, nb - 1)] == 2)
    check_grouped(res, ps.filter(pa.array(keep)), "ps_partkey",
                  ["ps_supplycost"], fns=("min",))
    f = out_dtypes(res)["ps_supplycost_min"]
    assert (f["dtype"], f["precision"], f["scale"]) == ("decimal128", 15, 2)


def test_q15_shape_max_over_grouped_sum(ctx, reg):
    """max(total_revenue) with no group key over the Decimal(38,2) sum
    column of a preceding grouped aggregate."""
    rng = np.random.default_rng(110)
    n = 6000
    t = pa.table({
        "supplier_no": pa.array(rng.integers(0, 400, size=n,
                                             dtype=np.int64)),
        "rev": dec_array(rng.integers(-10**9, 10**12, size=n),
                         nulls(rng, n, 0.1), 15, 2)})
    reg("mm9r", t)
    inner = agg_plan(scan_of(t, "mm9r"), ["supplier_no"], [
        {"fn": "sum", "as": "total_revenue", "expr": {"col": "rev"}}])
    res = run(agg_plan(inner, [], [
        {"fn": "max", "as": "m", "expr": {"col": "total_revenue"}}]))
    sums = plain(t.group_by("supplier_no").aggregate([("rev", "sum")])
                 ["rev_sum"])
    assert len(res["rows"]) == 1
    assert got_columns(res)["m"][0] == max(s for s in sums if s is not None)
    f = out_dtypes(res)["m"]
    assert (f["dtype"], f["precision"], f["scale"]) == ("decimal128", 38, 2)


def test_dict8_rejected_by_both(ctx, reg):
    """min over a dictionary code column: bg_stage_validate and
    bg_execute_stage both answer BG_ERR_UNSUPPORTED."""
    t = pa.table({"k": pa.array(np.arange(64, dtype=np.int64) % 4),
                  "c": pa.array(np.arange(64, dtype=np.uint8))})
    reg("mm9d", t)
    doc = {"job_id": "job-mm", "stage_id": 1, "task_id": 0,
           "work_dir": "/tmp/stage-tests",
           "plan": {"op": "collect", "input": agg_plan(
               scan_of(t, "mm9d"), ["k"], minmax_aggs(["c"], ("min",)))}}
    with pytest.raises(RuntimeError, match=r"bg_stage_validate rc=-4"):
        stage.validate(doc)
    with pytest.raises(RuntimeError, match=r"bg_execute_stage rc=-4"):
        stage.execute(doc)


# ---- 10: the raw ops ---------------------------------------------------------

def test_raw_row_ops(ctx):
    rng = np.random.default_rng(111)
    n = 5000
    keys = rng.integers(0, 60, size=n, dtype=np.int64)
    vals = edge_decimals(rng, keys)
    strs = [s.encode() for s in edge_strings(rng, keys)]
    vd, vs = ~nulls(rng, n), ~nulls(rng, n)
    vd[keys == 20] = False  # one group with no non-NULL decimal
    vs[keys == 21] = False

    raw16 = np.frombuffer(b"".join(
        (v & ((1 << 128) - 1)).to_bytes(16, "little") for v in vals),
        dtype=np.uint8)
    kc, _ = ctx.upload_column(keys, gpu.BG_DT_INT64)
    dc, _ = ctx.upload_column(raw16, gpu.BG_DT_DECIMAL128,
                              validity=np.packbits(vd, bitorder="little"))
    sc = ctx.upload_utf8_column(strs)
    sc = ctx.column(gpu.BG_DT_UTF8, sc._keep[0], n,
                    validity=ctx.upload(np.packbits(vs, bitorder="little")),
                    offsets=sc._keep[2])
    ops = [gpu.BG_AGG_OP_MIN_ROW, gpu.BG_AGG_OP_MAX_ROW,
           gpu.BG_AGG_OP_MIN_ROW, gpu.BG_AGG_OP_MAX_ROW]
    first, acc, counts, nn = ctx.hashagg([kc], [dc, dc, sc, sc], ops, n,
                                         max_groups=256, want_nncnt=True)
    ng = len(first)
    assert ng == len(set(keys.tolist()))
    want = {}
    for k, v, s, okd, oks in zip(keys.tolist(), vals, strs, vd, vs):
        w = want.setdefault(k, [[], []])
        if okd:
            w[0].append(v)
        if oks:
            w[1].append(s)
    dacc = ctx.upload(acc)
    for a, op in enumerate(ops):
        src, which = (vals, 0) if a < 2 else (strs, 1)
        pick = min if op == gpu.BG_AGG_OP_MIN_ROW else max
        rows, valid = ctx.agg_winner_rows(dacc, 16 * len(ops), ng,
                                          byte_off=16 * a)
        for g in range(ng):
            k = int(keys[first[g]])
            r = gpu.decode_agg_value(op, bytes(acc[g, a]))
            assert int.from_bytes(bytes(acc[g, a, 8:]), "little") == 0
            assert (r is None) == (nn[g, a] == 0) == (not want[k][which])
            assert bool(valid[g]) == (r is not None)
            assert int(rows[g]) == (r or 0)
            if r is not None:
                assert int(keys[r]) == k
                assert src[r] == pick(want[k][which])
    assert any(nn[g, 0] == 0 for g in range(ng))

    # no input column to read the value from
    out = ctx.alloc(16 * ng)
    assert ctx.L.bg_agg_materialize(dacc.ptr, 16 * len(ops),
                                    gpu.BG_AGG_OP_MIN_ROW, ng, out.ptr, None,
                                    0, None) == BG_ERR_INVALID

    # an op over a dtype it cannot read is refused
    def rc_of(col, op):
        ngo = ctypes.c_int64()
        fb, ab, cb = ctx.alloc(4 * 256), ctx.alloc(16 * 256), \
            ctx.alloc(8 * 256)
        return ctx.L.bg_hashagg((gpu.BgColumn * 1)(kc), 1,
                                (gpu.BgColumn * 1)(col),
                                (ctypes.c_int32 * 1)(op), 1, None, n, 256,
                                fb.ptr, ab.ptr, cb.ptr, ctypes.byref(ngo))

    assert rc_of(kc, gpu.BG_AGG_OP_MIN_ROW) == BG_ERR_UNSUPPORTED
    assert rc_of(kc, gpu.BG_AGG_OP_MAX_I32) == BG_ERR_UNSUPPORTED
    assert rc_of(dc, gpu.BG_AGG_OP_MIN_I32) == BG_ERR_UNSUPPORTED


def test_raw_i32_ops(ctx):
    rng = np.random.default_rng(112)
    n = 5000
    keys = rng.integers(0, 60, size=n, dtype=np.int64)
    v = rng.integers(-10**4, 10**4, size=n).astype(np.int32)
    v[:4] = [I32_MIN, I32_MAX, -1, 0]
    ok = ~nulls(rng, n)
    ok[keys == 20] = False
    kc, _ = ctx.upload_column(keys, gpu.BG_DT_INT64)
    for dt in (gpu.BG_DT_INT32, gpu.BG_DT_DATE32):
        vc, _ = ctx.upload_column(v, dt, validity=np.packbits(
            ok, bitorder="little"))
        ops = [gpu.BG_AGG_OP_MIN_I32, gpu.BG_AGG_OP_MAX_I32]
        first, acc, counts, nn = ctx.hashagg([kc], [vc, vc], ops, n,
                                             max_groups=256, want_nncnt=True)
        ng = len(first)
        dacc = ctx.upload(acc)
        outs = []
        for a, op in enumerate(ops):
            ob = ctx.alloc(4 * ng)
            vb = ctx.alloc(ng // 8 + 16)
            nnb = ctx.upload(nn)
            gpu._check(ctx.L.bg_agg_materialize(
                dacc.at(16 * a), 32, op, ng, ob.ptr, nnb.at(8 * a), 16,
                vb.ptr), "bg_agg_materialize")
            bits = np.unpackbits(vb.download(np.uint8, (ng + 7) // 8),
                                 bitorder="little")[:ng]
            outs.append((ob.download(np.int32, ng), bits))
        for g in range(ng):
            k = int(keys[first[g]])
            grp = v[(keys == k) & ok].tolist()
            for a, (op, pick) in enumerate(zip(ops, (min, max))):
                if not grp:
                    assert nn[g, a] == 0 and outs[a][1][g] == 0
                    continue
                assert gpu.decode_agg_value(op, bytes(acc[g, a])) == \
                    pick(grp)
                assert outs[a][1][g] == 1 and outs[a][0][g] == pick(grp)
