"""CPU-side checks (no GPU) of cast, div, lit_f64 and Float64 mul|add|sub in
the plan grammar: bg_stage_validate infers each result's dtype, precision
and scale wherever an expression is accepted, and refuses ill-typed uses
with a message naming the node and the operands."""
import pytest

from datafusion_ballista_amd import stage

SCAN = {"op": "scan",
        "schema": [{"name": "k32", "dtype": "int32"},
                   {"name": "k64", "dtype": "int64"},
                   {"name": "l_quantity", "dtype": "decimal128",
                    "precision": 15, "scale": 2},
                   {"name": "share", "dtype": "decimal128",
                    "precision": 38, "scale": 4},
                   {"name": "volume", "dtype": "decimal128",
                    "precision": 38, "scale": 4},
                   {"name": "tax", "dtype": "decimal128",
                    "precision": 15, "scale": 6},
                   {"name": "f", "dtype": "float64"},
                   {"name": "g", "dtype": "float64"},
                   {"name": "d", "dtype": "date32"},
                   {"name": "c_name", "dtype": "utf8"}],
        "source": {"kind": "device", "table": "t"}}

F64 = {"dtype": "float64"}
I64 = {"dtype": "int64"}


def DEC(p, s):
    return {"dtype": "decimal128", "precision": p, "scale": s}


def cast(arg, to):
    return {"cast": {"arg": arg if isinstance(arg, dict) else {"col": arg},
                     "to": to}}


def col(name):
    return {"col": name}


def _doc(plan):
    return {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
            "plan": {"op": "collect", "input": plan}}


def _project(*exprs):
    return _doc({"op": "project", "input": SCAN,
                 "exprs": [{"as": f"e{i}", "expr": e}
                           for i, e in enumerate(exprs)]})


def _types(res):
    """(dtype, precision, scale) per output field; decimals only carry the
    last two."""
    return [(f["dtype"], f.get("precision"), f.get("scale"))
            if f["dtype"] == "decimal128" else (f["dtype"], None, None)
            for f in res["schema"]]


def _one(expr):
    return _types(stage.validate(_project(expr)))[0]


# ---------------------------------------------------------------------------
# inferred types
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["k32", "k64", "l_quantity", "share"])
def test_cast_to_float64(src):
    assert _one(cast(src, F64)) == ("float64", None, None)


@pytest.mark.parametrize("src", ["k32", "k64", "l_quantity", "f"])
@pytest.mark.parametrize("p,s", [(30, 15), (38, 15), (19, 6), (15, 2),
                                 (1, 0), (38, 38)])
def test_cast_to_decimal_carries_precision_and_scale(src, p, s):
    assert _one(cast(src, DEC(p, s))) == ("decimal128", p, s)


def test_cast_int32_to_int64():
    assert _one(cast("k32", I64)) == ("int64", None, None)


def test_cast_of_a_cast_q17():
    """q17.txt:27: CAST(0.2 * CAST(avg AS Float64) AS Decimal128(30,15))"""
    e = cast({"mul": [{"lit_f64": 0.2}, cast("l_quantity", F64)]},
             DEC(30, 15))
    assert _one(e) == ("decimal128", 30, 15)


def test_div_of_decimals_default_scale_is_s1_plus_4():
    assert _one({"div": [col("share"), col("volume")]}) == \
        ("decimal128", 38, 8)
    assert _one({"div": [col("l_quantity"), col("tax")]}) == \
        ("decimal128", 38, 6)


def test_div_default_scale_is_capped_at_38():
    e = {"div": [cast("l_quantity", DEC(38, 36)), col("l_quantity")]}
    assert _one(e) == ("decimal128", 38, 38)


@pytest.mark.parametrize("scale", [0, 4, 6, 12])
def test_div_explicit_scale_pins_the_result_type(scale):
    e = {"div": [col("share"), col("volume")], "scale": scale}
    assert _one(e) == ("decimal128", 38, scale)


@pytest.mark.parametrize("op", ["mul", "add", "sub", "div"])
def test_float64_arithmetic(op):
    exprs = [{op: [col("f"), col("g")]},
             {op: [col("f"), {"lit_f64": 0.0001}]},
             {op: [{"lit_f64": 100}, col("g")]}]       # integer token
    res = stage.validate(_project(*exprs))
    assert _types(res) == [("float64", None, None)] * 3


def test_q14_projection():
    """q14.txt:22: 100 * CAST(a AS Float64) / CAST(b AS Float64)"""
    e = {"div": [{"mul": [{"lit_f64": 100}, cast("share", F64)]},
                 cast("volume", F64)]}
    assert _one(e) == ("float64", None, None)


def test_decimal_arithmetic_is_unchanged():
    res = stage.validate(_project(
        {"mul": [col("l_quantity"), col("tax")]},
        {"sub": [col("l_quantity"), {"lit": 100}]},
        {"add": [col("tax"), {"lit": 1}]}))
    assert _types(res) == [("decimal128", 38, 8), ("decimal128", 38, 2),
                           ("decimal128", 38, 6)]


def test_cast_as_aggregate_input():
    res = stage.validate(_doc({
        "op": "hash_aggregate", "mode": "single", "group_by": ["k32"],
        "aggs": [{"fn": "sum", "as": "s",
                  "expr": cast("l_quantity", F64)},
                 {"fn": "sum", "as": "w",
                  "expr": cast("l_quantity", DEC(30, 15))},
                 {"fn": "max", "as": "m",
                  "expr": {"div": [col("share"), col("volume")]}}],
        "input": SCAN}))
    t = dict(zip((f["name"] for f in res["schema"]), _types(res)))
    assert t["k32"] == ("int32", None, None)
    assert t["s"] == ("float64", None, None)
    assert t["w"][0] == "decimal128" and t["w"][2] == 15
    assert t["m"][0] == "decimal128" and t["m"][2] == 8


def test_cast_as_predicate_operand():
    res = stage.validate(_doc({"op": "filter", "input": SCAN, "predicates": [
        {"expr": cast("l_quantity", DEC(30, 15)), "cmp": "lt",
         "hi": 24 * 10**15},
        {"expr": cast("k32", I64), "cmp": "eq", "lo": 7}]}))
    assert res["ok"] is True
    assert len(res["schema"]) == len(SCAN["schema"])


def test_cast_inside_case_branches():
    e = {"case": {"when": [{"col": "k32", "cmp": "eq", "lo": 1}],
                  "then": cast("l_quantity", DEC(30, 15)),
                  "else": cast("tax", DEC(30, 15))}}
    assert _one(e) == ("decimal128", 30, 15)


def test_cast_as_group_by_key_via_project():
    res = stage.validate(_doc({
        "op": "hash_aggregate", "mode": "single", "group_by": ["key"],
        "aggs": [{"fn": "count", "as": "c"}],
        "input": {"op": "project", "input": SCAN, "exprs": [
            {"as": "key", "expr": cast("k32", I64)}]}}))
    assert _types(res)[0] == ("int64", None, None)
    assert res["schema"][0]["name"] == "key"


def test_cast_as_shuffle_writer_key():
    doc = {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
           "schema_msg_hex": "00",
           "plan": {"op": "sort_shuffle_write", "k": 4,
                    "keys": [cast("k32", I64)], "input": SCAN}}
    assert stage.validate(doc)["ok"] is True


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("src,to,names", [
    ("c_name", F64, ("utf8", "float64")),
    ("d", F64, ("date32", "float64")),
    ("f", I64, ("float64", "int64")),
    ("k64", {"dtype": "int32"}, ("int64", "int32")),
    ("l_quantity", I64, ("decimal128(15,2)", "int64")),
    ("f", {"dtype": "utf8"}, ("float64", "utf8")),
])
def test_refuses_unsupported_cast_pair(src, to, names):
    msg = stage.validate_error(_project(cast(src, to)))
    assert "cast" in msg and src in msg
    for n in names:
        assert n in msg


def test_refusal_names_a_nested_argument():
    inner = {"date_part": {"part": "year", "arg": col("d")}}
    msg = stage.validate_error(_project(cast(inner, {"dtype": "utf8"})))
    assert "cast" in msg and "date_part(d)" in msg and "int32" in msg


@pytest.mark.parametrize("to", [
    {"dtype": "decimal128"},
    {"dtype": "decimal128", "precision": 19},
    {"dtype": "decimal128", "scale": 6},
    {"dtype": "decimal128", "precision": "19", "scale": 6},
])
def test_refuses_missing_precision_or_scale(to):
    msg = stage.validate_error(_project(cast("l_quantity", to)))
    assert "cast" in msg and "l_quantity" in msg
    assert "precision" in msg or "scale" in msg


@pytest.mark.parametrize("p,s", [(0, 0), (39, 2), (10, 11), (10, -1)])
def test_refuses_illegal_precision_or_scale(p, s):
    msg = stage.validate_error(_project(cast("l_quantity", DEC(p, s))))
    assert "cast" in msg and "l_quantity" in msg and f"({p},{s})" in msg


def test_refuses_cast_of_a_literal():
    msg = stage.validate_error(_project(cast({"lit_f64": 1.5}, DEC(10, 2))))
    assert "cast" in msg and "literal" in msg


@pytest.mark.parametrize("op", ["mul", "add", "sub", "div"])
@pytest.mark.parametrize("ops", [
    (col("f"), col("l_quantity")),
    (col("l_quantity"), col("f")),
    (col("f"), col("k64")),
    (col("l_quantity"), {"lit_f64": 0.5}),
    (col("f"), {"lit": 5}),
])
def test_refuses_float64_mixed_with_another_type(op, ops):
    msg = stage.validate_error(_project({op: list(ops)}))
    assert op in msg and "float64" in msg
    for o in ops:   # a column by its name, a literal by its node kind
        assert f"'{o['col'] if 'col' in o else list(o)[0]}'" in msg


def test_mixed_refusal_names_both_operands():
    msg = stage.validate_error(_project(
        {"mul": [col("f"), cast("k32", DEC(10, 0))]}))
    assert "mul" in msg and "'f'" in msg and "cast(k32)" in msg \
        and "float64" in msg and "decimal128" in msg


@pytest.mark.parametrize("ops", [
    (col("share"), {"lit": 7}),
    ({"lit": 7}, col("share")),
])
def test_refuses_decimal_div_with_a_literal(ops):
    msg = stage.validate_error(_project({"div": list(ops)}))
    assert "div" in msg and "literal" in msg and "share" in msg


def test_refuses_decimal_div_of_other_dtypes():
    msg = stage.validate_error(_project({"div": [col("k64"), col("share")]}))
    assert "div" in msg and "k64" in msg and "int64" in msg


def test_refuses_div_scale_that_cannot_align():
    msg = stage.validate_error(_project(
        {"div": [col("share"), col("volume")], "scale": 39}))
    assert "div" in msg and "39" in msg


@pytest.mark.parametrize("op", ["mul", "add", "sub", "div"])
@pytest.mark.parametrize("lits", [
    ({"lit_f64": 1.0}, {"lit_f64": 2.0}),
    ({"lit": 1}, {"lit": 2}),
    ({"lit": 1}, {"lit_f64": 2.0}),
])
def test_refuses_two_literals(op, lits):
    msg = stage.validate_error(_project({op: list(lits)}))
    assert op in msg and "two literals" in msg


def test_refuses_non_numeric_lit_f64():
    msg = stage.validate_error(_project(
        {"mul": [col("f"), {"lit_f64": "0.5"}]}))
    assert "lit_f64" in msg


def test_float64_column_compares_stay_refused():
    """Out of scope here: cast results do not make Float64 column-to-column
    compares expressible."""
    msg = stage.validate_error(_doc({
        "op": "filter", "predicates": [
            {"col": "x", "cmp": "lt", "rhs": {"col": "g"}}],
        "input": {"op": "project", "input": SCAN, "exprs": [
            {"as": "x", "expr": cast("l_quantity", F64)},
            {"as": "g", "expr": col("g")}]}}))
    assert "rhs" in msg and "float64" in msg
