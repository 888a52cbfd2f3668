"""CPU-side checks (no GPU) of the scalar-expression additions to the plan
grammar: bg_stage_validate infers date_part -> int32 and substr -> utf8,
accepts "expr" predicate operands, string IN lists and column-to-column
("rhs") compares in filters and in case.when, and refuses every ill-typed
use with a message naming the node and the column."""
import pytest

from datafusion_ballista_amd import stage

SCAN = {"op": "scan",
        "schema": [{"name": "l_shipdate", "dtype": "date32"},
                   {"name": "l_commitdate", "dtype": "date32"},
                   {"name": "l_receiptdate", "dtype": "date32"},
                   {"name": "l_orderkey", "dtype": "int64"},
                   {"name": "l_shipmode", "dtype": "dict8"},
                   {"name": "c_phone", "dtype": "utf8"},
                   {"name": "c_acctbal", "dtype": "decimal128",
                    "precision": 15, "scale": 2},
                   {"name": "l_tax", "dtype": "decimal128",
                    "precision": 15, "scale": 4},
                   {"name": "l_price", "dtype": "decimal128",
                    "precision": 15, "scale": 2},
                   {"name": "f", "dtype": "float64"},
                   {"name": "g", "dtype": "float64"},
                   {"name": "c_name", "dtype": "utf8"}],
        "source": {"kind": "device", "table": "t"}}


def _doc(plan):
    return {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
            "plan": {"op": "collect", "input": plan}}


def _project(*exprs):
    return _doc({"op": "project", "input": SCAN,
                 "exprs": [{"as": f"e{i}", "expr": e}
                           for i, e in enumerate(exprs)]})


def _filter(*preds):
    return _doc({"op": "filter", "input": SCAN, "predicates": list(preds)})


def _dtypes(res):
    return [f["dtype"] for f in res["schema"]]


@pytest.mark.parametrize("part", ["year", "quarter", "month", "day", "doy",
                                  "dow"])
def test_date_part_projects_int32(part):
    res = stage.validate(_project(
        {"date_part": {"part": part, "arg": {"col": "l_shipdate"}}},
        {"col": "l_orderkey"}))
    assert res["ok"] is True
    assert _dtypes(res) == ["int32", "int64"]


def test_substr_projects_utf8():
    res = stage.validate(_project(
        {"substr": {"arg": {"col": "c_phone"}, "start": 1, "count": 2}},
        {"substr": {"arg": {"col": "c_phone"}, "start": 3}}))
    assert res["ok"] is True
    assert _dtypes(res) == ["utf8", "utf8"]


def test_group_by_projected_year_and_code():
    """The q9/q22 shape: GROUP BY a projected date_part / substr column."""
    res = stage.validate(_doc({
        "op": "hash_aggregate", "mode": "single",
        "group_by": ["o_year", "cntrycode"],
        "aggs": [{"fn": "sum", "as": "s", "expr": {"col": "c_acctbal"}}],
        "input": {"op": "project", "input": SCAN, "exprs": [
            {"as": "o_year", "expr": {"date_part": {
                "part": "year", "arg": {"col": "l_shipdate"}}}},
            {"as": "cntrycode", "expr": {"substr": {
                "arg": {"col": "c_phone"}, "start": 1, "count": 2}}},
            {"as": "c_acctbal", "expr": {"col": "c_acctbal"}}]}}))
    assert _dtypes(res)[:2] == ["int32", "utf8"]


def test_filter_expr_operand_with_string_in():
    res = stage.validate(_filter(
        {"expr": {"substr": {"arg": {"col": "c_phone"}, "start": 1,
                             "count": 2}}, "in": ["13", "31"]},
        {"col": "c_name", "in": ["a", "b"]},
        {"expr": {"date_part": {"part": "year",
                                "arg": {"col": "l_shipdate"}}},
         "cmp": "eq", "lo": 1995}))
    assert res["ok"] is True


@pytest.mark.parametrize("cmp", ["lt", "le", "gt", "ge", "eq", "ne"])
def test_filter_rhs_compare_on_dates(cmp):
    res = stage.validate(_filter(
        {"col": "l_receiptdate", "cmp": cmp, "rhs": {"col": "l_commitdate"}},
        {"col": "l_shipdate", "cmp": "lt", "rhs": {"col": "l_commitdate"}},
        {"col": "l_receiptdate", "cmp": "ge_lt", "lo": 8766, "hi": 9131}))
    assert res["ok"] is True


def test_filter_rhs_compare_in_any_group_and_on_decimals():
    res = stage.validate(_doc({"op": "filter", "input": SCAN, "any": [
        [{"col": "c_acctbal", "cmp": "gt", "rhs": {"col": "l_price"}}],
        [{"col": "l_shipmode", "cmp": "ne", "rhs": {"col": "l_shipmode"}}]]}))
    assert res["ok"] is True


def test_case_when_inherits_the_predicate_grammar():
    res = stage.validate(_project(
        {"case": {"when": [{"col": "l_receiptdate", "cmp": "gt",
                            "rhs": {"col": "l_commitdate"}},
                           {"expr": {"substr": {"arg": {"col": "c_phone"},
                                                "start": 1, "count": 2}},
                            "in": ["13"]}],
                  "then": {"col": "c_acctbal"}, "else": {"lit": 0}}}))
    assert res["ok"] is True
    assert _dtypes(res) == ["decimal128"]


# ---- refusals: each names the offending node and column ----

def test_refuses_date_part_of_non_date():
    msg = stage.validate_error(_project(
        {"date_part": {"part": "year", "arg": {"col": "l_orderkey"}}}))
    assert "date_part" in msg and "l_orderkey" in msg and "int64" in msg


def test_refuses_unknown_part():
    msg = stage.validate_error(_project(
        {"date_part": {"part": "week", "arg": {"col": "l_shipdate"}}}))
    assert "date_part" in msg and "week" in msg


def test_refuses_substr_of_non_utf8():
    msg = stage.validate_error(_project(
        {"substr": {"arg": {"col": "l_shipdate"}, "start": 1, "count": 2}}))
    assert "substr" in msg and "l_shipdate" in msg and "date32" in msg


def test_refuses_negative_count():
    msg = stage.validate_error(_project(
        {"substr": {"arg": {"col": "c_phone"}, "start": 1, "count": -1}}))
    assert "negative substring length not allowed" in msg
    assert "substr" in msg and "c_phone" in msg


def test_refuses_nested_ill_typed_expr_in_predicate():
    msg = stage.validate_error(_filter(
        {"expr": {"substr": {"arg": {"date_part": {
            "part": "year", "arg": {"col": "l_shipdate"}}}, "start": 1}},
         "in": ["19"]}))
    assert "substr" in msg and "date_part(l_shipdate)" in msg \
        and "int32" in msg


def test_refuses_string_in_on_non_utf8_operand():
    msg = stage.validate_error(_filter(
        {"col": "l_shipmode", "in": ["MAIL", "SHIP"]}))
    assert "'in'" in msg and "string" in msg and "l_shipmode" in msg \
        and "dict8" in msg


def test_refuses_integer_in_on_utf8_operand():
    msg = stage.validate_error(_filter(
        {"expr": {"substr": {"arg": {"col": "c_phone"}, "start": 1,
                             "count": 2}}, "in": [13, 31]}))
    assert "'in'" in msg and "integer" in msg and "substr(c_phone)" in msg \
        and "utf8" in msg


def test_refuses_rhs_dtype_mismatch():
    msg = stage.validate_error(_filter(
        {"col": "l_shipdate", "cmp": "lt", "rhs": {"col": "l_orderkey"}}))
    assert "rhs" in msg and "l_shipdate" in msg and "l_orderkey" in msg \
        and "date32" in msg and "int64" in msg


def test_refuses_rhs_scale_mismatch():
    msg = stage.validate_error(_filter(
        {"col": "c_acctbal", "cmp": "lt", "rhs": {"col": "l_tax"}}))
    assert "scale" in msg and "c_acctbal" in msg and "l_tax" in msg


@pytest.mark.parametrize("extra", [{"lo": 1}, {"hi": 1}, {"like": "a%"},
                                   {"in": [1]}])
def test_refuses_rhs_with_literal_forms(extra):
    pred = {"col": "l_shipdate", "cmp": "lt", "rhs": {"col": "l_commitdate"}}
    pred.update(extra)
    msg = stage.validate_error(_filter(pred))
    assert "rhs" in msg and "l_shipdate" in msg and list(extra)[0] in msg


def test_refuses_unknown_column_compare():
    # ge_lt is a literal form: with "rhs" present it is not a compare
    msg = stage.validate_error(_filter(
        {"col": "l_shipdate", "cmp": "ge_lt", "rhs": {"col": "l_commitdate"}}))
    assert "ge_lt" in msg


def test_refuses_unknown_rhs_column():
    msg = stage.validate_error(_filter(
        {"col": "l_shipdate", "cmp": "lt", "rhs": {"col": "nope"}}))
    assert "nope" in msg


@pytest.mark.parametrize("a,b", [("f", "g"), ("c_phone", "c_name")])
def test_refuses_float_and_utf8_column_compares(a, b):
    msg = stage.validate_error(_filter(
        {"col": a, "cmp": "lt", "rhs": {"col": b}}))
    assert "rhs" in msg and a in msg and b in msg


def test_refusal_inside_case_when_is_the_same_validator():
    msg = stage.validate_error(_project(
        {"case": {"when": [{"col": "l_shipdate", "cmp": "lt",
                            "rhs": {"col": "l_orderkey"}}],
                  "then": {"col": "c_acctbal"}, "else": {"lit": 0}}}))
    assert "rhs" in msg and "l_shipdate" in msg and "l_orderkey" in msg


def test_literal_forms_keep_their_meaning():
    """lt/eq/gt without "rhs" are still the column-vs-literal compares."""
    res = stage.validate(_filter(
        {"col": "l_shipdate", "cmp": "lt", "hi": 9000},
        {"col": "l_orderkey", "cmp": "eq", "lo": 7},
        {"col": "c_acctbal", "cmp": "gt", "lo": 0},
        {"col": "c_phone", "like": "13%"},
        {"col": "l_shipmode", "in": [1, 2]}))
    assert res["ok"] is True
    msg = stage.validate_error(_filter(
        {"col": "l_shipdate", "cmp": "le", "hi": 9000}))
    assert "le" in msg
