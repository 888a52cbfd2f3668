"""CPU-side checks (no GPU) of the window node in the plan grammar
(DataFusion WindowAggExec / BoundedWindowAggExec, Ballista's
PartitionedBoundedWindowAggExec): bg_stage_validate accepts every fn and
every frame shape with the exact output schema, and refuses each malformed
node with the right status and a message naming the node and the offender."""
import copy
import ctypes
import json

import pytest

from datafusion_ballista_amd import gpu, stage

BG_ERR_INVALID, BG_ERR_UNSUPPORTED = -3, -4
I64 = {"dtype": "int64"}
D17 = {"dtype": "decimal128", "precision": 17, "scale": 2}
INPUT_SCHEMA = [{"name": "k", **I64},
                {"name": "k32", "dtype": "int32"},
                {"name": "d", "dtype": "date32"},
                {"name": "f", "dtype": "float64"},
                {"name": "x", **D17},
                {"name": "v", **I64},
                {"name": "s", "dtype": "utf8"},
                {"name": "k2", **I64}, {"name": "k3", **I64},
                {"name": "k4", **I64}, {"name": "k5", **I64}]
SCAN = {"op": "scan", "schema": INPUT_SCHEMA,
        "source": {"kind": "device", "table": "t"}}

UNB, CUR = "unbounded", "current_row"


def P(n):
    return {"preceding": n}


def F(n):
    return {"following": n}


def frame(units, start, end):
    return {"units": units, "start": start, "end": end}


RUNNING = frame("rows", UNB, CUR)
WHOLE = frame("rows", UNB, UNB)


def window(exprs, partition_by=("k",), order_by=("d",)):
    order = [o if isinstance(o, dict) else {"col": o} for o in order_by]
    node = {"op": "window", "partition_by": list(partition_by),
            "order_by": order, "exprs": copy.deepcopy(exprs), "input": SCAN}
    return {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
            "plan": {"op": "collect", "input": node}}


def schema_of(doc):
    res = stage.validate(doc)
    assert res["ok"] is True
    return res["schema"]


def refusal(doc):
    """-> (return code, message) of a plan bg_stage_validate refuses."""
    L = gpu.load_library()
    out = ctypes.c_char_p()
    rc = L.bg_stage_validate(json.dumps(doc).encode(), ctypes.byref(out))
    assert rc != 0, "plan unexpectedly validated"
    return rc, L.bg_last_error().decode()


# fn, expr, expected output field (without the name)
FNS = [("row_number", None, I64), ("rank", None, I64),
       ("dense_rank", None, I64),
       ("sum", {"col": "v"}, I64),
       ("sum", {"col": "x"},
        {"dtype": "decimal128", "precision": 38, "scale": 2}),
       ("sum", {"col": "f"}, {"dtype": "float64"}),
       ("avg", {"col": "x"},
        {"dtype": "decimal128", "precision": 21, "scale": 6}),
       ("avg", {"col": "f"}, {"dtype": "float64"}),
       ("min", {"col": "x"}, D17), ("max", {"col": "v"}, I64),
       ("min", {"col": "k32"}, {"dtype": "int32"}),
       ("max", {"col": "d"}, {"dtype": "date32"}),
       ("min", {"col": "f"}, {"dtype": "float64"}),
       ("count", {"col": "s"}, I64), ("count", None, I64)]


@pytest.mark.parametrize("fn,expr,field", FNS,
                         ids=[f"{f}-{(e or {}).get('col', 'none')}"
                              for f, e, _ in FNS])
def test_every_fn_validates_with_its_schema(fn, expr, field):
    e = {"fn": fn, "as": "w"}
    if expr is not None:
        e["expr"] = expr
    if fn not in ("row_number", "rank", "dense_rank"):
        e["frame"] = RUNNING
    assert schema_of(window([e])) == INPUT_SCHEMA + [{"name": "w", **field}]


ROWS_FRAMES = [(UNB, CUR), (UNB, UNB), (P(2), F(1)), (P(3), P(1)),
               (F(1), F(3)), (CUR, UNB)]
RANGE_PEER_FRAMES = [(UNB, CUR), (CUR, CUR), (UNB, UNB)]
RANGE_OFFSET_FRAMES = [(P(1), F(1)), (P(2), CUR), (CUR, F(2)), (F(1), F(2))]


@pytest.mark.parametrize("start,end", ROWS_FRAMES)
def test_rows_frames_validate(start, end):
    e = {"fn": "sum", "as": "w", "expr": {"col": "v"},
         "frame": frame("rows", start, end)}
    assert schema_of(window([e]))[-1] == {"name": "w", **I64}


@pytest.mark.parametrize("start,end", RANGE_PEER_FRAMES)
def test_range_peer_frames_validate_with_two_order_keys(start, end):
    e = {"fn": "count", "as": "w", "frame": frame("range", start, end)}
    assert schema_of(window([e], order_by=("d", "v")))[-1] == \
        {"name": "w", **I64}


@pytest.mark.parametrize("start,end", RANGE_OFFSET_FRAMES)
@pytest.mark.parametrize("order", [{"col": "v"},
                                   {"col": "d", "desc": True},
                                   {"col": "k32", "nulls_first": True},
                                   {"col": "f"}])
def test_range_offset_frames_validate(order, start, end):
    e = {"fn": "sum", "as": "w", "expr": {"col": "x"},
         "frame": frame("range", start, end)}
    assert schema_of(window([e], order_by=(order,)))[-1]["precision"] == 38


def test_fractional_range_offset_over_a_float64_key():
    e = {"fn": "sum", "as": "w", "expr": {"col": "f"},
         "frame": frame("range", P(2.0), CUR)}
    assert schema_of(window([e], order_by=("f",)))[-1] == \
        {"name": "w", "dtype": "float64"}
    rc, msg = refusal(window([e], order_by=("v",)))
    assert rc == BG_ERR_INVALID and "window" in msg and "'w'" in msg


def test_empty_partition_by_and_empty_order_by():
    e = [{"fn": "rank", "as": "r"},
         {"fn": "avg", "as": "a", "expr": {"col": "x"}, "frame": WHOLE}]
    want = INPUT_SCHEMA + [
        {"name": "r", **I64},
        {"name": "a", "dtype": "decimal128", "precision": 21, "scale": 6}]
    assert schema_of(window(e, partition_by=())) == want
    assert schema_of(window(e, order_by=())) == want
    assert schema_of(window(e, partition_by=(), order_by=())) == want


def test_expression_input_and_several_exprs_in_one_node():
    e = [{"fn": "sum", "as": "a",
          "expr": {"mul": [{"col": "x"}, {"col": "x"}]}, "frame": RUNNING},
         {"fn": "row_number", "as": "b"},
         {"fn": "max", "as": "c", "expr": {"col": "x"}, "frame": WHOLE}]
    assert schema_of(window(e))[-3:] == [
        {"name": "a", "dtype": "decimal128", "precision": 38, "scale": 4},
        {"name": "b", **I64}, {"name": "c", **D17}]


SUM_V = {"fn": "sum", "as": "w", "expr": {"col": "v"}, "frame": RUNNING}


def with_(**kw):
    e = copy.deepcopy(SUM_V)
    for k, v in kw.items():
        if v is None:
            e.pop(k, None)
        else:
            e[k] = v
    return e


REFUSALS = {
    "unknown fn": (window([with_(fn="ntile")]), BG_ERR_INVALID, ["ntile"]),
    "aggregate without frame":
        (window([with_(frame=None)]), BG_ERR_INVALID, ["'w'", "frame"]),
    "aggregate without expr":
        (window([with_(expr=None)]), BG_ERR_INVALID, ["'w'", "expr"]),
    "min without expr":
        (window([with_(fn="min", expr=None, frame=WHOLE)]), BG_ERR_INVALID,
         ["min", "expr"]),
    "expr on a ranking fn":
        (window([{"fn": "rank", "as": "r", "expr": {"col": "v"}}]),
         BG_ERR_INVALID, ["rank", "'r'", "expr"]),
    "unknown partition column":
        (window([SUM_V], partition_by=("nope",)), BG_ERR_INVALID,
         ["partition_by", "'nope'"]),
    "unknown order column":
        (window([SUM_V], order_by=("nope",)), BG_ERR_INVALID,
         ["order_by", "'nope'"]),
    "duplicate as":
        (window([SUM_V, {"fn": "rank", "as": "w"}]), BG_ERR_INVALID,
         ["'w'", "duplicate"]),
    "as equal to an input column":
        (window([with_(**{"as": "v"})]), BG_ERR_INVALID, ["'v'", "input"]),
    "groups":
        (window([with_(frame=frame("groups", UNB, CUR))]),
         BG_ERR_UNSUPPORTED, ["'w'", "groups"]),
    "negative offset":
        (window([with_(frame=frame("rows", P(-1), CUR))]), BG_ERR_INVALID,
         ["'w'", "negative"]),
    "start after end (following, preceding)":
        (window([with_(frame=frame("rows", F(1), P(1)))]), BG_ERR_INVALID,
         ["'w'", "1 following", "1 preceding"]),
    "start after end (current row, preceding)":
        (window([with_(frame=frame("range", CUR, P(1)))], order_by=("v",)),
         BG_ERR_INVALID, ["'w'", "current row", "1 preceding"]),
    "start after end (1 preceding, 3 preceding)":
        (window([with_(frame=frame("rows", P(1), P(3)))]), BG_ERR_INVALID,
         ["'w'", "3 preceding"]),
    "range offset with no order key":
        (window([with_(frame=frame("range", P(1), CUR))], order_by=()),
         BG_ERR_INVALID, ["'w'", "order_by", "1 preceding"]),
    "range offset with two order keys":
        (window([with_(frame=frame("range", P(1), CUR))],
                order_by=("d", "v")),
         BG_ERR_INVALID, ["'w'", "order_by", "1 preceding"]),
    "range offset over utf8":
        (window([with_(frame=frame("range", P(1), CUR))], order_by=("s",)),
         BG_ERR_UNSUPPORTED, ["'w'", "utf8"]),
    "range offset over decimal128":
        (window([with_(frame=frame("range", CUR, F(1)))], order_by=("x",)),
         BG_ERR_UNSUPPORTED, ["'w'", "decimal128"]),
    "sliding min":
        (window([with_(fn="min", frame=frame("rows", P(2), CUR))]),
         BG_ERR_UNSUPPORTED, ["'w'", "min", "2 preceding"]),
    "sliding max over range":
        (window([with_(fn="max", frame=frame("range", CUR, UNB))]),
         BG_ERR_UNSUPPORTED, ["'w'", "max", "current row"]),
    "min over utf8":
        (window([with_(fn="min", expr={"col": "s"}, frame=WHOLE)]),
         BG_ERR_UNSUPPORTED, ["'w'", "min", "utf8"]),
    "sum over int32":
        (window([with_(expr={"col": "k32"})]), BG_ERR_UNSUPPORTED,
         ["'w'", "sum", "int32"]),
    "avg over int64":
        (window([with_(fn="avg")]), BG_ERR_UNSUPPORTED,
         ["'w'", "avg", "int64"]),
    "sum over utf8":
        (window([with_(expr={"col": "s"})]), BG_ERR_UNSUPPORTED,
         ["'w'", "sum", "utf8"]),
    "five partition keys":
        (window([SUM_V], partition_by=("k", "k2", "k3", "k4", "k5")),
         BG_ERR_INVALID, ["partition_by", "5"]),
    "five order keys":
        (window([SUM_V], order_by=("k", "k2", "k3", "k4", "k5")),
         BG_ERR_INVALID, ["order_by", "5"]),
    "no exprs": (window([]), BG_ERR_INVALID, ["exprs"]),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_node_and_the_offender(name):
    doc, want_rc, words = REFUSALS[name]
    rc, msg = refusal(doc)
    assert rc == want_rc, msg
    assert "window" in msg
    for w in words:
        assert w in msg, (w, msg)
