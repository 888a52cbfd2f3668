"""CPU-side checks (no GPU) of the build-side-preserving join types in the
plan grammar: bg_stage_validate accepts semi_build / anti_build /
outer_build / full with the right output schema, refuses probe-side
outputs where only build rows are emitted, and still refuses unknown
types."""
import pytest

from datafusion_ballista_amd import stage

BUILD = {"op": "scan",
         "schema": [{"name": "c_custkey", "dtype": "int64"},
                    {"name": "c_name", "dtype": "utf8"},
                    {"name": "c_acctbal", "dtype": "decimal128",
                     "precision": 15, "scale": 2}],
         "source": {"kind": "device", "table": "c"}}
PROBE = {"op": "scan",
         "schema": [{"name": "o_orderkey", "dtype": "int64"},
                    {"name": "o_custkey", "dtype": "int64"},
                    {"name": "o_orderdate", "dtype": "date32"}],
         "source": {"kind": "device", "table": "o"}}


def _doc(join_type, output):
    return {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
            "plan": {"op": "collect", "input": {
                "op": "hash_join", "build": BUILD, "probe": PROBE,
                "build_keys": ["c_custkey"], "probe_keys": ["o_custkey"],
                "join_type": join_type, "output": output}}}


@pytest.mark.parametrize("jt", ["semi_build", "anti_build"])
def test_validate_build_rows_only_types(jt):
    res = stage.validate(_doc(jt, [
        {"side": "build", "col": "c_custkey"},
        {"side": "build", "col": "c_acctbal", "as": "bal"},
        {"side": "build", "col": "c_name"}]))
    assert res["ok"] is True
    assert [f["name"] for f in res["schema"]] == ["c_custkey", "bal", "c_name"]
    assert [f["dtype"] for f in res["schema"]] == \
        ["int64", "decimal128", "utf8"]


@pytest.mark.parametrize("jt", ["outer_build", "full"])
def test_validate_outer_types_take_both_sides(jt):
    res = stage.validate(_doc(jt, [
        {"side": "build", "col": "c_custkey"},
        {"side": "probe", "col": "o_orderkey"},
        {"side": "probe", "col": "o_orderdate", "as": "od"},
        {"side": "build", "col": "c_name"}]))
    assert res["ok"] is True
    assert [f["name"] for f in res["schema"]] == \
        ["c_custkey", "o_orderkey", "od", "c_name"]
    assert [f["dtype"] for f in res["schema"]] == \
        ["int64", "int64", "date32", "utf8"]


@pytest.mark.parametrize("jt", ["semi_build", "anti_build"])
def test_validate_rejects_probe_output_for_build_rows_only(jt):
    msg = stage.validate_error(_doc(jt, [
        {"side": "build", "col": "c_custkey"},
        {"side": "probe", "col": "o_orderkey"}]))
    assert jt in msg and "o_orderkey" in msg and "build" in msg


def test_validate_still_rejects_unknown_type():
    msg = stage.validate_error(_doc("right", [
        {"side": "build", "col": "c_custkey"}]))
    assert "right" in msg


def test_validate_existing_types_unchanged():
    for jt in ("inner", "semi", "anti", "left"):
        res = stage.validate(_doc(jt, [
            {"side": "probe", "col": "o_orderkey"}]))
        assert res["ok"] is True
