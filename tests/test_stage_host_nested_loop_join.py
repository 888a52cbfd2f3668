"""CPU-side checks (no GPU) of the nested_loop_join node in the plan grammar
(DataFusion NestedLoopJoinExec: a join without keys whose residual filter
alone decides): bg_stage_validate accepts the q11 and q22 filters, a band
filter and no filter at all on all eight join types with the schema a
hash_join of the same sides reports, and refuses keys on the node, unknown
join types, probe outputs of a build-rows-only type and every malformed
filter with a message that names the node and the offender."""
import copy
import ctypes
import json

import pytest

from datafusion_ballista_amd import gpu, stage

BG_ERR_INVALID, BG_ERR_UNSUPPORTED = -3, -4
D38 = {"dtype": "decimal128", "precision": 38, "scale": 15}
D19 = {"dtype": "decimal128", "precision": 19, "scale": 6}
# build: the scalar subquery's single row (q11: sum * 0.0001, q22: avg) next
# to a band's bounds; probe: the rows it is attached to
BUILD = {"op": "scan",
         "schema": [{"name": "b_thr38", **D38},
                    {"name": "b_avg", **D19},
                    {"name": "b_lo", "dtype": "int64"},
                    {"name": "b_hi", "dtype": "int64"},
                    {"name": "b_f", "dtype": "float64"},
                    {"name": "b_name", "dtype": "utf8"}],
         "source": {"kind": "device", "table": "b"}}
PROBE = {"op": "scan",
         "schema": [{"name": "p_key", "dtype": "int64"},
                    {"name": "p_val38", **D38},
                    {"name": "p_bal", "dtype": "decimal128", "precision": 15,
                     "scale": 2},
                    {"name": "p_bal19", **D19},
                    {"name": "p_x", "dtype": "int64"},
                    {"name": "p_f", "dtype": "float64"},
                    {"name": "p_phone", "dtype": "utf8"}],
         "source": {"kind": "device", "table": "p"}}

JOIN_TYPES = ["inner", "semi", "anti", "left", "semi_build", "anti_build",
              "outer_build", "full"]


def cross(*terms):
    return {"any": [{"cross": [{"build": b, "cmp": c, "probe": p}
                               for b, c, p in terms]}]}


# approved/q11.txt:69  filter=join_proj_push_down_1@1 > sum(..) * 0.0001@0
Q11 = cross(("b_thr38", "lt", "p_val38"))
# approved/q22.txt:14  filter=join_proj_push_down_1@1 > avg(c_acctbal)@0
Q22 = cross(("b_avg", "lt", "p_bal19"))
# b_lo <= p_x and p_x < b_hi
BAND = cross(("b_lo", "le", "p_x"), ("b_hi", "gt", "p_x"))
FILTERS = {"q11": Q11, "q22": Q22, "band": BAND, "none": None}

BUILD_OUT = [{"side": "build", "col": "b_thr38", "as": "thr"},
             {"side": "build", "col": "b_avg"}]
PROBE_OUT = [{"side": "probe", "col": "p_phone"},
             {"side": "probe", "col": "p_bal"}]
BUILD_SCHEMA = [{"name": "thr", **D38}, {"name": "b_avg", **D19}]
PROBE_SCHEMA = [{"name": "p_phone", "dtype": "utf8"},
                {"name": "p_bal", "dtype": "decimal128", "precision": 15,
                 "scale": 2}]


def outputs(jt):
    """-> (output list, expected schema) of join type jt."""
    if jt in ("semi_build", "anti_build"):
        return BUILD_OUT, BUILD_SCHEMA
    if jt in ("semi", "anti"):
        return PROBE_OUT, PROBE_SCHEMA
    return BUILD_OUT + PROBE_OUT, BUILD_SCHEMA + PROBE_SCHEMA


def _doc(join):
    return {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
            "plan": {"op": "collect", "input": join}}


def nlj(jt, filt=None, **extra):
    join = {"op": "nested_loop_join", "build": BUILD, "probe": PROBE,
            "join_type": jt, "output": outputs(jt)[0]}
    if filt is not None:
        join["filter"] = copy.deepcopy(filt)
    join.update(extra)
    return _doc(join)


def refusal(doc):
    """-> (return code, message) of a plan bg_stage_validate refuses."""
    L = gpu.load_library()
    out = ctypes.c_char_p()
    rc = L.bg_stage_validate(json.dumps(doc).encode(), ctypes.byref(out))
    assert rc != 0, "plan unexpectedly validated"
    return rc, L.bg_last_error().decode()


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("name", sorted(FILTERS))
def test_validate_accepts_with_the_hash_join_schema(jt, name):
    res = stage.validate(nlj(jt, FILTERS[name]))
    assert res["ok"] is True
    assert res["schema"] == outputs(jt)[1]
    # the schema hash_join reports for the same sides, type and outputs
    keyed = nlj(jt, FILTERS[name])
    keyed["plan"]["input"].update(op="hash_join", build_keys=["b_lo"],
                                  probe_keys=["p_key"])
    assert stage.validate(keyed)["schema"] == res["schema"]


def test_probe_chunk_rows_is_accepted():
    assert stage.validate(nlj("full", BAND, probe_chunk_rows=64))["ok"] is True


@pytest.mark.parametrize("keys", [{"build_keys": ["b_lo"]},
                                  {"probe_keys": ["p_key"]},
                                  {"build_keys": ["b_lo"],
                                   "probe_keys": ["p_key"]},
                                  {"build_keys": []}])
def test_keys_on_the_node_are_refused(keys):
    rc, msg = refusal(nlj("inner", Q22, **keys))
    assert rc == BG_ERR_INVALID
    assert "nested_loop_join" in msg and sorted(keys)[0] in msg
    assert "hash_join" in msg              # the node for keyed joins


def test_unknown_join_type_is_refused():
    for jt in ("left_mark", "cross"):
        doc = nlj("inner", Q11)
        doc["plan"]["input"]["join_type"] = jt
        rc, msg = refusal(doc)
        assert rc == BG_ERR_UNSUPPORTED
        assert "nested_loop_join" in msg and jt in msg
        assert "hash_join" not in msg


@pytest.mark.parametrize("jt", ["semi_build", "anti_build"])
def test_build_rows_only_type_refuses_a_probe_output(jt):
    doc = nlj(jt, Q22)
    doc["plan"]["input"]["output"] = BUILD_OUT + PROBE_OUT[:1]
    rc, msg = refusal(doc)
    assert rc == BG_ERR_INVALID
    for needle in ("nested_loop_join", jt, "p_phone", "build"):
        assert needle in msg, (needle, msg)
    assert "hash_join" not in msg


REFUSALS = {
    "cross_float64": (cross(("b_f", "lt", "p_f")), BG_ERR_UNSUPPORTED,
                      ["b_f", "p_f", "float64"]),
    "cross_utf8": (cross(("b_name", "eq", "p_phone")), BG_ERR_UNSUPPORTED,
                   ["b_name", "p_phone", "utf8"]),
    "cross_scale_mismatch": (cross(("b_avg", "lt", "p_bal")), BG_ERR_INVALID,
                             ["b_avg", "p_bal", "scale", "6", "2"]),
    "cross_dtype_mismatch": (cross(("b_lo", "lt", "p_bal")), BG_ERR_INVALID,
                             ["b_lo", "int64", "p_bal", "decimal128"]),
    "cross_build_column_is_a_probe_column":
        (cross(("p_x", "lt", "p_x")), BG_ERR_INVALID, ["p_x", "build"]),
    "cross_unknown_cmp": (cross(("b_lo", "neq", "p_x")), BG_ERR_INVALID,
                          ["neq"]),
    "five_groups": ({"any": [Q22["any"][0]] * 5}, BG_ERR_UNSUPPORTED,
                    ["5 groups", "4"]),
    "five_cross_terms": ({"any": [{"cross": Q22["any"][0]["cross"] * 5}]},
                         BG_ERR_UNSUPPORTED, ["group 0", "5 cross", "4"]),
    "empty_any": ({"any": []}, BG_ERR_INVALID, ["empty", "any"]),
    "empty_group": ({"any": [Q22["any"][0], {}]}, BG_ERR_INVALID,
                    ["group 1", "empty"]),
    "build_pred_names_probe_column":
        ({"any": [{"build": [{"col": "p_x", "cmp": "lt", "hi": 3}]}]},
         BG_ERR_INVALID, ["p_x", "build", "probe side"]),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_filter_refusals_name_the_node_and_the_offender(case):
    filt, want_rc, needles = REFUSALS[case]
    for jt in ("inner", "anti_build"):
        rc, msg = refusal(nlj(jt, filt))
        assert rc == want_rc, (case, rc, msg)
        assert "nested_loop_join filter:" in msg, msg
        assert "hash_join" not in msg, msg
        for needle in needles:
            assert needle in msg, (case, needle, msg)
