"""CPU-side checks (no GPU) of hash_join's residual "filter" in the plan
grammar: bg_stage_validate accepts the q21, q7 and q19 filter shapes on all
eight join types and reports the schema of the unfiltered join, and refuses
every malformed filter with a message that names the offender."""
import copy

import pytest

from datafusion_ballista_amd import stage

DEC = {"dtype": "decimal128", "precision": 15, "scale": 2}
BUILD = {"op": "scan",
         "schema": [{"name": "b_key", "dtype": "int64"},
                    {"name": "b_supp", "dtype": "int64"},
                    {"name": "b_name", "dtype": "utf8"},
                    {"name": "b_brand", "dtype": "utf8"},
                    {"name": "b_size", "dtype": "int32"},
                    {"name": "b_date", "dtype": "date32"},
                    {"name": "b_qty", **DEC},
                    {"name": "b_qty4", "dtype": "decimal128",
                     "precision": 15, "scale": 4},
                    {"name": "b_f", "dtype": "float64"}],
         "source": {"kind": "device", "table": "b"}}
PROBE = {"op": "scan",
         "schema": [{"name": "p_key", "dtype": "int64"},
                    {"name": "p_supp", "dtype": "int64"},
                    {"name": "p_name", "dtype": "utf8"},
                    {"name": "p_mode", "dtype": "utf8"},
                    {"name": "p_date", "dtype": "date32"},
                    {"name": "p_qty", **DEC},
                    {"name": "p_f", "dtype": "float64"}],
         "source": {"kind": "device", "table": "p"}}

JOIN_TYPES = ["inner", "semi", "anti", "left", "semi_build", "anti_build",
              "outer_build", "full"]

# approved/q21.txt:60-61  filter=l_suppkey@1 != l_suppkey@0
Q21 = {"any": [{"cross": [{"build": "b_supp", "cmp": "ne",
                           "probe": "p_supp"}]}]}
# q7: n_name = FRANCE AND n_name = GERMANY OR n_name = GERMANY AND n_name =
# FRANCE, one literal per side
Q7 = {"any": [
    {"build": [{"col": "b_name", "in": ["FRANCE"]}],
     "probe": [{"col": "p_name", "in": ["GERMANY"]}]},
    {"build": [{"col": "b_name", "in": ["GERMANY"]}],
     "probe": [{"col": "p_name", "in": ["FRANCE"]}]}]}
# q19: three ANDs of brand / container / quantity / size tests on one side
# and shipmode / quantity tests on the other
Q19 = {"any": [
    {"build": [{"col": "b_brand", "in": ["Brand#12"]},
               {"col": "b_name", "in": ["SM CASE", "SM BOX"]},
               {"col": "b_size", "cmp": "between", "lo": 1, "hi": 5}],
     "probe": [{"col": "p_qty", "cmp": "between", "lo": 100, "hi": 1100}]},
    {"build": [{"col": "b_brand", "in": ["Brand#23"]},
               {"col": "b_size", "cmp": "between", "lo": 1, "hi": 10}],
     "probe": [{"col": "p_qty", "cmp": "between", "lo": 1000, "hi": 2000},
               {"col": "p_mode", "like": "AIR%"}]},
    {"build": [{"col": "b_brand", "in": ["Brand#34"]},
               {"col": "b_size", "cmp": "between", "lo": 1, "hi": 15}],
     "probe": [{"col": "p_qty", "cmp": "between", "lo": 2000, "hi": 3000}]}]}


def _doc(jt, filt=None):
    both = jt not in ("semi_build", "anti_build")
    output = [{"side": "build", "col": "b_key"},
              {"side": "build", "col": "b_qty", "as": "qty"}]
    if both:
        output.append({"side": "probe", "col": "p_date"})
    join = {"op": "hash_join", "build": BUILD, "probe": PROBE,
            "build_keys": ["b_key"], "probe_keys": ["p_key"],
            "join_type": jt, "output": output}
    if filt is not None:
        join["filter"] = filt
    return {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
            "plan": {"op": "collect", "input": join}}


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("filt", [Q21, Q7, Q19], ids=["q21", "q7", "q19"])
def test_validate_accepts_filter_with_unfiltered_schema(jt, filt):
    plain = stage.validate(_doc(jt))
    res = stage.validate(_doc(jt, filt))
    assert res["ok"] is True
    assert res["schema"] == plain["schema"]
    # the filter's columns (b_supp, p_supp, b_name, ...) are not outputs
    assert [f["name"] for f in res["schema"]][:2] == ["b_key", "qty"]


def cross(b, cmp, p):
    return {"any": [{"cross": [{"build": b, "cmp": cmp, "probe": p}]}]}


REFUSALS = {
    "build_pred_names_probe_column":
        ({"any": [{"build": [{"col": "p_mode", "in": ["AIR"]}]}]},
         ["p_mode", "build", "probe side"]),
    "probe_pred_names_build_column":
        ({"any": [{"probe": [{"col": "b_size", "cmp": "lt", "hi": 3}]}]},
         ["b_size", "probe", "build side"]),
    "pred_names_column_of_neither_side":
        ({"any": [{"build": [{"col": "zzz", "cmp": "lt", "hi": 3}]}]},
         ["zzz", "neither"]),
    "pred_rhs_names_other_side":
        ({"any": [{"build": [{"col": "b_date", "cmp": "lt",
                              "rhs": {"col": "p_date"}}]}]},
         ["p_date", "probe side"]),
    "cross_build_column_is_a_probe_column":
        (cross("p_supp", "ne", "p_supp"), ["p_supp", "build"]),
    "cross_probe_column_unknown":
        (cross("b_supp", "ne", "nope"), ["nope", "probe"]),
    "cross_dtype_mismatch":
        (cross("b_supp", "ne", "p_date"),
         ["b_supp", "int64", "p_date", "date32", "dtype"]),
    "cross_scale_mismatch":
        (cross("b_qty4", "lt", "p_qty"), ["b_qty4", "p_qty", "scale", "4", "2"]),
    "cross_utf8":
        (cross("b_name", "eq", "p_name"), ["b_name", "p_name", "utf8"]),
    "cross_float64":
        (cross("b_f", "lt", "p_f"), ["b_f", "p_f", "float64"]),
    "cross_unknown_cmp":
        (cross("b_supp", "neq", "p_supp"), ["neq"]),
    "empty_any": ({"any": []}, ["empty", "any"]),
    "empty_group":
        ({"any": [Q21["any"][0], {}]}, ["group 1", "empty"]),
    "empty_group_of_empty_lists":
        ({"any": [{"build": [], "probe": [], "cross": []}]},
         ["group 0", "empty"]),
    "five_groups": ({"any": [Q21["any"][0]] * 5}, ["5 groups", "4"]),
    "five_cross_terms":
        ({"any": [{"cross": Q21["any"][0]["cross"] * 5}]},
         ["group 0", "5 cross", "4"]),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_validate_refuses_and_names_the_offender(case):
    filt, needles = REFUSALS[case]
    for jt in ("inner", "semi_build"):
        msg = stage.validate_error(_doc(jt, copy.deepcopy(filt)))
        assert msg, f"{case}: accepted"
        for needle in needles:
            assert needle in msg, (case, needle, msg)


def test_four_groups_and_four_cross_terms_are_accepted():
    g = {"cross": Q21["any"][0]["cross"] * 4,
         "build": [{"col": "b_size", "cmp": "lt", "hi": 3}]}
    assert stage.validate(_doc("full", {"any": [g] * 4}))["ok"] is True


def test_every_cross_dtype_and_cmp_is_accepted():
    for b, p in (("b_supp", "p_supp"), ("b_date", "p_date"),
                 ("b_qty", "p_qty")):
        for cmp in ("lt", "le", "gt", "ge", "eq", "ne"):
            assert stage.validate(_doc("anti", cross(b, cmp, p)))["ok"] is True
