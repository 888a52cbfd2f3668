"""CPU-side checks (no GPU) of MIN/MAX over Decimal128, Utf8, Int32 and
Date32: bg_stage_validate types them as the executor runs them (same dtype,
precision and scale as the input, in single, partial and final mode),
refuses min/max over a dictionary column as the executor does, and
decode_agg_value reads the I32 and ROW accumulator records."""
import pytest

from datafusion_ballista_amd import gpu, stage

FIELDS = {
    "d15": {"dtype": "decimal128", "precision": 15, "scale": 2},
    "d38": {"dtype": "decimal128", "precision": 38, "scale": 4},
    "s": {"dtype": "utf8"},
    "dt": {"dtype": "date32"},
    "i": {"dtype": "int32"},
}


def _scan(fields):
    return {"op": "scan", "schema": fields,
            "source": {"kind": "device", "table": "t"}}


SCAN = _scan([{"name": "k", "dtype": "int64"},
              {"name": "code", "dtype": "dict8"}] +
             [dict(name=n, **f) for n, f in FIELDS.items()])


def _doc(plan):
    return {"job_id": "j", "stage_id": 1, "task_id": 0, "work_dir": "/tmp/w",
            "plan": {"op": "collect", "input": plan}}


def _agg(inp, mode, aggs):
    return _doc({"op": "hash_aggregate", "mode": mode, "group_by": ["k"],
                 "aggs": aggs, "input": inp})


def _field(res, name):
    f = dict(next(f for f in res["schema"] if f["name"] == name))
    del f["name"]
    return f


@pytest.mark.parametrize("col", sorted(FIELDS))
@pytest.mark.parametrize("fn", ["min", "max"])
def test_single_keeps_input_type(col, fn):
    res = stage.validate(_agg(SCAN, "single", [
        {"fn": fn, "as": "m", "expr": {"col": col}}]))
    assert res["ok"] is True
    assert [f["name"] for f in res["schema"]] == ["k", "m"]
    assert _field(res, "m") == FIELDS[col]


@pytest.mark.parametrize("col", sorted(FIELDS))
@pytest.mark.parametrize("fn", ["min", "max"])
def test_partial_adds_count_and_final_reads_it_back(col, fn):
    res = stage.validate(_agg(SCAN, "partial", [
        {"fn": fn, "as": "m", "expr": {"col": col}}]))
    assert [f["name"] for f in res["schema"]] == ["k", "m", "m$n"]
    assert _field(res, "m") == FIELDS[col]
    assert _field(res, "m$n") == {"dtype": "int64"}
    # final over exactly the schema that partial emits
    fin = stage.validate(_agg(_scan(res["schema"]), "final",
                              [{"fn": fn, "as": "m"}]))
    assert [f["name"] for f in fin["schema"]] == ["k", "m"]
    assert _field(fin, "m") == FIELDS[col]


@pytest.mark.parametrize("mode", ["single", "partial"])
@pytest.mark.parametrize("fn", ["min", "max"])
def test_dict8_is_rejected_as_the_executor_rejects_it(fn, mode):
    """A dictionary code has no value order: the executor answers
    BG_ERR_UNSUPPORTED (-4), so validation must too."""
    doc = _agg(SCAN, mode, [{"fn": fn, "as": "m", "expr": {"col": "code"}}])
    with pytest.raises(RuntimeError, match=r"rc=-4.*min/max over dict8"):
        stage.validate(doc)


def test_final_over_dict8_partial_is_rejected():
    part = _scan([{"name": "k", "dtype": "int64"},
                  {"name": "m", "dtype": "dict8"},
                  {"name": "m$n", "dtype": "int64"}])
    with pytest.raises(RuntimeError, match=r"rc=-4"):
        stage.validate(_agg(part, "final", [{"fn": "min", "as": "m"}]))


def test_existing_minmax_still_validate():
    res = stage.validate(_agg(
        _scan([{"name": "k", "dtype": "int64"},
               {"name": "f", "dtype": "float64"}]), "single",
        [{"fn": "min", "as": "a", "expr": {"col": "k"}},
         {"fn": "max", "as": "b", "expr": {"col": "f"}},
         {"fn": "count", "as": "c"}]))
    assert [f["dtype"] for f in res["schema"]] == ["int64", "int64",
                                                   "float64", "int64"]


def _acc(word0, word1=0):
    return word0.to_bytes(8, "little") + word1.to_bytes(8, "little")


def test_decode_i32_ops_as_their_i64_counterparts():
    for v in (-2**31, 2**31 - 1, -1, 0, 1, 19000):
        enc_max = (v & (2**64 - 1)) ^ (1 << 63)
        assert gpu.decode_agg_value(gpu.BG_AGG_OP_MAX_I32, _acc(enc_max)) == v
        assert gpu.decode_agg_value(gpu.BG_AGG_OP_MAX_I64, _acc(enc_max)) == v
        enc_min = ~enc_max & (2**64 - 1)
        assert gpu.decode_agg_value(gpu.BG_AGG_OP_MIN_I32, _acc(enc_min)) == v
        assert gpu.decode_agg_value(gpu.BG_AGG_OP_MIN_I64, _acc(enc_min)) == v


def test_decode_row_ops():
    for op in (gpu.BG_AGG_OP_MIN_ROW, gpu.BG_AGG_OP_MAX_ROW):
        assert gpu.decode_agg_value(op, _acc(0)) is None
        assert gpu.decode_agg_value(op, _acc(1)) == 0
        assert gpu.decode_agg_value(op, _acc(2**32)) == 2**32 - 1


def test_op_numbers_match_the_header():
    assert (gpu.BG_AGG_OP_MIN_I32, gpu.BG_AGG_OP_MAX_I32,
            gpu.BG_AGG_OP_MIN_ROW, gpu.BG_AGG_OP_MAX_ROW) == (7, 8, 9, 10)
