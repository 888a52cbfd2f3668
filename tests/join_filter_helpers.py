"""What the join-filter suite (test_gpu_join_filter.py) and the nested-loop
join suite (test_gpu_nested_loop_join.py) share word for word: the ABI's
codes, the filter-term builders and the device-table scan node.  Each suite
keeps its own cases, references and handle wrappers.

Not a test module and not a conftest: imported as `join_filter_helpers` from
the tests directory.
"""
import ctypes
import operator

import numpy as np

from datafusion_ballista_amd import gpu, stage

BG_OK, BG_ERR_INVALID = 0, -3
INNER, SEMI, ANTI, OUTER_PROBE = 0, 1, 2, 3
SEMI_BUILD, ANTI_BUILD, OUTER_BUILD, OUTER_FULL = 4, 5, 6, 7
NULL_IDX = 0xFFFFFFFF
SENTINEL = 0xDEADBEEF
I64 = ctypes.c_int64
OPS = {"lt": operator.lt, "le": operator.le, "gt": operator.gt,
       "ge": operator.ge, "eq": operator.eq, "ne": operator.ne}
CMP_CODE = {"lt": gpu.BG_CMP_LT, "le": gpu.BG_CMP_LE, "gt": gpu.BG_CMP_GT,
            "ge": gpu.BG_CMP_GE, "eq": gpu.BG_CMP_EQ, "ne": gpu.BG_CMP_NE}


def bits(flags):
    """bool[n] -> Arrow LSB bitmap, padded like every mask here."""
    n = len(flags)
    out = np.zeros((n + 63) // 64 * 8 + 8, dtype=np.uint8)
    out[:(n + 7) // 8] = np.packbits(flags, bitorder="little")
    return out


def term(kind, group, dtype=0, cmp=0, b=None, bv=None, p=None, pv=None):
    ptr = lambda buf: buf.ptr.value if buf is not None else None  # noqa: E731
    return gpu.BgJoinFilterTerm(kind, group, dtype, cmp, ptr(b), ptr(bv),
                                ptr(p), ptr(pv))


def terms_array(terms):
    return (gpu.BgJoinFilterTerm * max(len(terms), 1))(*terms)


def scan_of(table, name):
    return {"op": "scan", "schema": stage.schema_json(table.schema),
            "source": {"kind": "device", "table": name}}
