"""ctypes host bindings for libballista_gpu.so (include/ballista_gpu.h).

The GpuStageContext owns device memory for one task's columns and exposes
the hot-path ops.  It fails loudly (RuntimeError) when the HIP extension or
the GPU is missing — no CPU fallback exists on the product path.

The ABI is stated once here — the constants, the struct classes and the
_SIGNATURES table below — and tests/test_cabi.py checks all three against
the header.  load_library() applies the table as argtypes/restype, so call
sites pass plain Python ints for 64-bit parameters.
"""

import ctypes
import os
import struct as _struct

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))

# ---- constants (mirror include/ballista_gpu.h) ----
BG_DT_INT32 = 1
BG_DT_INT64 = 2
BG_DT_DATE32 = 3
BG_DT_DECIMAL128 = 4
BG_DT_DICT8 = 5
BG_DT_UTF8 = 6
BG_DT_FLOAT64 = 7

BG_PRED_GE_LT = 0
BG_PRED_BETWEEN = 1
BG_PRED_LT = 2
BG_PRED_EQ = 3
BG_PRED_GT = 4

BG_DATE_PART_YEAR = 0
BG_DATE_PART_QUARTER = 1
BG_DATE_PART_MONTH = 2
BG_DATE_PART_DAY = 3
BG_DATE_PART_DOY = 4
BG_DATE_PART_DOW = 5

BG_CMP_LT = 0
BG_CMP_LE = 1
BG_CMP_GT = 2
BG_CMP_GE = 3
BG_CMP_EQ = 4
BG_CMP_NE = 5

BG_JOIN_FILTER_MAX_GROUPS = 4
BG_JOIN_FILTER_MAX_CROSS = 4
BG_JF_CROSS = 0
BG_JF_BUILD_MASK = 1
BG_JF_PROBE_MASK = 2

BG_AGG_OP_SUM_DEC128 = 0
BG_AGG_OP_SUM_I64 = 1
BG_AGG_OP_MIN_I64 = 2
BG_AGG_OP_MAX_I64 = 3
BG_AGG_OP_SUM_F64 = 4
BG_AGG_OP_MIN_F64 = 5
BG_AGG_OP_MAX_F64 = 6
BG_AGG_OP_MIN_I32 = 7  # Int32/Date32, encoded as MIN_I64
BG_AGG_OP_MAX_I32 = 8
BG_AGG_OP_MIN_ROW = 9  # Decimal128/Utf8: acc word 0 = winning row + 1
BG_AGG_OP_MAX_ROW = 10

BG_WIN_ROW_NUMBER = 0
BG_WIN_RANK = 1
BG_WIN_DENSE_RANK = 2
BG_WIN_ROWS = 0
BG_WIN_RANGE = 1
BG_WIN_UNBOUNDED = 0
BG_WIN_CURRENT_ROW = 1
BG_WIN_PRECEDING = 2
BG_WIN_FOLLOWING = 3
BG_WIN_SUM = 0
BG_WIN_COUNT = 1
BG_WIN_MIN = 2
BG_WIN_MAX = 3

BG_PROJ_MUL = 0
BG_PROJ_ADD = 1
BG_PROJ_SUB = 2
BG_PROJ_RSUB_LIT = 3
BG_PROJ_MUL_LIT = 4
BG_PROJ_ADD_LIT = 5

BG_F64_MUL = 0
BG_F64_ADD = 1
BG_F64_SUB = 2
BG_F64_DIV = 3
BG_F64_MUL_LIT = 4
BG_F64_ADD_LIT = 5
BG_F64_LIT_SUB = 6
BG_F64_DIV_LIT = 7
BG_F64_LIT_DIV = 8

BG_LZ4_BLOCK = 65536
BG_LZ4_SLOT_STRIDE = 65544
LZ4_FRAME_HEADER = bytes.fromhex("04224d184040c0")  # magic+FLG+BD+HC

_DT_SIZE = {BG_DT_INT32: 4, BG_DT_DATE32: 4, BG_DT_INT64: 8,
            BG_DT_DECIMAL128: 16, BG_DT_DICT8: 1, BG_DT_FLOAT64: 8}

_NP_TO_DT = {
    np.dtype(np.int32): BG_DT_INT32,
    np.dtype(np.int64): BG_DT_INT64,
    np.dtype(np.uint8): BG_DT_DICT8,
    np.dtype(np.float64): BG_DT_FLOAT64,
}

# ---- structs: class BgFooBar mirrors the header's bg_foo_bar ----
_p, _i32, _u32, _i64 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32,
                        ctypes.c_int64)


class BgColumn(ctypes.Structure):
    _fields_ = [("dtype", _i32), ("precision", _i32), ("scale", _i32),
                ("_pad", _i32), ("d_data", _p), ("d_validity", _p),
                ("d_offsets", _p), ("len", _i64)]


class BgPred(ctypes.Structure):
    _fields_ = [("column", _i32), ("op", _i32), ("lo_lo", _i64),
                ("lo_hi", _i64), ("hi_lo", _i64), ("hi_hi", _i64)]


class BgSnappyPage(ctypes.Structure):
    _fields_ = [("d_src", _p), ("d_dst", _p), ("src_len", _i64),
                ("dst_cap", _i64)]


class BgPageExtractJob(ctypes.Structure):
    _fields_ = [("d_page", _p), ("d_out", _p), ("page_len", _i64),
                ("nvals", _i64), ("src_esz", _i64), ("has_def", _i32),
                ("flba_reverse", _i32), ("d_vidx", _p), ("d_n_present", _p)]


class BgDictIndicesJob(ctypes.Structure):
    _fields_ = [("d_page", _p), ("d_out_idx", _p), ("page_len", _i64),
                ("nvals", _i64), ("has_def", _i32), ("_pad", _i32),
                ("d_vidx", _p), ("d_n_present", _p), ("d_dense", _p)]


class BgDefLevelsJob(ctypes.Structure):
    _fields_ = [("d_page", _p), ("d_vidx", _p), ("d_valid_out", _p),
                ("page_len", _i64), ("nvals", _i64), ("bit_off", _i64),
                ("d_n_present", _p)]


class BgListLevelsJob(ctypes.Structure):
    _fields_ = [("d_page", _p), ("page_len", _i64), ("nslots", _i64),
                ("max_def", _i32), ("def_entry", _i32), ("def_valid", _i32),
                ("_pad", _i32), ("row_base", _i64), ("entry_base", _i64),
                ("d_counts", _p), ("d_row_sizes", _p), ("d_list_valid", _p),
                ("d_elem_valid", _p), ("d_vidx", _p)]


class BgBaPageJob(ctypes.Structure):
    _fields_ = [("d_page", _p), ("d_lens_out", _p), ("d_srcaddr_out", _p),
                ("page_len", _i64), ("nvals", _i64), ("has_def", _i32),
                ("_pad", _i32), ("d_vidx", _p), ("d_n_present", _p)]


class BgDeltaBpJob(ctypes.Structure):
    _fields_ = [("d_page", _p), ("d_out", _p), ("page_len", _i64),
                ("nvals", _i64), ("esz", _i64), ("has_def", _i32),
                ("_pad", _i32), ("d_vidx", _p), ("d_n_present", _p)]


class BgDeltaBaJob(ctypes.Structure):
    _fields_ = [("d_page", _p), ("d_lens_out", _p), ("d_srcaddr_out", _p),
                ("d_offs32", _p), ("d_data_out", _p), ("page_len", _i64),
                ("nvals", _i64), ("has_def", _i32), ("enc", _i32),
                ("d_vidx", _p), ("d_n_present", _p)]


class BgLz4BlockJob(ctypes.Structure):
    _fields_ = [("d_src", _p), ("d_dst_slot", _p), ("blen", _i32),
                ("_pad", _i32)]


class BgLz4Frame(ctypes.Structure):
    _fields_ = [("d_src", _p), ("d_dst", _p), ("src_len", _i64),
                ("dst_cap", _i64)]


class BgPackJob(ctypes.Structure):
    _fields_ = [("d_src", _p), ("d_dst", _p), ("nbytes", _i64),
                ("size_word", _u32), ("_pad", _u32)]


class BgJoinFilterTerm(ctypes.Structure):
    _fields_ = [("kind", _i32), ("group", _i32), ("dtype", _i32),
                ("cmp", _i32), ("d_build", _p), ("d_build_validity", _p),
                ("d_probe", _p), ("d_probe_validity", _p)]


# ---- function signatures: "<return> <one code per parameter>" ----
# Every data pointer is a c_void_p, which takes None, an int address, a
# c_void_p, byref(...), a ctypes array or a POINTER instance alike.
_CODES = {
    "v": None,
    "i": ctypes.c_int32, "u": ctypes.c_uint32,
    "l": ctypes.c_int64, "L": ctypes.c_uint64,
    "d": ctypes.c_double,
    "p": ctypes.c_void_p,                  # any data pointer
    "s": ctypes.c_char_p,                  # [const] char*
    "S": ctypes.POINTER(ctypes.c_char_p),  # char** / const char* const*
    "P": ctypes.POINTER(ctypes.c_void_p),  # void** / void* const*
}

_SIGNATURES = {
    "bg_last_error": "s", "bg_version": "i", "bg_source_hash": "s",
    "bg_last_kernel_ms": "d", "bg_init": "i i", "bg_device_count": "i p",
    "bg_synchronize": "i", "bg_malloc": "i LP", "bg_free": "i p",
    "bg_memset": "i piL", "bg_memcpy_h2d": "i ppL", "bg_memcpy_d2h": "i ppL",
    "bg_memcpy_dtod": "i ppL", "bg_pool_trim": "i", "bg_pool_stats": "i ppp",
    "bg_eval_predicates": "i pipilp", "bg_mask_to_indices": "i plpp",
    "bg_gather": "i plplp", "bg_gather_varlen": "i ppplpplp",
    "bg_sub_i32": "i plip", "bg_gather_bits": "i pplp",
    "bg_eval_like": "i pSpiiiilp", "bg_select": "i pppllp",
    "bg_fill_const": "i pllll", "bg_eval_in": "i ppilp",
    "bg_bitmap_or": "i pplp", "bg_date_part": "i pilp",
    "bg_substr": "i plillpplp", "bg_eval_compare_cols": "i ppilp",
    "bg_eval_in_utf8": "i pSpilp", "bg_hash_columns": "i pilp",
    "bg_partition_ids": "i plup", "bg_partition_indices": "i plupp",
    "bg_partition_indices_ex": "i pluppp", "bg_scatter_rows": "i plplp",
    "bg_hash_repartition": "i pipiluppP", "bg_hashjoin_build": "i plP",
    "bg_hashjoin_probe_count": "i pplp", "bg_hashjoin_probe_fill": "i pplpp",
    "bg_hashjoin_free": "i p", "bg_hashjoin_build2": "i pilP",
    "bg_hashjoin_probe_count2": "i ppilip",
    "bg_hashjoin_probe_fill2": "i ppilipp", "bg_hashjoin_free2": "i p",
    "bg_hashjoin_probe_mark2": "i ppil", "bg_hashjoin_build_rows2": "i pipp",
    "bg_hashjoin_probe_count2_filtered": "i ppilipip",
    "bg_hashjoin_probe_fill2_filtered": "i ppilipipp",
    "bg_hashjoin_probe_mark2_filtered": "i ppilpi",
    "bg_nljoin_open": "i lP", "bg_nljoin_count": "i plipip",
    "bg_nljoin_fill": "i plipipp", "bg_nljoin_mark": "i plpi",
    "bg_nljoin_build_rows": "i pipp", "bg_nljoin_free": "i p",
    "bg_idx_sentinel": "i plpp", "bg_bitmap_and": "i pplp",
    "bg_hashagg": "i pippipllpppp", "bg_hashagg2": "i pippipllppppp",
    "bg_project_dec128": "i ipplllp",
    "bg_cast": "i piiilpp", "bg_project_f64": "i ippdlp",
    "bg_div_dec128": "i ppilpp",
    "bg_project_dec128_multi": "i pippipippilP", "bg_sort_rows": "i ppilp",
    "bg_sort_rows2": "i pppilp", "bg_merge_join": "i plplppp",
    "bg_snappy_decompress": "i plp", "bg_page_extract": "i plplllii",
    "bg_dict_indices": "i pllip", "bg_page_extract_batch": "i pl",
    "bg_dict_indices_batch": "i pl", "bg_def_levels_batch": "i pl",
    "bg_list_levels_batch": "i pli", "bg_ba_extract_batch": "i pl",
    "bg_ba_from_dict": "i pppplpp", "bg_ba_materialize": "i pplpplp",
    "bg_delta_bp_batch": "i pl", "bg_delta_ba_batch": "i pli",
    "bg_bss_batch": "i pl", "bg_lz4_compress": "i plppp",
    "bg_lz4_compress_flat": "i plp", "bg_lz4_decompress": "i plp",
    "bg_pack_blocks": "i pl", "bg_hash_repartition_fused": "i pipilupppP",
    "bg_bitcopy": "i plpl", "bg_agg_materialize": "i plilpplp",
    "bg_agg_winner_rows": "i pllpp",
    "bg_copy_i64_strided": "i pllp", "bg_avg_finalize": "i pliplilpp",
    "bg_window_bounds": "i pipilpppp", "bg_window_rank": "i ipplp",
    "bg_window_frame": "i iililpipppplpp", "bg_window_agg": "i ipppplpp",
    "bg_execute_stage": "i sS", "bg_stage_free": "v s",
    "bg_stage_validate": "i sS", "bg_stage_register_table": "i spSil",
    "bg_stage_unregister_table": "i s", "bg_fill_rand": "i plLlli",
    "bg_q6_agg": "i ppppiilllppp", "bg_q1_agg": "i pppppppipp",
    # csrc/bg_internal.h (exported, not public API)
    "bg_set_error": "i is", "bg_debug_rb_message": "i lpipiliS",
}


def lib_path() -> str:
    return os.path.join(_DIR, "libballista_gpu.so")


_lib = None


def load_library() -> ctypes.CDLL:
    """dlopen the HIP extension and declare every entry point's signature;
    raises if the library is absent or unloadable."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError(
                f"libballista_gpu.so not found at {p}: the MI355X stage "
                "executor requires its HIP extension (run "
                "__graft_entry__.build()); there is no CPU fallback")
        lib = ctypes.CDLL(p)
        for name, sig in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = _CODES[sig[0]]
            fn.argtypes = [_CODES[c] for c in sig[2:]]
        _lib = lib
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        err = load_library().bg_last_error().decode()
        raise RuntimeError(f"{what} failed (rc={rc}): {err}")


def struct_unpack_bits(v: float) -> int:
    """f64 -> its bit pattern as a SIGNED i64 (BgPred bound fields)."""
    return _struct.unpack("<q", _struct.pack("<d", v))[0]


def _split_i128(v: int):
    v = int(v)
    return (ctypes.c_int64(v & 0xFFFFFFFFFFFFFFFF).value,
            ctypes.c_int64((v >> 64) & 0xFFFFFFFFFFFFFFFF).value)


def decode_agg_value(op, raw16: bytes):
    """Accumulator bytes -> python int/float per aggregate op.  A ROW op
    decodes to the winning input row, or None where the group had no
    non-NULL input (word 0 == 0)."""
    if op in (BG_AGG_OP_SUM_DEC128, BG_AGG_OP_SUM_I64):
        return int.from_bytes(raw16, "little", signed=True)
    if op == BG_AGG_OP_SUM_F64:
        return _struct.unpack("<d", raw16[:8])[0]
    enc = int.from_bytes(raw16[:8], "little")
    if op in (BG_AGG_OP_MIN_ROW, BG_AGG_OP_MAX_ROW):
        return enc - 1 if enc else None
    if op in (BG_AGG_OP_MIN_F64, BG_AGG_OP_MAX_F64):
        if op == BG_AGG_OP_MIN_F64:
            enc = ~enc & 0xFFFFFFFFFFFFFFFF
        bits = (~enc & 0xFFFFFFFFFFFFFFFF) if not (enc >> 63) \
            else enc ^ (1 << 63)
        return _struct.unpack("<d", _struct.pack("<Q", bits))[0]
    if op in (BG_AGG_OP_MAX_I64, BG_AGG_OP_MAX_I32):
        v = enc ^ (1 << 63)
    else:  # MIN_I64, MIN_I32
        v = (~enc & 0xFFFFFFFFFFFFFFFF) ^ (1 << 63)
    return v - (1 << 64) if v >= 1 << 63 else v


def lz4_frame_assemble(sizes, slot_bytes: bytes, length: int) -> bytes:
    """Host glue: device block slots -> one LZ4 frame (constant header,
    [u32 size] blocks — high bit = stored — end mark)."""
    out = [LZ4_FRAME_HEADER]
    for i, sz in enumerate(sizes):
        base = i * BG_LZ4_SLOT_STRIDE
        blen = min(BG_LZ4_BLOCK, length - i * BG_LZ4_BLOCK)
        if sz < 0:  # stored raw
            out.append(_struct.pack("<I", blen | 0x80000000))
            out.append(slot_bytes[base:base + blen])
        else:
            out.append(_struct.pack("<I", int(sz)))
            out.append(slot_bytes[base:base + int(sz)])
    out.append(b"\x00\x00\x00\x00")
    return b"".join(out)


class DeviceBuffer:
    """Caller-owned device allocation."""

    def __init__(self, ctx, nbytes: int):
        self._ctx = ctx
        self._owns = True
        self.nbytes = nbytes
        ptr = ctypes.c_void_p()
        _check(ctx.L.bg_malloc(nbytes, ctypes.byref(ptr)), "bg_malloc")
        self.ptr = ptr

    def at(self, byte_off: int) -> int:
        """Device address `byte_off` bytes into the buffer, as an int (what
        a pointer parameter or a job struct's pointer field takes)."""
        return self.ptr.value + byte_off

    def free(self):
        if self.ptr and self.ptr.value:
            self._ctx.L.bg_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        # return the buffer to the allocator pool when the last reference
        # dies — without this every stage leaks its temporaries and later
        # allocations pay fresh multi-GB hipMallocs (~100 ms/GB) instead
        # of a free-list hit.  Only buffers WE allocated: wrapper objects
        # built with __new__ around borrowed pointers (torch tensors) have
        # no _owns flag and must never be freed here.
        if not getattr(self, "_owns", False):
            return
        try:
            self.free()
        except Exception:
            pass  # interpreter shutdown: the library may already be gone

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        _check(self._ctx.L.bg_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes),
               "bg_memcpy_h2d")
        return self

    def download(self, dtype, count) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        _check(self._ctx.L.bg_memcpy_d2h(out.ctypes.data, self.ptr,
                                         out.nbytes), "bg_memcpy_d2h")
        return out


class GpuStageContext:
    """One GPU-backed task context (one process per GPU; the device ordinal
    is normally fixed by HIP_VISIBLE_DEVICES, SURVEY.md §2 executor row)."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        _check(self.L.bg_init(device), "bg_init")

    # ---- memory ----
    def alloc(self, nbytes: int) -> DeviceBuffer:
        # ownership lives with the returned DeviceBuffer (__del__ returns
        # it to the pool when the last reference dies) — pinning every
        # allocation on the context kept multi-GB stage temporaries alive
        # for the context's whole life, so long pipelines paid fresh
        # hipMallocs instead of pool hits
        return DeviceBuffer(self, nbytes)

    def upload(self, arr: np.ndarray) -> DeviceBuffer:
        return self.alloc(arr.nbytes).upload(arr)

    def close(self):
        pass  # buffers free themselves via DeviceBuffer.__del__

    def synchronize(self):
        _check(self.L.bg_synchronize(), "bg_synchronize")

    def pool_stats(self):
        """(live_bytes, live_buffers, cached_bytes) of the allocator pool."""
        out = (ctypes.c_int64 * 3)()
        _check(self.L.bg_pool_stats(
            ctypes.byref(out, 0), ctypes.byref(out, 8),
            ctypes.byref(out, 16)), "bg_pool_stats")
        return tuple(out)

    # ---- columns ----
    def column(self, dtype: int, buf: DeviceBuffer, n: int,
               validity: DeviceBuffer = None, precision=0, scale=0,
               offsets: DeviceBuffer = None) -> BgColumn:
        col = BgColumn(dtype, precision, scale, 0, buf.ptr,
                       validity.ptr if validity else None,
                       offsets.ptr if offsets else None, n)
        # the struct carries raw device pointers: keep the backing
        # DeviceBuffers alive as long as the column handle is
        col._keep = (buf, validity, offsets)
        return col

    def upload_utf8_column(self, strings):
        """list[bytes] -> BG_DT_UTF8 column (Arrow i32 offsets + data)."""
        data = b"".join(strings)
        offs = np.zeros(len(strings) + 1, dtype=np.int32)
        for i, b in enumerate(strings):
            offs[i + 1] = offs[i] + len(b)
        dbuf = self.upload(np.frombuffer(data, dtype=np.uint8)
                           if data else np.zeros(1, dtype=np.uint8))
        obuf = self.upload(offs)
        return self.column(BG_DT_UTF8, dbuf, len(strings), offsets=obuf)

    def upload_column(self, arr: np.ndarray, dtype: int = None,
                      validity: np.ndarray = None):
        """Fixed-width column upload; Decimal128 arrives as raw 16-B rows."""
        if dtype is None:
            dtype = _NP_TO_DT[arr.dtype]
        buf = self.upload(arr)
        vbuf = self.upload(validity) if validity is not None else None
        n = arr.nbytes // _DT_SIZE[dtype]
        return self.column(dtype, buf, n, vbuf), buf

    # ---- filter / gather ----
    def eval_predicates(self, cols, preds, n: int) -> DeviceBuffer:
        """cols: list[BgColumn]; preds: list[(col, op, lo, hi)] with python
        int bounds. Returns the device mask (ceil(n/64)*8 bytes)."""
        nwords = (n + 63) // 64
        mask = self.alloc(max(nwords * 8, 8))
        carr = (BgColumn * len(cols))(*cols)
        parr = (BgPred * len(preds))()
        for i, (c, op, lo, hi) in enumerate(preds):
            if isinstance(lo, float) or isinstance(hi, float):
                lo_lo = struct_unpack_bits(float(lo))
                hi_lo = struct_unpack_bits(float(hi))
                parr[i] = BgPred(c, op, lo_lo, 0, hi_lo, 0)
                continue
            lo_lo, lo_hi = _split_i128(lo)
            hi_lo, hi_hi = _split_i128(hi)
            parr[i] = BgPred(c, op, lo_lo, lo_hi, hi_lo, hi_hi)
        _check(self.L.bg_eval_predicates(carr, len(cols), parr, len(preds),
                                         n, mask.ptr), "bg_eval_predicates")
        return mask

    def mask_to_indices(self, mask: DeviceBuffer, n: int):
        idx = self.alloc(max(4 * n, 4))
        count = ctypes.c_int64()
        _check(self.L.bg_mask_to_indices(mask.ptr, n, idx.ptr,
                                         ctypes.byref(count)),
               "bg_mask_to_indices")
        return idx, count.value

    def gather(self, src: DeviceBuffer, elem_size: int, idx: DeviceBuffer,
               m: int) -> DeviceBuffer:
        dst = self.alloc(max(elem_size * m, elem_size))
        _check(self.L.bg_gather(src.ptr, elem_size, idx.ptr, m, dst.ptr),
               "bg_gather")
        return dst

    def gather_varlen(self, src_data: DeviceBuffer, src_offsets: DeviceBuffer,
                      idx: DeviceBuffer, m: int, max_bytes: int):
        """Variable-length take -> (offsets buf i32[m+1], data buf, total)."""
        out_offs = self.alloc(max(4 * (m + 1), 8))
        out_data = self.alloc(max(max_bytes, 1))
        total = ctypes.c_int64()
        _check(self.L.bg_gather_varlen(src_data.ptr, src_offsets.ptr, idx.ptr,
                                       m, out_offs.ptr, out_data.ptr,
                                       max_bytes, ctypes.byref(total)),
               "bg_gather_varlen")
        return out_offs, out_data, total.value

    # ---- scalar expressions ----
    def date_part(self, col: BgColumn, part: int, n: int) -> DeviceBuffer:
        """date_part(part, Date32 column) -> device i32[n] (BG_DATE_PART_*);
        the result shares the input's validity."""
        out = self.alloc(max(4 * n, 4))
        _check(self.L.bg_date_part(ctypes.byref(col), part, n, out.ptr),
               "bg_date_part")
        return out

    def cast(self, col: BgColumn, to_dtype: int, n: int, precision: int = 0,
             scale: int = 0) -> DeviceBuffer:
        """CAST(col AS to_dtype[(precision, scale)]) -> device buffer of n
        target-width rows; shares the input's validity.  Raises with the
        failed-row count when a valid row cannot be represented."""
        out = self.alloc(max(_DT_SIZE.get(to_dtype, 16) * n, 16))
        _check(self.L.bg_cast(ctypes.byref(col), to_dtype, precision, scale,
                              n, out.ptr, None), "bg_cast")
        return out

    def project_f64(self, op: int, a: BgColumn, b: BgColumn, lit: float,
                    n: int) -> DeviceBuffer:
        """Float64 arithmetic (BG_F64_*): a OP b, or a OP lit with b None."""
        out = self.alloc(max(8 * n, 8))
        _check(self.L.bg_project_f64(op, ctypes.byref(a),
                                     ctypes.byref(b) if b is not None
                                     else None, lit, n, out.ptr),
               "bg_project_f64")
        return out

    def div_dec128(self, a: BgColumn, b: BgColumn, mul_pow: int,
                   n: int) -> DeviceBuffer:
        """Decimal128 a / b after scale alignment by 10^mul_pow, truncated
        toward zero.  Raises on a zero divisor or an i128 overflow in a row
        valid in both inputs."""
        out = self.alloc(max(16 * n, 16))
        _check(self.L.bg_div_dec128(ctypes.byref(a), ctypes.byref(b), mul_pow,
                                    n, out.ptr, None), "bg_div_dec128")
        return out

    def substr(self, col: BgColumn, start: int, count: int = None,
               n: int = None):
        """substr(Utf8 column, start[, count]) in code points -> (offsets
        buf i32[n+1], data buf, total bytes); sized exactly first."""
        n = col.len if n is None else n
        has_count, cnt = (0, 0) if count is None else (1, count)
        out_offs = self.alloc(max(4 * (n + 1), 8))
        total = ctypes.c_int64()
        _check(self.L.bg_substr(ctypes.byref(col), start, has_count, cnt, n,
                                out_offs.ptr, None, 0, ctypes.byref(total)),
               "bg_substr(size)")
        out_data = self.alloc(max(total.value, 1))
        _check(self.L.bg_substr(ctypes.byref(col), start, has_count, cnt, n,
                                out_offs.ptr, out_data.ptr, total.value,
                                ctypes.byref(total)), "bg_substr")
        return out_offs, out_data, total.value

    def compare_cols(self, a: BgColumn, b: BgColumn, cmp: int, n: int,
                     mask: DeviceBuffer) -> DeviceBuffer:
        """AND `a <cmp> b` (BG_CMP_*) into the existing device mask."""
        _check(self.L.bg_eval_compare_cols(ctypes.byref(a), ctypes.byref(b),
                                           cmp, n, mask.ptr),
               "bg_eval_compare_cols")
        return mask

    def in_utf8(self, col: BgColumn, values, n: int,
                mask: DeviceBuffer) -> DeviceBuffer:
        """AND `col IN (values)` (list[bytes], exact byte equality) into the
        existing device mask."""
        varr = (ctypes.c_char_p * len(values))(*values)
        larr = (ctypes.c_int32 * len(values))(*[len(v) for v in values])
        _check(self.L.bg_eval_in_utf8(ctypes.byref(col), varr, larr,
                                      len(values), n, mask.ptr),
               "bg_eval_in_utf8")
        return mask

    # ---- hash repartition ----
    def hash_columns(self, key_cols, n: int) -> DeviceBuffer:
        hashes = self.alloc(max(8 * n, 8))
        karr = (BgColumn * len(key_cols))(*key_cols)
        _check(self.L.bg_hash_columns(karr, len(key_cols), n, hashes.ptr),
               "bg_hash_columns")
        return hashes

    def partition_ids(self, hashes: DeviceBuffer, n: int, k: int) -> DeviceBuffer:
        pids = self.alloc(max(4 * n, 4))
        _check(self.L.bg_partition_ids(hashes.ptr, n, k, pids.ptr),
               "bg_partition_ids")
        return pids

    def partition_indices(self, pids: DeviceBuffer, n: int, k: int):
        idx = self.alloc(max(4 * n, 4))
        offs = self.alloc(8 * (k + 1))
        _check(self.L.bg_partition_indices(pids.ptr, n, k, idx.ptr, offs.ptr),
               "bg_partition_indices")
        return idx, offs

    def _payload_outs(self, payload_cols, n: int):
        """One partition-major output buffer per payload column, plus the
        void*[ncols] the repartition entry points take."""
        outs = []
        for c in payload_cols:
            esz = _DT_SIZE[c.dtype]
            outs.append(self.alloc(max(esz * n, esz)))
        optrs = (ctypes.c_void_p * len(outs))(*[b.ptr.value for b in outs])
        return outs, optrs

    def hash_repartition(self, key_cols, payload_cols, n: int, k: int):
        """-> (indices buf, offsets buf, [out bufs partition-major])."""
        idx = self.alloc(max(4 * n, 4))
        offs = self.alloc(8 * (k + 1))
        outs, optrs = self._payload_outs(payload_cols, n)
        karr = (BgColumn * len(key_cols))(*key_cols)
        parr = (BgColumn * len(payload_cols))(*payload_cols)
        _check(self.L.bg_hash_repartition(
            karr, len(key_cols), parr, len(payload_cols), n, k, idx.ptr,
            offs.ptr, optrs), "bg_hash_repartition")
        return idx, offs, outs

    def hash_repartition_fused(self, key_cols, payload_cols, n: int, k: int):
        """Fused one-pass materialiser (k<=64, <=4 fixed-width payload
        cols): same outputs/stable order as hash_repartition."""
        idx = self.alloc(max(4 * n, 4))
        offs = self.alloc(8 * (k + 1))
        rank = self.alloc(max(4 * n, 4))
        outs, optrs = self._payload_outs(payload_cols, n)
        karr = (BgColumn * len(key_cols))(*key_cols)
        parr = (BgColumn * len(payload_cols))(*payload_cols)
        _check(self.L.bg_hash_repartition_fused(
            karr, len(key_cols), parr, len(payload_cols), n, k, idx.ptr,
            offs.ptr, rank.ptr, optrs), "bg_hash_repartition_fused")
        return idx, offs, outs

    # ---- aggregate / project / sort / join ----
    def q6_agg(self, shipdate: BgColumn, discount: BgColumn,
               quantity: BgColumn, price: BgColumn, date_lo: int, date_hi: int,
               disc_lo: int, disc_hi: int, qty_lt: int):
        """-> (count, exact i128 sum as python int)."""
        s_lo = ctypes.c_uint64()
        s_hi = ctypes.c_int64()
        cnt = ctypes.c_int64()
        _check(self.L.bg_q6_agg(ctypes.byref(shipdate), ctypes.byref(discount),
                                ctypes.byref(quantity), ctypes.byref(price),
                                date_lo, date_hi, disc_lo, disc_hi, qty_lt,
                                ctypes.byref(s_lo), ctypes.byref(s_hi),
                                ctypes.byref(cnt)), "bg_q6_agg")
        return cnt.value, (s_hi.value << 64) + s_lo.value

    def q1_agg(self, rf, ls, qty, price, disc, tax, shipdate, date_le: int):
        """-> dict group -> (count, [5 exact i128 sums])."""
        counts = np.zeros(256, dtype=np.int64)
        sums = np.zeros(256 * 5 * 16, dtype=np.uint8)
        _check(self.L.bg_q1_agg(
            ctypes.byref(rf), ctypes.byref(ls), ctypes.byref(qty),
            ctypes.byref(price), ctypes.byref(disc), ctypes.byref(tax),
            ctypes.byref(shipdate), date_le, counts.ctypes.data,
            sums.ctypes.data), "bg_q1_agg")
        out = {}
        raw = sums.reshape(256, 5, 16)
        for g in range(256):
            if counts[g] == 0:
                continue
            vals = [int.from_bytes(bytes(raw[g, a]), "little", signed=True)
                    for a in range(5)]
            out[g] = (int(counts[g]), vals)
        return out

    def hashagg(self, key_cols, agg_cols, agg_ops, n, max_groups,
                mask: DeviceBuffer = None, want_nncnt: bool = False):
        """General hash group-by. -> (first_row u32[g], acc i128 bytes
        [g, naggs], counts i64[g]) as numpy arrays (downloaded); with
        want_nncnt also the per-(group, agg) NON-NULL input counts
        i64[g, naggs] (SQL: SUM/MIN/MAX of an all-NULL group is NULL —
        nncnt 0 marks it)."""
        naggs = len(agg_cols)
        karr = (BgColumn * len(key_cols))(*key_cols)
        aarr = (BgColumn * max(naggs, 1))(*(agg_cols or [BgColumn()]))
        oarr = (ctypes.c_int32 * max(naggs, 1))(*(agg_ops or [0]))
        ng = ctypes.c_int64()
        # auto-grow on table-full (the scheduler's row estimates can be low,
        # like the reference's AQE-fed group estimates); the output buffers
        # grow with the group capacity
        cap = max_groups
        for _ in range(8):
            first = self.alloc(max(4 * cap, 4))
            acc = self.alloc(max(16 * cap * max(naggs, 1), 16))
            counts = self.alloc(max(8 * cap, 8))
            args = [karr, len(key_cols), aarr, oarr, naggs,
                    mask.ptr if mask else None, n, cap, first.ptr, acc.ptr,
                    counts.ptr]
            if want_nncnt:
                nncnt = self.alloc(max(8 * cap * max(naggs, 1), 8))
                rc = self.L.bg_hashagg2(*args, nncnt.ptr, ctypes.byref(ng))
            else:
                rc = self.L.bg_hashagg(*args, ctypes.byref(ng))
            if rc == 0:
                break
            err = self.L.bg_last_error().decode()
            if "table full" not in err or cap >= n:
                _check(rc, "bg_hashagg")
            cap = min(max(cap * 8, 64), max(n, 64))
        else:
            _check(rc, "bg_hashagg")
        g = ng.value
        ret = (first.download(np.uint32, g),
               acc.download(np.uint8, 16 * g * naggs).reshape(g, naggs, 16)
               if naggs else np.zeros((g, 0, 16), dtype=np.uint8),
               counts.download(np.int64, g))
        if want_nncnt:
            nn = nncnt.download(np.int64, g * naggs).reshape(g, naggs) \
                if naggs else np.zeros((g, 0), dtype=np.int64)
            return ret + (nn,)
        return ret

    def agg_winner_rows(self, acc: DeviceBuffer, acc_stride: int,
                        ngroups: int, byte_off: int = 0):
        """MIN_ROW/MAX_ROW records (device, acc_stride bytes apart, the
        first at byte_off) -> (rows u32[ngroups], valid bool[ngroups]) as
        numpy arrays: the winning input row per group (0 where none) and
        whether the group had a non-NULL input."""
        rows = self.alloc(max(4 * ngroups, 4))
        valid = self.alloc(max((ngroups + 7) // 8, 1))
        _check(self.L.bg_agg_winner_rows(acc.at(byte_off), acc_stride,
                                         ngroups, rows.ptr, valid.ptr),
               "bg_agg_winner_rows")
        bits = valid.download(np.uint8, (ngroups + 7) // 8)
        return (rows.download(np.uint32, ngroups),
                np.unpackbits(bits, bitorder="little")[:ngroups].astype(bool))

    def project_dec128(self, op, a: BgColumn, b: BgColumn, lit, n):
        out = self.alloc(max(16 * n, 16))
        lo, hi = _split_i128(lit)
        _check(self.L.bg_project_dec128(op, ctypes.byref(a),
                                        ctypes.byref(b) if b else None,
                                        lo, hi, n, out.ptr),
               "bg_project_dec128")
        return out

    def sort_rows(self, key_cols, descending, n):
        """Stable multi-column ORDER BY -> row permutation DeviceBuffer."""
        perm = self.alloc(max(4 * n, 4))
        karr = (BgColumn * len(key_cols))(*key_cols)
        darr = (ctypes.c_int32 * len(key_cols))(*[1 if d else 0
                                                  for d in descending])
        _check(self.L.bg_sort_rows(karr, darr, len(key_cols), n, perm.ptr),
               "bg_sort_rows")
        return perm

    # ---- window functions over sorted rows; buffers are the caller's ----
    @staticmethod
    def _ptr(buf):
        return buf.ptr if buf is not None else None

    def window_bounds(self, part_cols, order_cols, n, part_start=None,
                      part_end=None, peer_start=None, peer_end=None):
        """Partition / peer-group extents (u32[n] DeviceBuffers, any None)."""
        parr = (BgColumn * max(len(part_cols), 1))(*part_cols)
        oarr = (BgColumn * max(len(order_cols), 1))(*order_cols)
        _check(self.L.bg_window_bounds(
            parr, len(part_cols), oarr, len(order_cols), n,
            self._ptr(part_start), self._ptr(part_end), self._ptr(peer_start),
            self._ptr(peer_end)), "bg_window_bounds")

    def window_rank(self, fn, part_start, peer_start, n, out):
        _check(self.L.bg_window_rank(fn, self._ptr(part_start),
                                     self._ptr(peer_start), n, out.ptr),
               "bg_window_rank")

    def window_frame(self, units, start, end, order_col, descending, bounds,
                     n, lo, hi):
        """start/end: (kind, offset); a float offset travels as its f64
        bits.  bounds: (part_start, part_end, peer_start, peer_end)."""
        def off(o):
            return struct_unpack_bits(o) if isinstance(o, float) else int(o)
        _check(self.L.bg_window_frame(
            units, start[0], off(start[1]), end[0], off(end[1]),
            ctypes.byref(order_col) if order_col is not None else None,
            1 if descending else 0, *[self._ptr(b) for b in bounds], n,
            lo.ptr, hi.ptr), "bg_window_frame")

    def window_agg(self, fn, val, part_start, lo, hi, n, out, valid_out=None):
        """val None = count(*); lo None = the frame starts at part_start."""
        _check(self.L.bg_window_agg(
            fn, ctypes.byref(val) if val is not None else None,
            self._ptr(part_start), self._ptr(lo), hi.ptr, n, out.ptr,
            self._ptr(valid_out)), "bg_window_agg")

    def merge_join(self, build_sorted: DeviceBuffer, nb: int,
                   probe_sorted: DeviceBuffer, np_: int):
        """Inner merge join of key-sorted i64 buffers -> (probe_pos,
        build_pos DeviceBuffers into the sorted orders, n_matches)."""
        matches = ctypes.c_int64()
        _check(self.L.bg_merge_join(build_sorted.ptr, nb, probe_sorted.ptr,
                                    np_, ctypes.byref(matches), None, None),
               "bg_merge_join(count)")
        m = matches.value
        pbuf = self.alloc(max(4 * m, 4))
        bbuf = self.alloc(max(4 * m, 4))
        _check(self.L.bg_merge_join(build_sorted.ptr, nb, probe_sorted.ptr,
                                    np_, ctypes.byref(matches), pbuf.ptr,
                                    bbuf.ptr), "bg_merge_join(fill)")
        return pbuf, bbuf, m

    # ---- codecs ----
    def _decompress(self, fn, job_cls, items):
        """items: list of (src, src_len, dst, dst_cap), src/dst DeviceBuffers
        or raw addresses. -> decompressed lengths (-1 = malformed)."""
        arr = (job_cls * len(items))()
        for i, (src, slen, dst, dcap) in enumerate(items):
            arr[i] = job_cls(getattr(src, "ptr", src), getattr(dst, "ptr", dst),
                             slen, dcap)
        lens = np.zeros(len(items), dtype=np.int64)
        _check(getattr(self.L, fn)(arr, len(items), lens.ctypes.data), fn)
        return lens.tolist()

    def snappy_decompress(self, pages):
        """pages: list of (src DeviceBuffer, src_len, dst DeviceBuffer,
        dst_cap). -> list of decompressed lengths (-1 = malformed)."""
        return self._decompress("bg_snappy_decompress", BgSnappyPage, pages)

    def lz4_decompress(self, frames):
        """frames: list of (src DeviceBuffer, src_len, dst DeviceBuffer,
        dst_cap) pointing at LZ4 frame magic. -> decompressed lengths."""
        return self._decompress("bg_lz4_decompress", BgLz4Frame, frames)

    def lz4_compress(self, src: DeviceBuffer, length: int):
        """Device LZ4 -> (block sizes i64[nblocks], negative = stored raw;
        slots DeviceBuffer)."""
        nblocks = (length + BG_LZ4_BLOCK - 1) // BG_LZ4_BLOCK if length else 0
        slots = self.alloc(max(nblocks * BG_LZ4_SLOT_STRIDE, 8))
        sizes = np.zeros(max(nblocks, 1), dtype=np.int64)
        nb = ctypes.c_int64()
        _check(self.L.bg_lz4_compress(src.ptr, length, slots.ptr,
                                      sizes.ctypes.data, ctypes.byref(nb)),
               "bg_lz4_compress")
        return sizes[:nblocks], slots


class GpuHashJoin:
    """INNER equi-join (Int64 keys) — bg_hashjoin_* wrapper.
    Build once, probe many (HashJoinExec build/probe semantics)."""

    def __init__(self, ctx: GpuStageContext, build_keys: BgColumn, n_build: int):
        self.ctx = ctx
        self._handle = ctypes.c_void_p()
        _check(ctx.L.bg_hashjoin_build(ctypes.byref(build_keys), n_build,
                                       ctypes.byref(self._handle)),
               "bg_hashjoin_build")

    def probe(self, probe_keys: BgColumn, n_probe: int):
        """-> (probe_idx DeviceBuffer, build_idx DeviceBuffer, n_matches)."""
        ctx = self.ctx
        matches = ctypes.c_int64()
        _check(ctx.L.bg_hashjoin_probe_count(self._handle,
                                             ctypes.byref(probe_keys),
                                             n_probe, ctypes.byref(matches)),
               "bg_hashjoin_probe_count")
        m = matches.value
        pbuf = ctx.alloc(max(4 * m, 4))
        bbuf = ctx.alloc(max(4 * m, 4))
        _check(ctx.L.bg_hashjoin_probe_fill(self._handle,
                                            ctypes.byref(probe_keys), n_probe,
                                            pbuf.ptr, bbuf.ptr),
               "bg_hashjoin_probe_fill")
        return pbuf, bbuf, m

    def free(self):
        if self._handle and self._handle.value:
            self.ctx.L.bg_hashjoin_free(self._handle)
            self._handle = ctypes.c_void_p()
