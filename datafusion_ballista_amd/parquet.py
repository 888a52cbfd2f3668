"""GPU Parquet column-chunk decode (first slice).

Replaces the CPU side of `DataSourceExec(Parquet)` feeding the hot path for
the common TPC-H column shapes: Snappy- or uncompressed column chunks,
PLAIN-encoded values (INT32/INT64/DOUBLE/FIXED_LEN_BYTE_ARRAY(16) decimal),
required-or-no-null optional columns.  Pages are decompressed and unpacked
ON DEVICE (bg_snappy_decompress + bg_page_extract); the host only parses
footer/page metadata (thrift) and drives the copies — the same split as the
shuffle path (metadata host-side, bytes device-side).

Coverage: V1 + V2 data pages, PLAIN + dictionary encodings, the three
DELTA encodings + BYTE_STREAM_SPLIT, BYTE_ARRAY strings, FLBA decimals,
nullable columns (definition levels -> Arrow validity bitmap + slot->value
scatter on device), and LIST columns of primitives,
strings and decimals (repetition + definition levels walked on device by
bg_list_levels_batch; read_list_column_all).
Fails loudly: deeper nesting (max_rep > 1), LIST + V2 pages, codecs
beyond SNAPPY/UNCOMPRESSED/ZSTD/GZIP (the latter two via an explicit
host-codec bridge; LIST itself is SNAPPY/UNCOMPRESSED only).

The thrift compact-protocol PageHeader parser below restates the published
parquet-format spec (PageHeader/DataPageHeader structs); parity is pinned
against pyarrow's own reader in tests.
"""

import ctypes

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from . import gpu

# thrift compact type ids
_CT_BOOL_T = 1
_CT_BOOL_F = 2
_CT_BYTE = 3
_CT_I16 = 4
_CT_I32 = 5
_CT_I64 = 6
_CT_DOUBLE = 7
_CT_BINARY = 8
_CT_LIST = 9
_CT_SET = 10
_CT_MAP = 11
_CT_STRUCT = 12


class _Reader:
    def __init__(self, buf, pos=0):
        self.b = buf
        self.i = pos

    def varint(self):
        x = 0
        s = 0
        while True:
            c = self.b[self.i]
            self.i += 1
            x |= (c & 0x7F) << s
            if not (c & 0x80):
                return x
            s += 7

    def zigzag(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def skip(self, t):
        if t in (_CT_BOOL_T, _CT_BOOL_F):
            return
        if t == _CT_BYTE:
            self.i += 1
        elif t in (_CT_I16, _CT_I32, _CT_I64):
            self.varint()
        elif t == _CT_DOUBLE:
            self.i += 8
        elif t == _CT_BINARY:
            n = self.varint()
            self.i += n
        elif t in (_CT_LIST, _CT_SET):
            h = self.b[self.i]
            self.i += 1
            n = h >> 4
            et = h & 0x0F
            if n == 15:
                n = self.varint()
            for _ in range(n):
                self.skip(et)
        elif t == _CT_MAP:
            n = self.varint()
            if n:
                kv = self.b[self.i]
                self.i += 1
                for _ in range(n):
                    self.skip(kv >> 4)
                    self.skip(kv & 0x0F)
        elif t == _CT_STRUCT:
            self.struct_generic()
        else:
            raise ValueError(f"thrift type {t}")

    def struct_generic(self, want=None):
        """Parse a struct; collect fields listed in `want` {fid: 'i32'|...};
        skip everything else.  Returns {fid: value, ...} plus nested structs
        requested as ('struct', subwant)."""
        out = {}
        fid = 0
        while True:
            h = self.b[self.i]
            self.i += 1
            if h == 0:
                return out
            delta = h >> 4
            t = h & 0x0F
            fid = fid + delta if delta else self.zigzag()
            if want and fid in want:
                spec = want[fid]
                if spec == "i32" or spec == "i64":
                    out[fid] = self.zigzag()
                elif spec == "bool":
                    out[fid] = (t == _CT_BOOL_T)
                elif isinstance(spec, tuple) and spec[0] == "struct":
                    out[fid] = self.struct_generic(spec[1])
                else:
                    self.skip(t)
            else:
                self.skip(t)


# PageType: 0 DATA_PAGE, 2 DICTIONARY_PAGE, 3 DATA_PAGE_V2
# Encoding: 0 PLAIN, 3 RLE, 4 BIT_PACKED, 8 RLE_DICTIONARY
def parse_page_header(buf, pos):
    r = _Reader(buf, pos)
    h = r.struct_generic({
        1: "i32",   # type
        2: "i32",   # uncompressed_page_size
        3: "i32",   # compressed_page_size
        5: ("struct", {1: "i32", 2: "i32", 3: "i32", 4: "i32"}),  # v1 header
        7: ("struct", {1: "i32", 2: "i32"}),  # dictionary page header
        8: ("struct", {1: "i32", 2: "i32", 3: "i32", 4: "i32", 5: "i32",
                       6: "i32", 7: "bool"}),  # DataPageHeaderV2
    })
    return h, r.i


_PHYS_NP = {
    "INT32": (np.int32, 4),
    "INT64": (np.int64, 8),
    "DOUBLE": (np.float64, 8),
    "FLOAT": (np.float32, 4),
}


def _snappy_pages(ctx, chunk, scratch, jobs):
    """One batched bg_snappy_decompress of `jobs` = (file_off, csz,
    scratch_off, usz) pages from the resident file buffer into their
    scratch slots; raises on a page that does not decode to usz bytes."""
    arr = (gpu.BgSnappyPage * len(jobs))()
    for i, (poff, csz, soff, usz) in enumerate(jobs):
        arr[i] = gpu.BgSnappyPage(chunk.at(poff), scratch.at(soff), csz, usz)
    lens = np.zeros(len(jobs), dtype=np.int64)
    gpu._check(ctx.L.bg_snappy_decompress(arr, len(jobs), lens.ctypes.data),
               "bg_snappy_decompress")
    for i, (_, _, _, usz) in enumerate(jobs):
        if lens[i] != usz:
            raise RuntimeError(f"snappy page {i} failed ({lens[i]})")


def _nullable_ptrs(vidx, npres, slot, page):
    """The (d_vidx, d_n_present) pair of a mode-2 job: the slot -> value-
    index map from `slot` on and the page's present-count cell.  A required
    column has neither (vidx is None): (None, None)."""
    if vidx is None:
        return None, None
    return vidx.at(4 * slot), npres.at(8 * page)


class GpuParquetColumnReader:
    """Decode one (row_group, column) chunk to a contiguous device buffer."""

    def __init__(self, ctx: "gpu.GpuStageContext", path: str):
        self.ctx = ctx
        self.path = path
        self.pf = pq.ParquetFile(path)
        self.raw = open(path, "rb").read()
        # whole file resident once; every page is addressed by file offset
        self._file_buf = ctx.upload(np.frombuffer(self.raw, dtype=np.uint8))

    def read_column(self, rg: int, col: int):
        return self.read_column_all(col, rgs=[rg])

    def read_column_all(self, col: int, rgs=None):
        """Decode a column across row groups in ONE batched pass (one
        snappy launch over every page of every chunk — chunks alone hold
        too few pages to fill 256 CUs).
        -> (DeviceBuffer of raw values, num_values, physical_type,
        validity DeviceBuffer or None (required/non-null column))."""
        ctx = self.ctx
        if rgs is None:
            rgs = range(self.pf.metadata.num_row_groups)
        rgs = list(rgs)
        meta = self.pf.metadata.row_group(rgs[0]).column(col)
        codec = meta.compression  # 'SNAPPY' | 'UNCOMPRESSED' | ...
        if codec not in ("SNAPPY", "UNCOMPRESSED", "ZSTD", "GZIP"):
            raise RuntimeError(f"codec {codec} not GPU-decodable yet")
        # ZSTD/GZIP: no device decoder yet — pages are
        # HOST-decompressed with arrow's own codec and uploaded once; all
        # page-content decode (encodings, levels, strings) stays on device.
        # Explicitly a host-codec bridge, never a silent whole-path
        # fallback.
        phys = meta.physical_type
        if phys in _PHYS_NP:
            src_esz = dst_esz = _PHYS_NP[phys][1]
            flba = False
        elif phys == "BYTE_ARRAY":
            src_esz = dst_esz = 0  # variable width: lens+addr staging
            flba = False
        elif phys == "FIXED_LEN_BYTE_ARRAY":
            # parquet stores decimals at the minimal width for the
            # precision (FLBA(7) for Decimal(15,2)), big-endian; the device
            # sign-extends to 16-byte LE decimal128
            src_esz = self.pf.schema.column(col).length
            dst_esz = 16
            flba = True
        else:
            raise RuntimeError(f"physical type {phys} not GPU-decodable yet")

        chunk = self._file_buf  # page offsets below are absolute file offsets
        if self.pf.schema.column(col).max_repetition_level > 0:
            # nested column through the FLAT path would misread the page
            # body ([u32 rlen][rep] sits ahead of the def section): route
            # LIST columns to read_list_column_all, reject deeper nesting
            raise RuntimeError(
                "nested column: use read_list_column_all (max_rep == 1)")
        max_def0 = self.pf.schema.column(col).max_definition_level
        headers = []  # (rg, ptype, file_off, csz, usz, nvals, enc, ndict,
        #               soff, v2) with v2 = None (V1) or
        #               (def_len, values_csz, values_usz, is_compressed);
        #               for V2, usz is the SLOT length (the V1-shaped
        #               [u32 dlen][levels][values] image synthesized below)
        scratch_total = 0
        total_values = 0
        for rg in rgs:
            m = self.pf.metadata.row_group(rg).column(col)
            start = m.data_page_offset
            if m.has_dictionary_page and \
                    m.dictionary_page_offset is not None and \
                    m.dictionary_page_offset < start:
                start = m.dictionary_page_offset
            end = start + m.total_compressed_size
            pos = start
            total_values += m.num_values
            while pos < end:
                h, data_pos = parse_page_header(self.raw, pos)
                ptype = h.get(1, 0)
                usz = h[2]
                csz = h[3]
                nvals = enc = ndict = 0
                v2 = None
                if ptype == 2:
                    ndict = h.get(7, {}).get(1, 0)
                elif ptype == 0:
                    dph = h.get(5, {})
                    nvals = dph.get(1, 0)
                    enc = dph.get(2, 0)
                    if enc not in (0, 2, 5, 6, 7, 8, 9):
                        raise RuntimeError(
                            f"encoding {enc}: not GPU-decodable yet")
                elif ptype == 3:
                    # DataPageV2 (PageHeader field 8): levels sit ahead of
                    # the (optionally compressed) values, uncompressed
                    dph = h.get(8, {})
                    nvals = dph.get(1, 0)
                    enc = dph.get(4, 0)
                    def_len = dph.get(5, 0)
                    rep_len = dph.get(6, 0)
                    is_comp = dph.get(7, 1)
                    if rep_len:
                        raise RuntimeError(
                            "DATA_PAGE_V2 repetition levels (nested): "
                            "not GPU-decodable yet")
                    if enc not in (0, 2, 5, 6, 7, 8, 9):
                        raise RuntimeError(
                            f"encoding {enc}: not GPU-decodable yet")
                    values_csz = csz - def_len
                    values_usz = usz - def_len
                    # synthesize the V1 page shape so every downstream
                    # kernel (def walk, extract, dict) is unchanged
                    slot_len = (4 + def_len + values_usz) if max_def0 > 0 \
                        else values_usz
                    v2 = (def_len, values_csz, values_usz, is_comp)
                    usz = slot_len
                headers.append((rg, ptype, data_pos, csz, usz, nvals, enc,
                                ndict, scratch_total, v2))
                scratch_total += (usz + 255) & ~255
                pos = data_pos + csz

        scratch = ctx.alloc(max(scratch_total, 256))

        ba = phys == "BYTE_ARRAY"
        if ba:
            ba_lens = ctx.alloc(max(8 * total_values, 8))
            ba_srcaddr = ctx.alloc(max(8 * total_values, 8))
            out = None
        else:
            out = ctx.alloc(max(total_values * dst_esz, dst_esz))
        extracts = []        # PLAIN: (scratch_off, usz, dst_off, nvals, pidx)
        deltas = []          # DELTA_BINARY_PACKED pages (same tuple)
        delta_ba = []        # DELTA(_LENGTH)_BYTE_ARRAY pages (+enc)
        bss = []             # BYTE_STREAM_SPLIT pages
        dict_runs = {}       # rg -> {"dict": (soff, usz, ndict), "pages": []}
        got_values = 0
        snappy_jobs = []
        data_pages = []      # (scratch_off, usz, dst_off, nvals) in order
        v2_fixups = []  # (kind, scratch_off, file_off, nbytes); kind is an
        # explicit tag ("def" = [u32 dlen] prefix + level bytes, "raw" =
        # uncompressed values copy) — sign-encoding the length misclassified
        # zero-length raw copies (all-null uncompressed V2 pages) as prefix
        # entries and desynchronized the prefix index
        for (rg, ptype, poff, csz, usz, nvals, enc, ndict, soff,
             v2) in headers:
            if v2 is not None:
                def_len, values_csz, values_usz, is_comp = v2
                voff = (4 + def_len) if max_def0 > 0 else 0
                if max_def0 > 0:
                    v2_fixups.append(("def", soff, poff, def_len))
                if codec == "SNAPPY" and is_comp:
                    snappy_jobs.append((poff + def_len, values_csz,
                                        soff + voff, values_usz))
                else:
                    v2_fixups.append(("raw", soff + voff, poff + def_len,
                                      values_usz))
            elif codec == "SNAPPY":
                snappy_jobs.append((poff, csz, soff, usz))
            if ptype == 2:
                dict_runs.setdefault(rg, {"dict": None, "pages": []})
                dict_runs[rg]["dict"] = (soff, usz, ndict)
            elif ptype in (0, 3):
                pidx = len(data_pages)
                data_pages.append((soff, usz, got_values, nvals))
                if enc == 5:
                    if phys not in ("INT32", "INT64"):
                        raise RuntimeError(
                            "DELTA_BINARY_PACKED: INT32/INT64 only")
                    deltas.append((soff, usz, got_values, nvals, pidx))
                elif enc == 9:
                    if flba or phys == "BYTE_ARRAY":
                        raise RuntimeError(
                            "BYTE_STREAM_SPLIT: fixed-width plain types")
                    bss.append((soff, usz, got_values, nvals, pidx))
                elif enc in (6, 7):
                    if phys != "BYTE_ARRAY":
                        raise RuntimeError(
                            "DELTA(_LENGTH)_BYTE_ARRAY: BYTE_ARRAY only")
                    delta_ba.append((soff, usz, got_values, nvals, pidx,
                                     enc))
                elif enc == 0:
                    extracts.append((soff, usz, got_values, nvals, pidx))
                else:
                    if rg not in dict_runs or dict_runs[rg]["dict"] is None:
                        raise RuntimeError("dict-coded page without dict page")
                    dict_runs[rg]["pages"].append(
                        (soff, usz, got_values, nvals, pidx))
                got_values += nvals
        if got_values != total_values:
            raise RuntimeError(f"decoded {got_values} != {total_values} values")
        if v2_fixups:
            # synthesize the V1 image pieces: [u32 dlen] prefix + the
            # uncompressed level bytes (and raw values when the page body
            # is not compressed), copied device-to-device from the
            # resident file buffer via a tiny staged prefix table
            prefixes = np.array([d for (k, _, _, d) in v2_fixups
                                 if k == "def"], dtype=np.uint32)
            pbuf = ctx.upload(prefixes) if len(prefixes) else None
            pi = 0
            for (kind, soff, foff, dlen) in v2_fixups:
                if kind == "raw":  # uncompressed values copy (may be empty)
                    if dlen:
                        gpu._check(ctx.L.bg_memcpy_dtod(scratch.at(soff),
                                                        chunk.at(foff), dlen),
                                   "v2 values copy")
                    continue
                gpu._check(ctx.L.bg_memcpy_dtod(scratch.at(soff),
                                                pbuf.at(4 * pi), 4),
                           "v2 dlen prefix")
                pi += 1
                if dlen:
                    gpu._check(ctx.L.bg_memcpy_dtod(scratch.at(soff + 4),
                                                    chunk.at(foff), dlen),
                               "v2 def levels copy")

        if codec == "SNAPPY":
            _snappy_pages(ctx, chunk, scratch, snappy_jobs)
        elif codec in ("ZSTD", "GZIP"):
            if any(h[9] is not None for h in headers):
                raise RuntimeError(
                    f"{codec} + DataPageV2: not GPU-decodable yet")
            pa_codec = pa.Codec(codec.lower())
            host = np.zeros(scratch_total, dtype=np.uint8)
            for (rg, ptype, poff, csz, usz, nvals, enc, ndict, soff,
                 v2) in headers:
                dec = pa_codec.decompress(self.raw[poff:poff + csz],
                                          decompressed_size=usz)
                host[soff:soff + usz] = np.frombuffer(dec, dtype=np.uint8)
            gpu._check(ctx.L.bg_memcpy_h2d(scratch.ptr, host.ctypes.data,
                                           scratch_total), "bg_memcpy_h2d")
        else:
            # uncompressed: device-to-device copy page payloads into the
            # aligned scratch slots
            for (rg, ptype, poff, csz, usz, nvals, enc, ndict, soff,
                 v2) in headers:
                if v2 is not None:
                    continue  # synthesized above
                gpu._check(ctx.L.bg_memcpy_dtod(scratch.at(soff),
                                                chunk.at(poff), csz),
                           "bg_memcpy_dtod")

        # OPTIONAL column (max_def=1): decode definition levels on device
        # into the column validity bitmap + per-slot value indices, then
        # extract with the mode-2 (nullable) jobs; REQUIRED column: values
        # at offset 0  (ONE batched launch each)
        max_def = max_def0
        valid = vidx = npres = None
        mode = 0
        if max_def > 0:
            mode = 2
            nwords = (total_values + 31) // 32
            valid = ctx.upload(np.zeros(nwords, dtype=np.uint32))
            vidx = ctx.alloc(max(4 * total_values, 4))
            npres = ctx.alloc(max(8 * len(data_pages), 8))
            djobs = (gpu.BgDefLevelsJob * len(data_pages))()
            for i, (soff, usz, dst_off, nvals) in enumerate(data_pages):
                djobs[i] = gpu.BgDefLevelsJob(
                    scratch.at(soff), vidx.at(4 * dst_off), valid.ptr.value,
                    usz, nvals, dst_off, npres.at(8 * i))
            gpu._check(ctx.L.bg_def_levels_batch(djobs, len(data_pages)),
                       "bg_def_levels_batch")
        if extracts and ba:
            jobs = (gpu.BgBaPageJob * len(extracts))()
            for i, (soff, usz, dst_off, nvals, pidx) in enumerate(extracts):
                jobs[i] = gpu.BgBaPageJob(
                    scratch.at(soff), ba_lens.at(8 * dst_off),
                    ba_srcaddr.at(8 * dst_off), usz, nvals, mode, 0,
                    *_nullable_ptrs(vidx, npres, dst_off, pidx))
            gpu._check(ctx.L.bg_ba_extract_batch(jobs, len(extracts)),
                       "bg_ba_extract_batch")
        elif extracts:
            jobs = (gpu.BgPageExtractJob * len(extracts))()
            for i, (soff, usz, dst_off, nvals, pidx) in enumerate(extracts):
                jobs[i] = gpu.BgPageExtractJob(
                    scratch.at(soff), out.at(dst_off * dst_esz), usz, nvals,
                    src_esz, mode, 1 if flba else 0,
                    *_nullable_ptrs(vidx, npres, dst_off, pidx))
            gpu._check(ctx.L.bg_page_extract_batch(jobs, len(extracts)),
                       "bg_page_extract_batch")
        if delta_ba:
            jobs7 = (gpu.BgDeltaBaJob * len(delta_ba))()
            for i, (soff, usz, dst_off, nvals, pidx, enc) in \
                    enumerate(delta_ba):
                jobs7[i] = gpu.BgDeltaBaJob(
                    scratch.at(soff), ba_lens.at(8 * dst_off),
                    ba_srcaddr.at(8 * dst_off), None, None, usz, nvals, mode,
                    enc, *_nullable_ptrs(vidx, npres, dst_off, pidx))
            gpu._check(ctx.L.bg_delta_ba_batch(jobs7, len(delta_ba), 1),
                       "bg_delta_ba_batch(1)")
        if bss:
            jobs9 = (gpu.BgPageExtractJob * len(bss))()
            for i, (soff, usz, dst_off, nvals, pidx) in enumerate(bss):
                jobs9[i] = gpu.BgPageExtractJob(
                    scratch.at(soff), out.at(dst_off * dst_esz), usz, nvals,
                    src_esz, mode, 0,
                    *_nullable_ptrs(vidx, npres, dst_off, pidx))
            gpu._check(ctx.L.bg_bss_batch(jobs9, len(bss)), "bg_bss_batch")
        if deltas:
            djobs2 = (gpu.BgDeltaBpJob * len(deltas))()
            for i, (soff, usz, dst_off, nvals, pidx) in enumerate(deltas):
                djobs2[i] = gpu.BgDeltaBpJob(
                    scratch.at(soff), out.at(dst_off * dst_esz), usz, nvals,
                    dst_esz, mode, 0,
                    *_nullable_ptrs(vidx, npres, dst_off, pidx))
            gpu._check(ctx.L.bg_delta_bp_batch(djobs2, len(deltas)),
                       "bg_delta_bp_batch")

        all_dict_pages = [(rg, pg) for rg, d in dict_runs.items()
                          for pg in d["pages"]]
        if all_dict_pages:
            # PLAIN-decode every row group's dictionary (batched)
            dict_bufs = {}
            if ba:
                # string dictionaries: lens+addr walk, then one
                # materialize per rg into (i32 offsets, bytes)
                for rg, d in dict_runs.items():
                    if not d["pages"]:
                        continue
                    dsoff, dusz, ndict = d["dict"]
                    dl = ctx.alloc(max(8 * ndict, 8))
                    da = ctx.alloc(max(8 * ndict, 8))
                    j1 = (gpu.BgBaPageJob * 1)(gpu.BgBaPageJob(
                        scratch.at(dsoff), dl.ptr.value, da.ptr.value, dusz,
                        ndict, 0, 0, None, None))
                    gpu._check(ctx.L.bg_ba_extract_batch(j1, 1),
                               "bg_ba_extract(dict)")
                    doffs = ctx.alloc(max(4 * (ndict + 1), 8))
                    tot = ctypes.c_int64()
                    gpu._check(ctx.L.bg_ba_materialize(dl.ptr, da.ptr, ndict,
                                                       doffs.ptr, None, 0,
                                                       ctypes.byref(tot)),
                               "bg_ba_materialize(dict size)")
                    ddata = ctx.alloc(max(tot.value, 1))
                    gpu._check(ctx.L.bg_ba_materialize(
                        dl.ptr, da.ptr, ndict, doffs.ptr, ddata.ptr, tot.value,
                        ctypes.byref(tot)), "bg_ba_materialize(dict)")
                    dict_bufs[rg] = (doffs, ddata)
            else:
                djobs = []
                for rg, d in dict_runs.items():
                    if not d["pages"]:
                        continue
                    dsoff, dusz, ndict = d["dict"]
                    dbuf = ctx.alloc(max(ndict * dst_esz, dst_esz))
                    dict_bufs[rg] = dbuf
                    djobs.append(gpu.BgPageExtractJob(
                        scratch.at(dsoff), dbuf.ptr.value, dusz, ndict,
                        src_esz, 0, 1 if flba else 0))
                jarr = (gpu.BgPageExtractJob * len(djobs))(*djobs)
                gpu._check(ctx.L.bg_page_extract_batch(jarr, len(djobs)),
                           "bg_page_extract(dicts)")
            # ONE batched index expansion over every dict-coded page
            nidx_total = sum(pg[3] for (_, pg) in all_dict_pages)
            idx = ctx.alloc(max(4 * nidx_total, 4))
            dense = ctx.alloc(max(4 * nidx_total, 4)) if mode else None
            jobs = (gpu.BgDictIndicesJob * len(all_dict_pages))()
            run = 0
            gathers = []  # (rg, idx_off, dst_off, nvals) merged per rg below
            for i, (rg, (soff, usz, dst_off, nvals, pidx)) in \
                    enumerate(all_dict_pages):
                jobs[i] = gpu.BgDictIndicesJob(
                    scratch.at(soff), idx.at(4 * run), usz, nvals, mode, 0,
                    *_nullable_ptrs(vidx, npres, dst_off, pidx),
                    dense.at(4 * run) if mode else None)
                gathers.append((rg, run, dst_off, nvals))
                run += nvals
            gpu._check(ctx.L.bg_dict_indices_batch(jobs, len(all_dict_pages)),
                       "bg_dict_indices_batch")
            # merge adjacent pages of one rg into single gathers
            merged = []
            for rg, ioff, dst_off, nvals in gathers:
                if merged and merged[-1][0] == rg and \
                        merged[-1][2] + merged[-1][3] == dst_off:
                    merged[-1][3] += nvals
                else:
                    merged.append([rg, ioff, dst_off, nvals])
            for rg, ioff, dst_off, nvals in merged:
                if ba:
                    doffs, ddata = dict_bufs[rg]
                    gpu._check(ctx.L.bg_ba_from_dict(
                        idx.at(4 * ioff), doffs.ptr, ddata.ptr,
                        vidx.at(4 * dst_off) if mode else None, nvals,
                        ba_lens.at(8 * dst_off), ba_srcaddr.at(8 * dst_off)),
                               "bg_ba_from_dict")
                else:
                    gpu._check(ctx.L.bg_gather(dict_bufs[rg].ptr, dst_esz,
                                               idx.at(4 * ioff), nvals,
                                               out.at(dst_off * dst_esz)),
                               "bg_gather(dict)")
        if ba:
            offs32 = ctx.alloc(max(4 * (total_values + 1), 8))
            tot = ctypes.c_int64()
            gpu._check(ctx.L.bg_ba_materialize(ba_lens.ptr, ba_srcaddr.ptr,
                                               total_values, offs32.ptr, None,
                                               0, ctypes.byref(tot)),
                       "bg_ba_materialize(size)")
            cap = tot.value
            data = ctx.alloc(max(cap, 1))
            gpu._check(ctx.L.bg_ba_materialize(
                ba_lens.ptr, ba_srcaddr.ptr, total_values, offs32.ptr,
                data.ptr, cap, ctypes.byref(tot)), "bg_ba_materialize")
            enc7 = [d for d in delta_ba if d[5] == 7]
            if enc7:
                jobs8 = (gpu.BgDeltaBaJob * len(enc7))()
                for i, (soff, usz, dst_off, nvals, pidx, enc) in \
                        enumerate(enc7):
                    jobs8[i] = gpu.BgDeltaBaJob(
                        scratch.at(soff), ba_lens.at(8 * dst_off),
                        ba_srcaddr.at(8 * dst_off), offs32.at(4 * dst_off),
                        data.ptr.value, usz, nvals, mode, enc,
                        *_nullable_ptrs(vidx, npres, dst_off, pidx))
                gpu._check(ctx.L.bg_delta_ba_batch(jobs8, len(enc7), 2),
                           "bg_delta_ba_batch(2)")
            ctx.synchronize()
            return ((offs32, data, tot.value), total_values, "BYTE_ARRAY",
                    valid)
        ctx.synchronize()
        return (out, total_values, phys if not flba else "DECIMAL128",
                valid)

    def read_list_column_all(self, col: int, rgs=None):
        """Decode a LIST<primitive> column (max_rep == 1) across row
        groups: repetition + definition levels walk on device
        (bg_list_levels_batch: parquet-format.md "Nested Encoding"; the
        reference reads these via arrow-rs' list reader), element values
        via the UNCHANGED mode-2 extract/dict kernels re-pointed past the
        [u32 rlen][rep] section.  List offsets are the prefix sum of the
        per-row entry counts — computed host-side from one row_sizes
        download (i32/row; an explicit bridge, like the ZSTD host codec).

        -> dict(offsets=np.int32[nrows+1], n_rows, n_entries,
                values=DeviceBuffer (entry space), phys,
                elem_valid=DeviceBuffer u32 words,
                list_valid=DeviceBuffer u32 words or None (required list),
                row_sizes=DeviceBuffer i32[nrows])"""
        ctx = self.ctx
        if rgs is None:
            rgs = range(self.pf.metadata.num_row_groups)
        rgs = list(rgs)
        sc = self.pf.schema.column(col)
        max_rep = sc.max_repetition_level
        max_def = sc.max_definition_level
        if max_rep != 1:
            raise RuntimeError(
                f"max_rep={max_rep}: only 1-level LIST is GPU-decodable")
        # level thresholds from the schema's nullability shape:
        #   optional list adds 1, the repeated level adds 1, optional
        #   element adds 1 (parquet-format.md Nested Encoding)
        arrow_field = self.pf.schema_arrow.field(
            sc.path.split(".")[0])
        list_nullable = arrow_field.nullable
        elem_nullable = max_def == (2 if not list_nullable else 3)
        def_entry = max_def - (1 if elem_nullable else 0)
        def_valid = 1 if list_nullable else 0
        meta = self.pf.metadata.row_group(rgs[0]).column(col)
        codec = meta.compression
        if codec not in ("SNAPPY", "UNCOMPRESSED"):
            raise RuntimeError(f"LIST + codec {codec}: not GPU-decodable")
        phys = meta.physical_type
        ba = phys == "BYTE_ARRAY"
        flba = phys == "FIXED_LEN_BYTE_ARRAY"
        if ba:
            src_esz, esz = 0, 0
        elif flba:
            src_esz, esz = self.pf.schema.column(col).length, 16
        elif phys in _PHYS_NP:
            src_esz = esz = _PHYS_NP[phys][1]
        else:
            raise RuntimeError(f"LIST of {phys}: not GPU-decodable yet")

        chunk = self._file_buf
        headers = []  # (soff, usz, nslots, enc, ndict_or_0, rg)
        scratch_total = 0
        total_slots = 0
        for rg in rgs:
            m = self.pf.metadata.row_group(rg).column(col)
            start = m.data_page_offset
            if m.has_dictionary_page and \
                    m.dictionary_page_offset is not None and \
                    m.dictionary_page_offset < start:
                start = m.dictionary_page_offset
            end = start + m.total_compressed_size
            pos = start
            total_slots += m.num_values
            while pos < end:
                h, data_pos = parse_page_header(self.raw, pos)
                ptype = h.get(1, 0)
                usz, csz = h[2], h[3]
                if ptype == 3:
                    raise RuntimeError(
                        "LIST + DataPageV2: not GPU-decodable yet")
                if ptype == 2:
                    ndict = h.get(7, {}).get(1, 0)
                    headers.append((data_pos, csz, usz, 0, 0, ndict, rg))
                elif ptype == 0:
                    dph = h.get(5, {})
                    nvals, enc = dph.get(1, 0), dph.get(2, 0)
                    if enc not in (0, 2, 8):
                        raise RuntimeError(
                            f"LIST + encoding {enc}: not GPU-decodable")
                    headers.append((data_pos, csz, usz, nvals, enc, 0, rg))
                pos = data_pos + csz
        scratch_offs = []
        for (_, _, usz, *_rest) in headers:
            scratch_offs.append(scratch_total)
            scratch_total += (usz + 255) & ~255
        scratch = ctx.alloc(max(scratch_total, 256))
        snappy_jobs = []
        for (poff, csz, usz, *_rest), soff in zip(headers, scratch_offs):
            if codec == "SNAPPY":
                snappy_jobs.append((poff, csz, soff, usz))
            else:
                gpu._check(ctx.L.bg_memcpy_dtod(scratch.at(soff),
                                                chunk.at(poff), csz),
                           "bg_memcpy_dtod")
        if snappy_jobs:
            _snappy_pages(ctx, chunk, scratch, snappy_jobs)

        data_idx = [i for i, h in enumerate(headers) if h[3] > 0]
        npages = len(data_idx)
        # pass 1: per-page {rows, entries, present, rlen}
        counts = ctx.alloc(max(32 * npages, 32))
        jobs = (gpu.BgListLevelsJob * npages)()
        for j, i in enumerate(data_idx):
            (_, _, usz, nslots, enc, _, rg) = headers[i]
            jobs[j] = gpu.BgListLevelsJob(
                scratch.at(scratch_offs[i]), usz, nslots, max_def, def_entry,
                def_valid, 0, 0, 0, counts.at(32 * j), None, None, None, None)
        gpu._check(ctx.L.bg_list_levels_batch(jobs, npages, 1),
                   "bg_list_levels_batch(1)")
        ctx.synchronize()
        cts = counts.download(np.int64, 4 * npages).reshape(npages, 4)
        rows_pp, ents_pp, pres_pp, rlen_pp = (cts[:, 0], cts[:, 1],
                                              cts[:, 2], cts[:, 3])
        n_rows = int(rows_pp.sum())
        n_entries = int(ents_pp.sum())
        row_bases = np.concatenate(([0], np.cumsum(rows_pp)))
        ent_bases = np.concatenate(([0], np.cumsum(ents_pp)))

        row_sizes = ctx.upload(np.zeros(max(n_rows, 1), dtype=np.int32))
        lv_words = (n_rows + 31) // 32
        ev_words = (n_entries + 31) // 32
        list_valid = ctx.upload(np.zeros(max(lv_words, 1),
                                         dtype=np.uint32)) \
            if list_nullable else None
        elem_valid = ctx.upload(np.zeros(max(ev_words, 1), dtype=np.uint32))
        vidx = ctx.alloc(max(4 * n_entries, 4))
        all_valid = ctx.upload(np.full(max(lv_words, ev_words, 1),
                                       0xffffffff, dtype=np.uint32))
        # pass 2
        for j, i in enumerate(data_idx):
            (_, _, usz, nslots, enc, _, rg) = headers[i]
            jobs[j] = gpu.BgListLevelsJob(
                scratch.at(scratch_offs[i]), usz, nslots, max_def, def_entry,
                def_valid, 0, int(row_bases[j]), int(ent_bases[j]), None,
                row_sizes.ptr.value,
                (list_valid if list_valid is not None else all_valid).ptr.value,
                elem_valid.ptr.value, vidx.at(4 * int(ent_bases[j])))
        gpu._check(ctx.L.bg_list_levels_batch(jobs, npages, 2),
                   "bg_list_levels_batch(2)")

        # element values (entry space) — mode-2 extract/dict re-pointed
        # past [u32 rlen][rep]; BYTE_ARRAY elements via the same
        # lens/addr staging + materialize the flat path uses
        if ba:
            out = None
            ba_lens = ctx.alloc(max(8 * n_entries, 8))
            ba_srcaddr = ctx.alloc(max(8 * n_entries, 8))
        else:
            out = ctx.alloc(max(n_entries * esz, esz))
        npres = ctx.upload(pres_pp.astype(np.int64)) if npages else None
        plain, dict_pages = [], []
        for j, i in enumerate(data_idx):
            (_, _, usz, nslots, enc, _, rg) = headers[i]
            shift = 4 + int(rlen_pp[j])
            tup = (scratch_offs[i] + shift, usz - shift,
                   int(ent_bases[j]), int(ents_pp[j]), j, rg)
            (plain if enc == 0 else dict_pages).append(tup)
        if plain and ba:
            bjobs = (gpu.BgBaPageJob * len(plain))()
            for i, (soff, plen, ebase, ents, j, rg) in enumerate(plain):
                bjobs[i] = gpu.BgBaPageJob(
                    scratch.at(soff), ba_lens.at(8 * ebase),
                    ba_srcaddr.at(8 * ebase), plen, ents, 2, 0,
                    *_nullable_ptrs(vidx, npres, ebase, j))
            gpu._check(ctx.L.bg_ba_extract_batch(bjobs, len(plain)),
                       "bg_ba_extract_batch(list)")
        elif plain:
            ejobs = (gpu.BgPageExtractJob * len(plain))()
            for i, (soff, plen, ebase, ents, j, rg) in enumerate(plain):
                ejobs[i] = gpu.BgPageExtractJob(
                    scratch.at(soff), out.at(ebase * esz), plen, ents, src_esz,
                    2, 1 if flba else 0,
                    *_nullable_ptrs(vidx, npres, ebase, j))
            gpu._check(ctx.L.bg_page_extract_batch(ejobs, len(plain)),
                       "bg_page_extract_batch(list)")
        if dict_pages:
            dict_bufs = {}
            for i, h in enumerate(headers):
                if h[5] > 0:  # dictionary page of rg h[6]
                    if ba:
                        dsoff, dusz, ndict = scratch_offs[i], h[2], h[5]
                        dl = ctx.alloc(max(8 * ndict, 8))
                        da = ctx.alloc(max(8 * ndict, 8))
                        j1 = (gpu.BgBaPageJob * 1)(gpu.BgBaPageJob(
                            scratch.at(dsoff), dl.ptr.value, da.ptr.value,
                            dusz, ndict, 0, 0, None, None))
                        gpu._check(ctx.L.bg_ba_extract_batch(j1, 1),
                                   "bg_ba_extract(ldict)")
                        doffs = ctx.alloc(max(4 * (ndict + 1), 8))
                        tot = ctypes.c_int64()
                        gpu._check(ctx.L.bg_ba_materialize(
                            dl.ptr, da.ptr, ndict, doffs.ptr, None, 0,
                            ctypes.byref(tot)), "bg_ba_materialize(lsize)")
                        ddata = ctx.alloc(max(tot.value, 1))
                        gpu._check(ctx.L.bg_ba_materialize(
                            dl.ptr, da.ptr, ndict, doffs.ptr, ddata.ptr,
                            tot.value, ctypes.byref(tot)),
                                   "bg_ba_materialize(ldict)")
                        dict_bufs[h[6]] = (doffs, ddata)
                    else:
                        dbuf = ctx.alloc(max(h[5] * esz, esz))
                        j1 = (gpu.BgPageExtractJob * 1)(gpu.BgPageExtractJob(
                            scratch.at(scratch_offs[i]), dbuf.ptr.value, h[2],
                            h[5], src_esz, 0, 1 if flba else 0))
                        gpu._check(ctx.L.bg_page_extract_batch(j1, 1),
                                   "bg_page_extract(ldict)")
                        dict_bufs[h[6]] = dbuf
            nidx = sum(p[3] for p in dict_pages)
            idx = ctx.alloc(max(4 * nidx, 4))
            dense = ctx.alloc(max(4 * nidx, 4))
            djobs = (gpu.BgDictIndicesJob * len(dict_pages))()
            run = 0
            gathers = []
            for i, (soff, plen, ebase, ents, j, rg) in \
                    enumerate(dict_pages):
                djobs[i] = gpu.BgDictIndicesJob(
                    scratch.at(soff), idx.at(4 * run), plen, ents, 2, 0,
                    *_nullable_ptrs(vidx, npres, ebase, j), dense.at(4 * run))
                gathers.append((rg, run, ebase, ents))
                run += ents
            gpu._check(ctx.L.bg_dict_indices_batch(djobs, len(dict_pages)),
                       "bg_dict_indices_batch(list)")
            for rg, ioff, ebase, ents in gathers:
                if ba:
                    doffs, ddata = dict_bufs[rg]
                    gpu._check(ctx.L.bg_ba_from_dict(
                        idx.at(4 * ioff), doffs.ptr, ddata.ptr,
                        vidx.at(4 * ebase), ents, ba_lens.at(8 * ebase),
                        ba_srcaddr.at(8 * ebase)), "bg_ba_from_dict(list)")
                else:
                    gpu._check(ctx.L.bg_gather(dict_bufs[rg].ptr, esz,
                                               idx.at(4 * ioff), ents,
                                               out.at(ebase * esz)),
                               "bg_gather(ldict)")
        if ba:
            offs32 = ctx.alloc(max(4 * (n_entries + 1), 8))
            tot = ctypes.c_int64()
            gpu._check(ctx.L.bg_ba_materialize(ba_lens.ptr, ba_srcaddr.ptr,
                                               n_entries, offs32.ptr, None, 0,
                                               ctypes.byref(tot)),
                       "bg_ba_materialize(lsz)")
            data = ctx.alloc(max(tot.value, 1))
            gpu._check(ctx.L.bg_ba_materialize(ba_lens.ptr, ba_srcaddr.ptr,
                                               n_entries, offs32.ptr, data.ptr,
                                               tot.value, ctypes.byref(tot)),
                       "bg_ba_materialize(list)")
            out = (offs32, data, tot.value)
        ctx.synchronize()
        sizes = row_sizes.download(np.int32, max(n_rows, 1))[:n_rows]
        offsets = np.zeros(n_rows + 1, dtype=np.int32)
        np.cumsum(sizes, out=offsets[1:])
        assert offsets[-1] == n_entries, (offsets[-1], n_entries)
        return {"offsets": offsets, "n_rows": n_rows,
                "n_entries": n_entries, "values": out, "phys": phys,
                "elem_valid": elem_valid, "list_valid": list_valid,
                "row_sizes": row_sizes}
