"""Page-level conformance of the Parquet decode kernels.

Hand-built pages (tests/parquet_pages.py, written from the parquet-format
spec and cross-checked against pyarrow in test_parquet_pages_host.py) go
straight into the bg_*_batch entry points; every comparison is exact.
Each test puts all its pages into one or two batch calls.

Every output buffer starts as 0xA5 bytes.  Where the kernels promise that
NULL slots stay untouched (page extract, DELTA_BINARY_PACKED,
BYTE_STREAM_SPLIT) the sentinel must survive; where they promise a value
(dictionary index 0, byte-array length 0) that value is asserted; and the
64 bytes after every output slice must still hold the sentinel.

Not covered because the reader does not support it: repetition depth > 1
(the host reader rejects max_rep > 1 before any kernel runs) and
DataPageV2 level layout (levels outside the page body).
"""
import ctypes

import numpy as np
import pytest

import parquet_pages as pp
from datafusion_ballista_amd import gpu

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = gpu.GpuStageContext(0)
    yield c
    c.close()


class _In:
    """All of a test's pages in one device buffer, each followed by at least
    pp.SLACK zero bytes."""

    def __init__(self):
        self.buf = bytearray()

    def add(self, page):
        off = len(self.buf)
        self.buf += page
        self.buf += bytes(pp.SLACK + (-len(page)) % 8)
        return off

    def upload(self, ctx):
        self.dev = ctx.upload(np.frombuffer(bytes(self.buf), dtype=np.uint8))
        return self

    def at(self, off):
        return self.dev.at(off)


class _Out:
    """All of a test's outputs in one sentinel-filled device buffer; each
    slice is 8-byte aligned and followed by at least GUARD sentinel bytes.
    zero=True slices (validity bitmaps, which the kernels OR into) start
    as zeros."""

    def __init__(self):
        self.size = 0
        self.slices = []

    def reserve(self, nbytes, zero=False):
        off = self.size
        self.size += (nbytes + 7) // 8 * 8 + GUARD
        self.slices.append((off, nbytes, zero))
        return off

    def upload(self, ctx):
        host = np.full(self.size, SENT, dtype=np.uint8)
        for off, nbytes, zero in self.slices:
            if zero:
                host[off:off + nbytes] = 0
        self.dev = ctx.upload(host)
        return self

    def at(self, off):
        return self.dev.at(off)

    def download(self, ctx):
        ctx.synchronize()
        self.host = self.dev.download(np.uint8, self.size)
        return self

    def get(self, off, nbytes, dtype=np.uint8):
        return self.host[off:off + nbytes].view(dtype)

    def check_guards(self):
        for off, nbytes, _ in self.slices:
            end = off + (nbytes + 7) // 8 * 8 + GUARD
            assert (self.host[off + nbytes:end] == SENT).all(), \
                f"write past the output slice at byte {off} (+{nbytes})"


def _ok(ctx, rc, what):
    assert rc == 0, f"{what}: rc={rc} {ctx.L.bg_last_error().decode()}"


def _arr(cls, jobs):
    return (cls * len(jobs))(*jobs)


class _Column:
    """Pages of one nullable column: runs bg_def_levels_batch over them and
    keeps what the mode-2 jobs need (vidx slice and n_present cell per
    page) plus the expected values of both."""

    def __init__(self, pin, out, pages_levels):
        # pages_levels: [(page offset in pin, page_len, levels)]
        self.pages = pages_levels
        self.total = sum(len(lv) for _, _, lv in pages_levels)
        self.nwords = (self.total + 31) // 32
        self.o_valid = out.reserve(4 * self.nwords, zero=True)
        self.o_vidx = out.reserve(4 * self.total)
        self.o_npres = out.reserve(8 * len(pages_levels))
        self.slot0 = []
        at = 0
        for _, _, lv in pages_levels:
            self.slot0.append(at)
            at += len(lv)
        self.pin, self.out = pin, out

    def run(self, ctx):
        jobs = [gpu.BgDefLevelsJob(
            self.pin.at(off), self.out.at(self.o_vidx + 4 * s0),
            self.out.at(self.o_valid), plen, len(lv), s0,
            self.out.at(self.o_npres + 8 * i))
            for i, ((off, plen, lv), s0) in
            enumerate(zip(self.pages, self.slot0))]
        _ok(ctx, ctx.L.bg_def_levels_batch(_arr(gpu.BgDefLevelsJob, jobs),
                                           len(jobs)), "bg_def_levels_batch")

    def ptrs(self, i):
        """(d_vidx, d_n_present) of page i."""
        return (self.out.at(self.o_vidx + 4 * self.slot0[i]),
                self.out.at(self.o_npres + 8 * i))

    def check(self):
        """whole bitmap, every vidx, every n_present."""
        out = self.out
        allv = [b for _, _, lv in self.pages for b in lv]
        assert np.array_equal(out.get(self.o_valid, 4 * self.nwords, np.uint32),
                              pp.bitmap_words(allv, self.nwords))
        got_vidx = out.get(self.o_vidx, 4 * self.total, np.uint32)
        got_np = out.get(self.o_npres, 8 * len(self.pages), np.int64)
        for i, ((_, _, lv), s0) in enumerate(zip(self.pages, self.slot0)):
            vidx, cnt = pp.walk_def_levels(lv)
            assert got_np[i] == cnt, f"page {i}: n_present"
            assert got_vidx[s0:s0 + len(lv)].tolist() == vidx, f"page {i}"


_PLANS = ["rle", "packed", "alternate"]


# ===========================================================================
# DELTA_BINARY_PACKED
# ===========================================================================
@pytest.mark.parametrize("esz", [8, 4])
def test_delta_bp_required(ctx, esz):
    """Every bit width 0..8*esz over four block layouts, junk widths of
    unneeded miniblocks, total > nvals, total == 1, wrapping sequences."""
    dt = {8: np.int64, 4: np.int32}[esz]
    cases = pp.dbp_cases(esz)
    pin, out = _In(), _Out()
    jobs, outs = [], []
    offs = [pin.add(c["page"]) for c in cases]
    for c in cases:
        outs.append(out.reserve(c["nvals"] * esz))
    pin.upload(ctx), out.upload(ctx)
    for c, off, o in zip(cases, offs, outs):
        jobs.append(gpu.BgDeltaBpJob(pin.at(off), out.at(o), len(c["page"]),
                                     c["nvals"], esz, 0, 0, None, None))
    _ok(ctx, ctx.L.bg_delta_bp_batch(_arr(gpu.BgDeltaBpJob, jobs), len(jobs)),
        "bg_delta_bp_batch")
    out.download(ctx)
    for c, o in zip(cases, outs):
        got = out.get(o, c["nvals"] * esz, dt)
        assert got.tolist() == c["values"], c["name"]
    out.check_guards()


@pytest.mark.parametrize("esz", [8, 4])
def test_delta_bp_nullable(ctx, esz):
    """has_def == 2: vidx / n_present come from bg_def_levels_batch in the
    same test; NULL slots keep the sentinel."""
    dt = {8: np.int64, 4: np.int32}[esz]
    bits = 8 * esz
    rng = np.random.default_rng(21 + esz)
    items = []
    for k, kind in enumerate(pp.NULL_PATTERNS):
        for n in (1, 2, 33, 129, 300):
            lv = pp.null_pattern(kind, n)
            npres = sum(lv)
            vals = pp.width_values(rng, bits - 6 - k, npres, bits) \
                if npres else []
            page = pp.with_def_levels(
                pp.rle_hybrid(lv, 1, _PLANS[(k + n) % 3]),
                pp.dbp(vals, wrap_bits=bits, block_size=128 << (n % 2)))
            items.append((f"{kind} n={n}", lv, vals, page))
    pin, out = _In(), _Out()
    offs = [pin.add(page) for *_, page in items]
    col = _Column(pin, out, [(off, len(page), lv)
                             for off, (_, lv, _, page) in zip(offs, items)])
    o_vals = out.reserve(col.total * esz)
    pin.upload(ctx), out.upload(ctx)
    col.run(ctx)
    jobs = [gpu.BgDeltaBpJob(pin.at(off), out.at(o_vals + esz * s0),
                             len(page), len(lv), esz, 2, 0, *col.ptrs(i))
            for i, (off, s0, (_, lv, _, page)) in
            enumerate(zip(offs, col.slot0, items))]
    _ok(ctx, ctx.L.bg_delta_bp_batch(_arr(gpu.BgDeltaBpJob, jobs), len(jobs)),
        "bg_delta_bp_batch")
    out.download(ctx)
    col.check()
    sent = np.frombuffer(bytes([SENT]) * esz, dtype=dt)[0]
    got = out.get(o_vals, col.total * esz, dt)
    for s0, (name, lv, vals, _) in zip(col.slot0, items):
        it = iter(vals)
        want = [next(it) if b else int(sent) for b in lv]
        assert got[s0:s0 + len(lv)].tolist() == want, name
    out.check_guards()


# ===========================================================================
# RLE / bit-packed dictionary indices
# ===========================================================================
def _with_null_slots(rng, values):
    """Definition levels that hold `values` with NULL slots in between."""
    lv = []
    for _ in values:
        lv += [0] * int(rng.choice([0, 0, 0, 1, 2])) + [1]
    return lv + [0] * int(rng.integers(0, 3))


@pytest.mark.parametrize("mode", ["required", "levels-rle", "levels-packed",
                                  "nullable"])
def test_dict_indices_batch(ctx, mode):
    """Bit widths 0..32, every count in DICT_NVALS, forced run plans (one
    bit-packed run of > 64 groups with a 2-byte header, short alternating
    runs, an RLE run longer than nvals, non-zero padding bits)."""
    cases = pp.dict_cases()
    rng = np.random.default_rng(8)
    has_def = {"required": 0, "nullable": 2}.get(mode, 1)
    pages, levels = [], []
    for c in cases:
        n = len(c["values"])
        if mode == "required":
            lv, page = [1] * n, c["body"]
        else:
            lv = _with_null_slots(rng, c["values"]) if has_def == 2 \
                else [1] * n
            plan = "alternate" if has_def == 2 else mode.split("-")[1]
            page = pp.with_def_levels(pp.rle_hybrid(lv, 1, plan), c["body"])
        pages.append(page)
        levels.append(lv)
    pin, out = _In(), _Out()
    offs = [pin.add(p) for p in pages]
    col = _Column(pin, out, [(off, len(p), lv) for off, p, lv in
                             zip(offs, pages, levels)]) if has_def == 2 \
        else None
    o_idx = [out.reserve(4 * len(lv)) for lv in levels]
    o_dense = [out.reserve(4 * len(c["values"])) if has_def == 2 else None
               for c in cases]
    pin.upload(ctx), out.upload(ctx)
    if col:
        col.run(ctx)
    jobs = []
    for i, (off, p, lv) in enumerate(zip(offs, pages, levels)):
        vp, npp = col.ptrs(i) if col else (None, None)
        jobs.append(gpu.BgDictIndicesJob(
            pin.at(off), out.at(o_idx[i]), len(p), len(lv), has_def, 0, vp,
            npp, out.at(o_dense[i]) if col else None))
    _ok(ctx, ctx.L.bg_dict_indices_batch(_arr(gpu.BgDictIndicesJob, jobs),
                                         len(jobs)), "bg_dict_indices_batch")
    out.download(ctx)
    if col:
        col.check()
    for c, lv, o in zip(cases, levels, o_idx):
        it = iter(c["values"])
        want = [next(it) if b else 0 for b in lv]   # NULL slot -> index 0
        assert out.get(o, 4 * len(lv), np.uint32).tolist() == want, c["name"]
    out.check_guards()


def test_dict_indices_single_page(ctx):
    c = next(c for c in pp.dict_cases()
             if c["name"] == "bw=17 n=1000 one packed run >64 groups")
    pin, out = _In(), _Out()
    off = pin.add(c["body"])
    o = out.reserve(4 * 1000)
    pin.upload(ctx), out.upload(ctx)
    _ok(ctx, ctx.L.bg_dict_indices(pin.at(off), len(c["body"]), 1000, 0,
                                   out.at(o)), "bg_dict_indices")
    out.download(ctx)
    assert out.get(o, 4000, np.uint32).tolist() == c["values"]
    out.check_guards()


# ===========================================================================
# definition levels
# ===========================================================================
def test_def_levels(ctx):
    """All-valid, all-null, alternating, long runs in each run kind; the
    pages lie back to back in one column, so neighbours share validity
    words (DEF_BATCHES first, e.g. 45 + 45 + 38 slots)."""
    cases = pp.def_cases()
    pin, out = _In(), _Out()
    offs = [pin.add(c["page"]) for c in cases]
    col = _Column(pin, out, [(off, len(c["page"]), c["levels"])
                             for off, c in zip(offs, cases)])
    assert col.slot0 == pp.def_bit_offsets()[0]
    pin.upload(ctx), out.upload(ctx)
    col.run(ctx)
    out.download(ctx)
    col.check()
    out.check_guards()


# ===========================================================================
# list levels, both passes
# ===========================================================================
def test_list_levels(ctx):
    """max_def 1, 2 (both shapes) and 3; NULL, empty, single- and multi-
    element rows with NULL elements; two pages per column whose row and
    entry bases are no multiples of 32."""
    cols = []
    pin, out = _In(), _Out()
    for ci, c in enumerate(pp.list_cases()):
        ln, en = c["list_nullable"], c["elem_nullable"]
        pages = []
        for pi, rows in enumerate(c["pages"]):
            rep, deff, max_def, vals = pp.rows_to_levels(rows, ln, en)
            page = pp.list_page(rep, deff, max_def,
                                pp.plain_fixed(np.array(vals, dtype=np.int32)),
                                plan=_PLANS[(ci + pi) % 3])
            want = pp.walk_list_levels(rep, deff, max_def, max_def - en, ln)
            rlen = int.from_bytes(page[:4], "little")
            pages.append(dict(off=pin.add(page), plen=len(page),
                              nslots=len(rep), want=want, rlen=rlen,
                              o_counts=out.reserve(32)))
        nrows = sum(p["want"]["rows"] for p in pages)
        nent = sum(p["want"]["entries"] for p in pages)
        cols.append(dict(
            name=c["name"], pages=pages, max_def=1 + ln + en,
            def_entry=1 + ln, def_valid=ln, nrows=nrows, nent=nent,
            o_sizes=out.reserve(4 * nrows),
            o_lvalid=out.reserve(4 * ((nrows + 31) // 32), zero=True),
            o_evalid=out.reserve(4 * ((nent + 31) // 32), zero=True),
            o_vidx=out.reserve(4 * nent)))
    pin.upload(ctx), out.upload(ctx)

    def jobs(pass_no):
        js = []
        for col in cols:
            rb = eb = 0
            for p in col["pages"]:
                js.append(gpu.BgListLevelsJob(
                    pin.at(p["off"]), p["plen"], p["nslots"], col["max_def"],
                    col["def_entry"], col["def_valid"], 0, rb, eb,
                    out.at(p["o_counts"]) if pass_no == 1 else None,
                    out.at(col["o_sizes"]), out.at(col["o_lvalid"]),
                    out.at(col["o_evalid"]), out.at(col["o_vidx"] + 4 * eb)))
                rb += p["want"]["rows"]
                eb += p["want"]["entries"]
        return _arr(gpu.BgListLevelsJob, js), len(js)

    for pass_no in (1, 2):
        _ok(ctx, ctx.L.bg_list_levels_batch(*jobs(pass_no), pass_no),
            f"bg_list_levels_batch({pass_no})")
    out.download(ctx)
    for col in cols:
        sizes, lvalid, evalid, vidx = [], [], [], []
        for p in col["pages"]:
            w = p["want"]
            assert out.get(p["o_counts"], 32, np.int64).tolist() == \
                [w["rows"], w["entries"], w["present"], p["rlen"]], col["name"]
            sizes += w["row_sizes"]
            lvalid += w["list_valid"]
            evalid += w["elem_valid"]
            vidx += w["vidx"]
        nrows, nent = col["nrows"], col["nent"]
        assert out.get(col["o_sizes"], 4 * nrows, np.int32).tolist() == sizes
        assert np.array_equal(
            out.get(col["o_lvalid"], 4 * ((nrows + 31) // 32), np.uint32),
            pp.bitmap_words(lvalid, (nrows + 31) // 32)), col["name"]
        assert np.array_equal(
            out.get(col["o_evalid"], 4 * ((nent + 31) // 32), np.uint32),
            pp.bitmap_words(evalid, (nent + 31) // 32)), col["name"]
        assert out.get(col["o_vidx"], 4 * nent, np.uint32).tolist() == vidx, \
            col["name"]
    out.check_guards()


# ===========================================================================
# PLAIN fixed width, FLBA decimals, BYTE_STREAM_SPLIT
# ===========================================================================
def _fixed_items():
    """[(name, src_esz, flba_reverse, out_esz, [src value bytes],
    [expected out bytes])] -- one entry per value, so a mode can drop some."""
    items = []
    for c in pp.fixed_cases():
        vals = pp.decode_plain_fixed(c["raw"], c["n"], c["esz"])
        items.append((c["name"], c["esz"], 0, c["esz"], vals, vals))
    for c in pp.flba_cases():
        w = c["width"]
        src = [int(v).to_bytes(w, "big", signed=True) for v in c["ints"]]
        dec = [int(v).to_bytes(16, "little", signed=True) for v in c["ints"]]
        items.append((c["name"], w, 1, 16, src, dec))
        items.append((c["name"] + " raw", w, 0, w, src, src))
    return items


def _run_fixed(ctx, entry, items, mode, encode):
    """items as _fixed_items(); mode 0 / 1 / 2; encode(src values) -> body."""
    pin, out = _In(), _Out()
    pages, levels = [], []
    for k, (name, _, _, _, src, _) in enumerate(items):
        n = len(src)
        lv = pp.null_pattern(pp.NULL_PATTERNS[k % 5], n) if mode == 2 \
            else [1] * n
        body = encode([s for s, b in zip(src, lv) if b])
        pages.append(body if mode == 0 else pp.with_def_levels(
            pp.rle_hybrid(lv, 1, _PLANS[k % 3]), body))
        levels.append(lv)
    offs = [pin.add(p) for p in pages]
    col = _Column(pin, out, [(off, len(p), lv) for off, p, lv in
                             zip(offs, pages, levels)]) if mode == 2 else None
    outs = [out.reserve(len(it[4]) * it[3]) for it in items]
    pin.upload(ctx), out.upload(ctx)
    if col:
        col.run(ctx)
    jobs = []
    for i, (it, off, p, o) in enumerate(zip(items, offs, pages, outs)):
        vp, npp = col.ptrs(i) if col else (None, None)
        jobs.append(gpu.BgPageExtractJob(pin.at(off), out.at(o), len(p),
                                         len(it[4]), it[1], mode, it[2], vp,
                                         npp))
    fn = getattr(ctx.L, entry)
    _ok(ctx, fn(_arr(gpu.BgPageExtractJob, jobs), len(jobs)), entry)
    out.download(ctx)
    if col:
        col.check()
    for it, lv, o in zip(items, levels, outs):
        name, _, _, oesz, src, exp = it
        present = iter([e for e, b in zip(exp, lv) if b])
        want = b"".join(next(present) if b else bytes([SENT]) * oesz
                        for b in lv)
        assert out.get(o, len(src) * oesz).tobytes() == want, (name, mode)
    out.check_guards()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_plain_and_flba_extract(ctx, mode):
    """src_esz 1..16 with and without flba_reverse (min, max, -1, 0, 1 and
    random: the sign byte decides the extension), 4- and 8-byte values at
    wave-boundary counts; modes 0 (required), 1 (all-present levels), 2."""
    _run_fixed(ctx, "bg_page_extract_batch", _fixed_items(), mode, b"".join)


@pytest.mark.parametrize("mode", [0, 2])
def test_byte_stream_split(ctx, mode):
    """esz 4 and 8, bit-exact over NaN payloads, +-0 and denormals."""
    items = [it for it in _fixed_items() if it[1] in (4, 8) and not it[2]
             and not it[0].endswith(" raw")]

    def encode(src):
        n = len(src)
        return bytes(src[i][k] for k in range(len(src[0]) if n else 0)
                     for i in range(n))
    _run_fixed(ctx, "bg_bss_batch", items, mode, encode)


# ===========================================================================
# BYTE_ARRAY: PLAIN / DELTA_LENGTH / DELTA_BYTE_ARRAY -> bg_ba_materialize
# ===========================================================================
_BA_ENCODERS = {0: pp.plain_byte_array, 6: pp.delta_length_byte_array,
                7: pp.delta_byte_array}


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("enc", [0, 6, 7])
def test_byte_arrays(ctx, enc, mode):
    """Every page of every ba_cases() column laid out as ONE column: Arrow
    offsets continue across pages, the encoding-7 prefix chain restarts at
    each page and skips NULL slots.  Mode 0 takes the NULL-free pages."""
    pages = [p for c in pp.ba_cases() for p in c["pages"]
             if mode == 2 or None not in p]
    pin, out = _In(), _Out()
    enc_pages, levels = [], []
    for k, p in enumerate(pages):
        lv = [int(s is not None) for s in p]
        body = _BA_ENCODERS[enc]([s for s in p if s is not None])
        enc_pages.append(body if mode == 0 else pp.with_def_levels(
            pp.rle_hybrid(lv, 1, _PLANS[k % 3]), body))
        levels.append(lv)
    offs = [pin.add(p) for p in enc_pages]
    col = _Column(pin, out, [(off, len(p), lv) for off, p, lv in
                             zip(offs, enc_pages, levels)]) if mode == 2 \
        else None
    slots = [s or b"" for p in pages for s in p]
    n = len(slots)
    total = sum(len(s) for s in slots)
    o_lens, o_src = out.reserve(8 * n), out.reserve(8 * n)
    o_offs, o_data = out.reserve(4 * (n + 1)), out.reserve(total)
    pin.upload(ctx), out.upload(ctx)
    if col:
        col.run(ctx)

    def jobs(with_out):
        js, s0 = [], 0
        for i, (off, p, lv) in enumerate(zip(offs, enc_pages, levels)):
            vp, npp = col.ptrs(i) if col else (None, None)
            common = (pin.at(off), out.at(o_lens + 8 * s0),
                      out.at(o_src + 8 * s0))
            if enc == 0:
                js.append(gpu.BgBaPageJob(*common, len(p), len(lv), mode, 0,
                                          vp, npp))
            else:
                js.append(gpu.BgDeltaBaJob(
                    *common, out.at(o_offs + 4 * s0) if with_out else None,
                    out.at(o_data) if with_out else None, len(p), len(lv),
                    mode, enc, vp, npp))
            s0 += len(lv)
        return js

    if enc == 0:
        _ok(ctx, ctx.L.bg_ba_extract_batch(_arr(gpu.BgBaPageJob, jobs(0)),
                                           len(pages)), "bg_ba_extract_batch")
    else:
        _ok(ctx, ctx.L.bg_delta_ba_batch(_arr(gpu.BgDeltaBaJob, jobs(0)),
                                         len(pages), 1), "bg_delta_ba_batch(1)")
    tot = ctypes.c_int64()
    _ok(ctx, ctx.L.bg_ba_materialize(out.at(o_lens), out.at(o_src), n,
                                     out.at(o_offs), out.at(o_data), total,
                                     ctypes.byref(tot)), "bg_ba_materialize")
    assert tot.value == total
    if enc == 7:
        _ok(ctx, ctx.L.bg_delta_ba_batch(_arr(gpu.BgDeltaBaJob, jobs(1)),
                                         len(pages), 2), "bg_delta_ba_batch(2)")
    out.download(ctx)
    if col:
        col.check()
    assert out.get(o_lens, 8 * n, np.int64).tolist() == \
        [len(s) for s in slots]                      # NULL slot -> length 0
    want_offs = np.concatenate(([0], np.cumsum([len(s) for s in slots])))
    assert out.get(o_offs, 4 * (n + 1), np.int32).tolist() == \
        want_offs.tolist()
    assert out.get(o_data, total).tobytes() == b"".join(slots)
    out.check_guards()


# ===========================================================================
# malformed pages: rejected, not read past
# ===========================================================================
_ENTRY_NAME = {"delta_bp": "bg_delta_bp_batch", "dict": "bg_dict_indices_batch",
               "def": "bg_def_levels_batch", "list": "bg_list_levels_batch",
               "extract": "bg_page_extract_batch", "bss": "bg_bss_batch",
               "ba": "bg_ba_extract_batch", "delta_ba": "bg_delta_ba_batch"}


def _run_one(ctx, entry, page, nvals, kw):
    """One single-job batch call; outputs are sized for nvals, so whatever
    a kernel writes before it rejects stays inside them.  -> (rc, result
    or None): result is what a valid page of this entry decodes to."""
    L = ctx.L
    pin, out = _In(), _Out()
    off = pin.add(page)
    has_def = kw.get("has_def", 0)
    plen = len(page)
    if entry == "delta_bp":
        esz = kw["esz"]
        o = out.reserve(nvals * esz)
        pin.upload(ctx), out.upload(ctx)
        rc = L.bg_delta_bp_batch(_arr(gpu.BgDeltaBpJob, [gpu.BgDeltaBpJob(
            pin.at(off), out.at(o), plen, nvals, esz, has_def, 0, None,
            None)]), 1)
        res = lambda: out.get(o, nvals * esz, np.int64).tolist()
    elif entry == "dict":
        o = out.reserve(4 * nvals)
        pin.upload(ctx), out.upload(ctx)
        rc = L.bg_dict_indices_batch(_arr(gpu.BgDictIndicesJob, [
            gpu.BgDictIndicesJob(pin.at(off), out.at(o), plen, nvals, has_def,
                                 0, None, None, None)]), 1)
        res = lambda: out.get(o, 4 * nvals, np.uint32).tolist()
    elif entry == "def":
        o_v = out.reserve(4 * nvals)
        o_b = out.reserve(4 * ((nvals + 31) // 32 + 1), zero=True)
        o_n = out.reserve(8)
        pin.upload(ctx), out.upload(ctx)
        rc = L.bg_def_levels_batch(_arr(gpu.BgDefLevelsJob, [
            gpu.BgDefLevelsJob(pin.at(off), out.at(o_v), out.at(o_b), plen,
                               nvals, 5, out.at(o_n))]), 1)
        res = lambda: (out.get(o_v, 4 * nvals, np.uint32).tolist(),
                       int(out.get(o_n, 8, np.int64)[0]))
    elif entry == "list":
        o = out.reserve(32)
        pin.upload(ctx), out.upload(ctx)
        md = kw["max_def"]
        rc = L.bg_list_levels_batch(_arr(gpu.BgListLevelsJob, [
            gpu.BgListLevelsJob(pin.at(off), plen, nvals, md, md, 0, 0, 0, 0,
                                out.at(o), None, None, None, None)]), 1, 1)
        res = lambda: out.get(o, 32, np.int64).tolist()[:3]
    elif entry in ("extract", "bss"):
        esz = kw["src_esz"]
        o = out.reserve(nvals * esz)
        pin.upload(ctx), out.upload(ctx)
        fn = L.bg_page_extract_batch if entry == "extract" else L.bg_bss_batch
        rc = fn(_arr(gpu.BgPageExtractJob, [gpu.BgPageExtractJob(
            pin.at(off), out.at(o), plen, nvals, esz, has_def, 0, None,
            None)]), 1)
        res = lambda: out.get(o, nvals * esz).tobytes()
    else:
        o_l, o_s = out.reserve(8 * nvals), out.reserve(8 * nvals)
        pin.upload(ctx), out.upload(ctx)
        if entry == "ba":
            rc = L.bg_ba_extract_batch(_arr(gpu.BgBaPageJob, [gpu.BgBaPageJob(
                pin.at(off), out.at(o_l), out.at(o_s), plen, nvals, has_def, 0,
                None, None)]), 1)
        else:
            rc = L.bg_delta_ba_batch(_arr(gpu.BgDeltaBaJob, [gpu.BgDeltaBaJob(
                pin.at(off), out.at(o_l), out.at(o_s), None, None, plen, nvals,
                has_def, kw["enc"], None, None)]), 1, 1)
        res = lambda: out.get(o_l, 8 * nvals, np.int64).tolist()
    err = L.bg_last_error().decode() if rc else ""
    out.download(ctx)
    out.check_guards()
    return rc, err, (res() if rc == 0 else None)


def _valid_probe(entry):
    """(page, nvals, kw, expected result) of a small valid page."""
    strs = [b"alpha", b"alphabet", b"alpine", b"beta"]
    if entry == "delta_bp":
        v = [100 + i * i for i in range(40)]
        return pp.dbp(v), 40, dict(esz=8), v
    if entry == "dict":
        v = [i % 50 for i in range(40)]
        return bytes([6]) + pp.rle_hybrid(v, 6, "packed"), 40, {}, v
    if entry == "def":
        lv = [1, 0] * 20
        return pp.with_def_levels(pp.rle_hybrid(lv, 1, "packed"), b""), 40, \
            {}, pp.walk_def_levels(lv)
    if entry == "list":
        rep, deff = [0, 1, 1, 0, 0, 1], [2, 2, 2, 1, 2, 2]
        return pp.list_page(rep, deff, 2, b""), 6, dict(max_def=2), [3, 5, 5]
    if entry in ("extract", "bss"):
        a = np.arange(40, dtype=np.int64) * 0x0102030405
        body = pp.plain_fixed(a) if entry == "extract" \
            else pp.byte_stream_split(a)
        return body, 40, dict(src_esz=8), a.tobytes()
    if entry == "ba":
        return pp.plain_byte_array(strs), 4, {}, [5, 8, 6, 4]
    return pp.delta_byte_array(strs), 4, dict(enc=7), [5, 8, 6, 4]


@pytest.mark.parametrize("entry", sorted(_ENTRY_NAME))
def test_malformed_pages_are_rejected(ctx, entry):
    """Each page has one named defect (pp.malformed_cases()).  Reject means
    a non-zero return, a bg_last_error naming the entry point, and a valid
    batch right after it still decoding correctly.  Every page is uploaded
    with pp.SLACK zero bytes behind it and corrupt lengths stay inside the
    slack, so a missed bound shows up as a wrong answer.

    The truncated final bit-packed group (a run whose declared byte count
    runs past the page) stays a reject: some writers emit it, but
    bg_dict_indices* does not accept it."""
    cases = [c for c in pp.malformed_cases() if c["entry"] == entry]
    assert cases
    ppage, pn, pkw, pwant = _valid_probe(entry)
    for c in cases:
        rc, err, _ = _run_one(ctx, entry, c["page"], c["nvals"], c["kw"])
        assert rc != 0, f"accepted: {c['name']}"
        assert err.startswith(_ENTRY_NAME[entry]), (c["name"], err)
        rc, err, got = _run_one(ctx, entry, ppage, pn, pkw)
        assert rc == 0, f"valid page refused after {c['name']}: {err}"
        assert got == pwant, f"wrong decode after {c['name']}"
