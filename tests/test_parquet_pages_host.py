"""CPU tests of tests/parquet_pages.py: the page builder and the reference
decoders the GPU page tests (test_gpu_parquet_pages.py) compare against.

Three layers:
  * round trip: every encoder through its decoder over the shared case
    tables;
  * cross-check: the decoders read page bodies pyarrow wrote (pulled out
    with the project's host page walker) and must give what pyarrow reads
    back -- without this the GPU tests would only compare the kernels with
    an encoder/decoder pair nothing outside had checked;
  * case-table invariants: each named case really has, in its encoded
    bytes, the feature it is named for.
"""
import decimal
import struct

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_pages as pp
from datafusion_ballista_amd.parquet import parse_page_header


# ===========================================================================
# round trip
# ===========================================================================
def test_varint_zigzag_round_trip():
    for v in [0, 1, 127, 128, 300, 2 ** 32, 2 ** 63, 2 ** 64 - 1]:
        assert pp._Cur(pp.uvarint(v)).varint() == v
    for v in [0, -1, 1, -2, pp.INT64_MIN, pp.INT64_MAX, 12345, -12345]:
        assert pp._Cur(pp.uvarint(pp.zigzag(v))).svarint() == v
    assert [pp.zigzag(v) for v in (0, -1, 1, -2, 2)] == [0, 1, 2, 3, 4]
    assert pp.uvarint(300) == b"\xac\x02"  # the spec's worked example


@pytest.mark.parametrize("esz", [8, 4])
def test_dbp_round_trip(esz):
    for c in pp.dbp_cases(esz):
        vals, end = pp.decode_dbp(c["page"], 0, c["bits"])
        assert end == len(c["page"]), c["name"]
        assert vals == c["all_values"], c["name"]
        assert vals[:c["nvals"]] == c["values"], c["name"]


def test_dict_round_trip():
    for c in pp.dict_cases():
        body = c["body"]
        assert body[0] == c["bw"]
        vals, _ = pp.decode_rle_hybrid(body, c["bw"], len(c["values"]), 1)
        assert vals == c["values"], c["name"]


def test_def_and_list_round_trip():
    for c in pp.def_cases():
        lv, body = pp.split_def_levels(c["page"])
        assert body == b""
        assert pp.decode_rle_hybrid(lv, 1, len(c["levels"]))[0] == c["levels"]
    for c in pp.list_cases():
        for rows in c["pages"]:
            rep, deff, max_def, vals = pp.rows_to_levels(
                rows, c["list_nullable"], c["elem_nullable"])
            body = pp.plain_fixed(np.array(vals, dtype=np.int32))
            r, d, b = pp.split_list_page(pp.list_page(rep, deff, max_def, body))
            assert b == body
            assert pp.decode_rle_hybrid(r, 1, len(rep))[0] == rep
            assert pp.decode_rle_hybrid(
                d, max_def.bit_length(), len(deff))[0] == deff
            assert _rows_from_levels(rep, deff, c["list_nullable"],
                                     c["elem_nullable"], vals) == rows


def test_fixed_round_trip():
    for c in pp.flba_cases():
        page = pp.flba_be(c["ints"], c["width"])
        assert pp.decode_flba_be(page, len(c["ints"]), c["width"]) == c["ints"]
    for c in pp.fixed_cases():
        dt = {4: np.uint32, 8: np.uint64}[c["esz"]]
        arr = np.frombuffer(c["raw"], dtype=dt)
        assert pp.plain_fixed(arr) == c["raw"]
        assert b"".join(pp.decode_plain_fixed(c["raw"], c["n"], c["esz"])) \
            == c["raw"]
        assert pp.decode_byte_stream_split(
            pp.byte_stream_split(arr), c["n"], c["esz"]) == c["raw"]


def test_byte_array_round_trip():
    for c in pp.ba_cases():
        for page in c["pages"]:
            strs = [s for s in page if s is not None]
            enc = pp.plain_byte_array(strs)
            assert pp.decode_plain_byte_array(enc, len(strs)) == \
                (strs, len(enc))
            enc = pp.delta_length_byte_array(strs)
            assert pp.decode_delta_length_byte_array(enc) == (strs, len(enc))
            enc = pp.delta_byte_array(strs)
            assert pp.decode_delta_byte_array(enc) == (strs, len(enc))


# ===========================================================================
# cross-check against pages pyarrow writes
# ===========================================================================
def _pages(path, col):
    """[(page_type, nvals, encoding, body bytes)] of column `col`, every row
    group, via the project's page-header walker (V1, uncompressed)."""
    raw = open(path, "rb").read()
    md = pq.ParquetFile(path).metadata
    out = []
    for rg in range(md.num_row_groups):
        m = md.row_group(rg).column(col)
        assert m.compression == "UNCOMPRESSED"
        start = m.data_page_offset
        if m.has_dictionary_page and m.dictionary_page_offset is not None:
            start = min(start, m.dictionary_page_offset)
        pos, end = start, start + m.total_compressed_size
        while pos < end:
            h, data_pos = parse_page_header(raw, pos)
            ptype, usz, csz = h.get(1, 0), h[2], h[3]
            assert usz == csz and ptype in (0, 2)
            if ptype == 2:
                out.append((2, h[7].get(1, 0), h[7].get(2, 0),
                            raw[data_pos:data_pos + csz]))
            else:
                out.append((0, h[5].get(1, 0), h[5].get(2, 0),
                            raw[data_pos:data_pos + csz]))
            pos = data_pos + csz
    return out


def _write(tmp_path, name, arr, nullable, encoding=None, use_dictionary=False):
    field = pa.field("c", arr.type, nullable=nullable)
    table = pa.Table.from_arrays([arr], schema=pa.schema([field]))
    path = str(tmp_path / f"{name}.parquet")
    kw = {}
    if encoding:
        kw["column_encoding"] = {"c": encoding}
    pq.write_table(table, path, compression="NONE", data_page_version="1.0",
                   use_dictionary=use_dictionary, write_statistics=False,
                   data_page_size=2048, write_batch_size=512, **kw)
    return path, pq.read_table(path).column("c").to_pylist()


def _decode_column(pages, nullable, decode_values, want_enc):
    """Reference-decode every data page; -> python list with None."""
    out, dictionary = [], None
    for ptype, nvals, enc, body in pages:
        if ptype == 2:
            dictionary = decode_values(body, nvals, 0)
            continue
        if nullable:
            lv, body = pp.split_def_levels(body)
            levels, _ = pp.decode_rle_hybrid(lv, 1, nvals)
        else:
            levels = [1] * nvals
        npres = sum(levels)
        assert enc in want_enc, enc
        if enc in (2, 8):  # PLAIN_DICTIONARY / RLE_DICTIONARY
            idx, _ = pp.decode_rle_hybrid(body, body[0], npres, 1)
            vals = [dictionary[i] for i in idx]
        else:
            vals = decode_values(body, npres, enc)
        it = iter(vals)
        out += [next(it) if lv else None for lv in levels]
    return out


def _with_nulls(values, nullable, seed):
    if not nullable:
        return list(values)
    rng = np.random.default_rng(seed)
    keep = rng.integers(0, 4, len(values)) > 0
    keep[:40] = False          # a long all-null stretch: RLE runs of 0
    keep[100:200] = True
    return [v if k else None for v, k in zip(values, keep)]


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("bits", [32, 64])
def test_pyarrow_delta_binary_packed(tmp_path, nullable, bits):
    rng = np.random.default_rng(bits)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = [int(v) for v in rng.integers(lo, hi, 3000, dtype=np.int64)]
    vals[10:14] = [hi, lo, hi, lo]                    # wrapping deltas
    vals[500:900] = range(7, 407)                     # width-0 miniblocks
    vals[900:1300] = [int(v) for v in rng.integers(0, 9, 400)]  # narrow
    data = _with_nulls(vals, nullable, 1)
    typ = pa.int32() if bits == 32 else pa.int64()
    path, want = _write(tmp_path, "dbp", pa.array(data, type=typ), nullable,
                        "DELTA_BINARY_PACKED")
    pages = _pages(path, 0)
    assert len(pages) > 1

    def dec(body, n, enc):
        v, _ = pp.decode_dbp(body, 0, bits)
        assert len(v) == n
        return v
    assert _decode_column(pages, nullable, dec, {5}) == want


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("enc_name,enc", [("PLAIN", 0),
                                          ("DELTA_LENGTH_BYTE_ARRAY", 6),
                                          ("DELTA_BYTE_ARRAY", 7)])
def test_pyarrow_byte_arrays(tmp_path, nullable, enc_name, enc):
    rng = np.random.default_rng(9)
    vals = []
    for i in range(1500):
        k = int(rng.integers(0, 6))
        if k == 0:
            vals.append(b"")
        elif k == 1 and vals:
            vals.append(vals[-1])                     # whole-previous prefix
        elif k == 2 and vals:
            vals.append(vals[-1][:int(rng.integers(0, 9))] + rng.bytes(3))
        else:
            vals.append(b"key-%04d-" % (i // 7) + rng.bytes(int(k)))
    vals[77] = bytes(range(256)) * 2
    data = _with_nulls(vals, nullable, 2)
    path, want = _write(tmp_path, "ba", pa.array(data, type=pa.binary()),
                        nullable, enc_name)
    pages = _pages(path, 0)
    assert len(pages) > 1

    def dec(body, n, e):
        if e == 0:
            return pp.decode_plain_byte_array(body, n)[0]
        v = (pp.decode_delta_length_byte_array if e == 6
             else pp.decode_delta_byte_array)(body)[0]
        assert len(v) == n
        return v
    assert _decode_column(pages, nullable, dec, {enc}) == want


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("typ", [pa.float32(), pa.float64()])
@pytest.mark.parametrize("enc_name,enc", [("PLAIN", 0),
                                          ("BYTE_STREAM_SPLIT", 9)])
def test_pyarrow_fixed_width(tmp_path, nullable, typ, enc_name, enc):
    npt = np.float32 if typ == pa.float32() else np.float64
    esz = np.dtype(npt).itemsize
    vals = [float(v) for v in
            np.random.default_rng(4).standard_normal(2000).astype(npt)]
    vals[3:6] = [0.0, -0.0, float(np.finfo(npt).tiny) / 4]
    data = _with_nulls(vals, nullable, 3)
    path, want = _write(tmp_path, "fx", pa.array(data, type=typ), nullable,
                        enc_name)

    def dec(body, n, e):
        raw = (b"".join(pp.decode_plain_fixed(body, n, esz)) if e == 0
               else pp.decode_byte_stream_split(body, n, esz))
        return list(np.frombuffer(raw, dtype=npt))

    def bits(lst):
        return [None if v is None else npt(v).tobytes() for v in lst]
    got = _decode_column(_pages(path, 0), nullable, dec, {enc})
    assert bits(got) == bits(want)


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("precision", [2, 9, 15, 18, 29, 38])
def test_pyarrow_flba_decimal(tmp_path, nullable, precision):
    rng = np.random.default_rng(precision)
    top = 10 ** precision - 1
    ints = [top, -top, -1, 0, 1] + [
        int(rng.integers(-2 ** 62, 2 ** 62)) % (top + 1) * (-1) ** i
        for i in range(600)]
    data = _with_nulls([decimal.Decimal(v) for v in ints], nullable, 5)
    path, want = _write(tmp_path, "dec",
                        pa.array(data, type=pa.decimal128(precision, 0)),
                        nullable, "PLAIN")
    width = pq.ParquetFile(path).schema.column(0).length
    assert 1 <= width <= 16

    def dec(body, n, e):
        return [decimal.Decimal(v) for v in pp.decode_flba_be(body, n, width)]
    assert _decode_column(_pages(path, 0), nullable, dec, {0}) == want


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("card", [1, 2, 3, 200, 40000])
def test_pyarrow_dictionary(tmp_path, nullable, card):
    rng = np.random.default_rng(card)
    vals = [int(v) * 1000003 for v in rng.integers(0, card, 6000)]
    vals[1000:1800] = [vals[1000]] * 800              # a long RLE run
    if card == 40000:
        vals = list(range(40000)) + vals              # every index, width 16
    data = _with_nulls(vals, nullable, 6)
    path, want = _write(tmp_path, "dict", pa.array(data, type=pa.int64()),
                        nullable, use_dictionary=True)
    pages = _pages(path, 0)
    assert pages[0][0] == 2

    def dec(body, n, e):
        return [struct.unpack("<q", b)[0]
                for b in pp.decode_plain_fixed(body, n, 8)]
    assert any(t == 0 and e in (2, 8) for t, _, e, _ in pages), \
        "no dictionary-coded data page was written"
    assert _decode_column(pages, nullable, dec, {0, 2, 8}) == want


def _rows_from_levels(rep, deff, ln, en, vals):
    """Rebuild list rows from rep/def levels (parquet-format Nested
    Encoding), by a walk of its own."""
    rows, it = [], iter(vals)
    max_def = 1 + ln + en
    for r, d in zip(rep, deff):
        if r == 0:
            if ln and d == 0:
                rows.append(None)
                continue
            rows.append([])
            if d == ln:
                continue
        rows[-1].append(next(it) if d == max_def else None)
    return rows


@pytest.mark.parametrize("ln,en", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pyarrow_list_levels(tmp_path, ln, en):
    case = next(c for c in pp.list_cases()
                if (c["list_nullable"], c["elem_nullable"]) == (ln, en))
    rows = [r for page in case["pages"] for r in page] * 9
    typ = pa.list_(pa.field("element", pa.int32(), nullable=bool(en)))
    path, want = _write(tmp_path, "list", pa.array(rows, type=typ), bool(ln),
                        "PLAIN")
    sc = pq.ParquetFile(path).schema.column(0)
    max_def = sc.max_definition_level
    assert (sc.max_repetition_level, max_def) == (1, 1 + ln + en)
    got = []
    for ptype, nslots, enc, body in _pages(path, 0):
        r, d, vals = pp.split_list_page(body)
        rep, _ = pp.decode_rle_hybrid(r, 1, nslots)
        deff, _ = pp.decode_rle_hybrid(d, max_def.bit_length(), nslots)
        npres = sum(1 for x in deff if x == max_def)
        ints = [struct.unpack("<i", b)[0]
                for b in pp.decode_plain_fixed(vals, npres, 4)]
        got += _rows_from_levels(rep, deff, ln, en, ints)
        # the direct walk the GPU test compares the kernel with
        w = pp.walk_list_levels(rep, deff, max_def, max_def - en, ln)
        page_rows = got[len(got) - w["rows"]:]
        assert w["row_sizes"] == [len(x or []) for x in page_rows]
        assert w["list_valid"] == [int(x is not None) for x in page_rows]
        assert w["elem_valid"] == [int(e is not None)
                                   for x in page_rows for e in (x or [])]
        assert w["present"] == npres
    assert got == want == rows


# ===========================================================================
# case-table invariants, asserted on the encoded bytes
# ===========================================================================
def _dbp_layout(page):
    """-> (block_size, miniblocks, total, [first block's width bytes])."""
    cur = pp._Cur(page)
    bs, mb, total = cur.varint(), cur.varint(), cur.varint()
    cur.svarint()
    if total <= 1:
        return bs, mb, total, []
    cur.svarint()
    return bs, mb, total, list(cur.take(mb))


@pytest.mark.parametrize("esz", [8, 4])
def test_dbp_case_table_invariants(esz):
    bits = 8 * esz
    cases = {c["name"]: c for c in pp.dbp_cases(esz)}
    assert len(cases) == len(pp.dbp_cases(esz)), "duplicate case names"
    seen = {bw: [] for bw in range(bits + 1)}
    for name, c in cases.items():
        if not name.startswith("bw="):
            continue
        bw = int(name.split()[0][3:])
        bs, mb, total, widths = _dbp_layout(c["page"])
        assert f"layout={bs}/{mb}" in name and f"n={total}" in name
        if total > 1:
            assert widths[0] == bw, name
            seen[bw].append(((bs, mb), total))
    for bw, got in seen.items():
        assert len({lay for lay, _ in got}) >= 2, f"bw={bw}: one layout only"
        counts = {n for _, n in got}
        assert {33, 257} <= counts, f"bw={bw}: counts {counts}"
    assert {lay for got in seen.values() for lay, _ in got} == \
        set(pp.DBP_LAYOUTS)
    assert {c["nvals"] for c in cases.values()} >= set(pp.DBP_COUNTS)
    # bw + shift > 64: an unaligned value of >= 58 bits must exist
    if esz == 8:
        assert any(len(seen[bw]) for bw in range(58, 64))

    bs, mb, total, widths = _dbp_layout(cases["junk widths n=33"]["page"])
    assert widths[1:] == [0xFF] * (mb - 1) and widths[0] <= 64
    c = cases["total>nvals"]
    assert _dbp_layout(c["page"])[2] > c["nvals"]
    assert _dbp_layout(cases["total==1"]["page"])[2] == 1
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    assert cases["wrap max->min"]["values"][1:3] == [hi, lo]
    # full-width deltas under a minimal min_delta: the top-width cases
    c = cases[f"bw={bits} layout=128/4 n=33"]
    cur = pp._Cur(c["page"])
    for _ in range(3):
        cur.varint()
    cur.svarint()
    assert cur.svarint() == lo, "min_delta is not the type's minimum"
    if esz == 4:
        a = cases["int32 wrap, 32-bit deltas"]
        b = cases["int32 wrap, 64-bit deltas"]
        assert a["values"] == b["values"] and a["page"] != b["page"]
        assert max(_dbp_layout(a["page"])[3]) <= 32
        assert max(_dbp_layout(b["page"])[3]) > 32


def test_dict_case_table_invariants():
    cases = {c["name"]: c for c in pp.dict_cases()}
    assert len(cases) == len(pp.dict_cases()), "duplicate case names"
    assert {c["bw"] for c in cases.values()} == set(range(33))
    assert {len(c["values"]) for c in cases.values()} >= set(pp.DICT_NVALS)
    for name, c in cases.items():
        body, bw, n = c["body"], c["bw"], len(c["values"])
        assert body[0] == bw
        cur = pp._Cur(body, 1)
        if ">64 groups" in name:
            h = cur.varint()
            assert h & 1 and (h >> 1) >= 65 and cur.pos == 3  # 2-byte header
        if "non-zero padding" in name:
            h = cur.varint()
            groups = h >> 1
            assert h & 1 and groups * 8 > n
            allv = pp._unpack(cur.take(groups * bw), bw, groups * 8)
            assert all(v != 0 for v in allv[n:]), name
        if "2-byte header" in name:
            h = cur.varint()
            assert not h & 1 and cur.pos == 3
        if "longer than nvals" in name:
            h = cur.varint()
            assert not h & 1 and (h >> 1) > n
        if "max index" in name:
            assert set(c["values"]) == {0xFFFFFFFF}
    assert any(c["plan"] == "alternate" and len(c["values"]) > 100
               for c in cases.values())
    # every width's all-ones index is really there (a narrow mask would show)
    for bw in range(1, 33):
        assert any(c["bw"] == bw and (1 << bw) - 1 in c["values"]
                   for c in cases.values()), bw


def test_def_case_table_invariants():
    cases = pp.def_cases()
    offs, total = pp.def_bit_offsets()
    assert total == sum(len(c["levels"]) for c in cases)
    k = 0
    for batch in pp.DEF_BATCHES:
        for j, n in enumerate(batch):
            c = cases[k]
            assert c["name"].startswith("shared word") and \
                len(c["levels"]) == n
            if j:  # shares a validity word with the page before it
                assert offs[k] % 32 != 0, (c["name"], offs[k])
            k += 1
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for kind, want in (("valid", {1}), ("null", {0})):
        for n in pp.DEF_NVALS:
            for plan in ("rle", "packed", "alternate"):
                c = cases[names.index(f"{kind} n={n} {plan}")]
                assert set(c["levels"]) == want and len(c["levels"]) == n
    for c in cases:   # the run kind the plan names is in the bytes
        lv, _ = pp.split_def_levels(c["page"])
        first = pp._Cur(lv).varint()
        if c["plan"] == "packed":
            assert first & 1 and (first >> 1) == (len(c["levels"]) + 7) // 8
        else:
            assert not first & 1


def test_list_and_ba_case_table_invariants():
    for c in pp.list_cases():
        ln, en = c["list_nullable"], c["elem_nullable"]
        rows = [r for p in c["pages"] for r in p]
        assert any(r == [] for r in rows)
        assert any(r is not None and len(r) == 1 for r in rows)
        assert any(r is not None and len(r) > 1 for r in rows)
        assert any(r is None for r in rows) == bool(ln)
        assert any(r and None in r and len(r) > 1 for r in rows) == bool(en)
        first = c["pages"][0]
        assert len(first) % 32 and sum(len(r or []) for r in first) % 32
    ba = {c["name"]: c["pages"] for c in pp.ba_cases()}
    assert len(ba["two pages"]) == 2
    p = ba["nulls between strings"][0]
    assert p[0] is None and p[-1] is None and None in p[1:-1]
    assert any(len(s) > 255 for s in ba["prefix 0 after a long string"][0])
    eq = [s for s in ba["all equal lengths (width-0 miniblocks)"][0]]
    enc = pp.delta_length_byte_array(eq)
    assert _dbp_layout(enc)[3][0] == 0
    enc = pp.delta_byte_array(ba["whole-previous prefix, empty suffix"][0])
    pre, p2 = pp.decode_dbp(enc)
    suf, _ = pp.decode_dbp(enc, p2)
    assert pre[1] == 6 and suf[1] == 0
    assert _dbp_layout(pp.dbp([1]))[2] == 1      # single value: total == 1


def test_flba_fixed_case_table_invariants():
    widths = {}
    for c in pp.flba_cases():
        widths.setdefault(c["width"], []).extend(c["ints"])
    assert set(widths) == set(range(1, 17))
    for w, ints in widths.items():
        lo, hi = -(1 << (8 * w - 1)), (1 << (8 * w - 1)) - 1
        assert {lo, hi, -1, 0, 1} <= set(ints), w
    assert {len(c["ints"]) for c in pp.flba_cases()} >= set(pp.FIXED_COUNTS)
    assert {(c["esz"], c["n"]) for c in pp.fixed_cases()} == \
        {(e, n) for e in (4, 8) for n in pp.FIXED_COUNTS}


def test_malformed_case_table_is_rejected_by_the_reference():
    """One named defect per page; where a reference decoder covers the
    page's encoding it must refuse the page too (or run out of values)."""
    cases = pp.malformed_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for want in ("dlen past page_len", "bit width 33", "width byte 65",
                 "miniblocks = 0", "not divisible", "total smaller",
                 "non-zero first prefix", "prefix longer", "11 continuation",
                 "byte count past the page", "truncated final bit-packed"):
        assert any(want in n for n in names), want

    def body_of(c):
        if c["kw"].get("has_def"):
            lv, body = pp.split_def_levels(c["page"])
            pp.decode_rle_hybrid(lv, 1, c["nvals"])
            return body
        return c["page"]

    for c in cases:
        n, kw = c["nvals"], c["kw"]
        with pytest.raises(ValueError):
            if c["entry"] == "delta_bp":
                vals, _ = pp.decode_dbp(body_of(c))
                if len(vals) < n:
                    raise ValueError("fewer values than asked for")
            elif c["entry"] == "dict":
                b = body_of(c)
                if not b or b[0] > 32:
                    raise ValueError("bit width")
                pp.decode_rle_hybrid(b, b[0], n, 1)
            elif c["entry"] == "def":
                lv, _ = pp.split_def_levels(c["page"])
                pp.decode_rle_hybrid(lv, 1, n)
            elif c["entry"] == "ba":
                pp.decode_plain_byte_array(body_of(c), n)
            elif c["entry"] == "delta_ba":
                dec = (pp.decode_delta_length_byte_array if kw["enc"] == 6
                       else pp.decode_delta_byte_array)
                vals, _ = dec(c["page"])
                if len(vals) < n:
                    raise ValueError("fewer values than asked for")
            elif c["entry"] == "list":
                r, d, _ = pp.split_list_page(c["page"])
                rep, _ = pp.decode_rle_hybrid(r, 1, n)
                deff, _ = pp.decode_rle_hybrid(d, 2, n)
                if max(deff) > kw["max_def"]:
                    raise ValueError("level above max_def")
            else:  # extract / bss: geometry only
                pp.decode_plain_fixed(body_of(c), n, kw["src_esz"])
        # corrupt lengths stay inside the slack uploaded after the page
        assert len(c["page"]) < 4096
