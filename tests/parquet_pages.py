"""Spec-level Parquet page builder, reference decoders and shared case tables.

Written from the parquet-format spec (Encodings.md, "Nested Encoding" in
README.md); shares no code with datafusion_ballista_amd/parquet.py or the
kernels.  The encoders build page bodies byte by byte so a test can force
any layout the format allows (bit widths, run structure, block geometry,
padding), including layouts no installed writer produces.  The decoders
are separate functions with their own cursor and bit reader, kept to plain
Python ints; tests/test_parquet_pages_host.py checks them against pages
pyarrow writes, which is what lets the GPU tests use them as the reference.

Not a test module and not a conftest: imported as `parquet_pages` from the
tests directory.
"""
import functools
import struct

import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


# ===========================================================================
# encoders
# ===========================================================================
def uvarint(v):
    """ULEB128 of a non-negative int."""
    assert v >= 0
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v):
    """Signed -> unsigned zigzag (0,-1,1,-2 -> 0,1,2,3), any precision."""
    return -2 * v - 1 if v < 0 else 2 * v


def _pack(values, bw):
    """LSB-first bit packing of `values` at `bw` bits each, whole bytes."""
    acc = 0
    for i, v in enumerate(values):
        assert 0 <= v < (1 << bw) or (bw == 0 and v == 0), (v, bw)
        acc |= v << (i * bw)
    return acc.to_bytes((len(values) * bw + 7) // 8, "little")


def rle_hybrid(values, bw, plan, pad_bits=0):
    """RLE / bit-packed hybrid with a forced run structure.

    plan: "rle"       one RLE run per stretch of equal values
          "packed"    a single bit-packed run of ceil(n/8) groups
          "alternate" RLE stretch, then one bit-packed group of 8, ...
          [(kind, count), ...]  explicit: ("rle", c) declares a run of c
              (it may exceed the values left; it consumes what is left),
              ("packed", c) packs the next c values (c % 8 == 0 except in
              the last run, whose final group is padded).
    Padding slots of a final bit-packed group hold `pad_bits` (masked to bw).
    The RLE run value takes ceil(bw/8) bytes."""
    values = [int(v) for v in values]
    n = len(values)
    if isinstance(plan, str):
        runs, pos, want_rle = [], 0, True
        if plan == "packed":
            runs = [("packed", n)]
        else:
            while pos < n:
                if plan == "rle" or want_rle:
                    e = pos
                    while e < n and values[e] == values[pos]:
                        e += 1
                    runs.append(("rle", e - pos))
                    pos = e
                else:
                    c = min(8, n - pos)
                    runs.append(("packed", c))
                    pos += c
                want_rle = not want_rle
            assert plan in ("rle", "alternate"), plan
    else:
        runs = list(plan)
    out = bytearray()
    pos = 0
    mask = (1 << bw) - 1
    for k, (kind, count) in enumerate(runs):
        if kind == "rle":
            take = min(count, n - pos)
            assert take > 0 and len(set(values[pos:pos + take])) == 1
            out += uvarint(count << 1)
            out += values[pos].to_bytes((bw + 7) // 8, "little")
            pos += take
        else:
            assert kind == "packed"
            assert count % 8 == 0 or k == len(runs) - 1
            groups = (count + 7) // 8
            chunk = values[pos:pos + count]
            chunk += [pad_bits & mask] * (groups * 8 - len(chunk))
            out += uvarint((groups << 1) | 1)
            out += _pack(chunk, bw)
            pos += min(count, n - pos)
    assert pos == n, (pos, n)
    return bytes(out)


def _wrap_signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def dbp(values, block_size=128, miniblocks=4, wrap_bits=64,
        junk_unused_widths=False, width=None, total=None):
    """DELTA_BINARY_PACKED stream.

    Deltas are taken in `wrap_bits`-bit wrapping arithmetic (an INT32
    column may be written either with 32-bit or with 64-bit deltas).  Each
    needed miniblock is packed at its minimal width, or at `width` (an int)
    when given, which must not be below the minimal one.  The last needed
    miniblock is padded to full length; unneeded trailing miniblocks have
    no data and a width byte of 0, or 0xFF with junk_unused_widths.
    `total` overrides the header's value count (malformed pages)."""
    values = [int(v) for v in values]
    n = len(values)
    assert block_size % miniblocks == 0
    mb_vals = block_size // miniblocks
    out = bytearray()
    out += uvarint(block_size) + uvarint(miniblocks)
    out += uvarint(n if total is None else total)
    out += uvarint(zigzag(values[0] if n else 0))
    deltas = [_wrap_signed(values[i + 1] - values[i], wrap_bits)
              for i in range(n - 1)]
    for b0 in range(0, len(deltas), block_size):
        block = deltas[b0:b0 + block_size]
        min_delta = min(block)
        out += uvarint(zigzag(min_delta))
        widths, bodies = [], []
        for m in range(miniblocks):
            adj = [d - min_delta for d in block[m * mb_vals:(m + 1) * mb_vals]]
            if not adj:
                widths.append(0xFF if junk_unused_widths else 0)
                continue
            w = max(a.bit_length() for a in adj)
            if width is not None:
                if width < w:
                    raise ValueError(f"width {width} below minimal {w}")
                w = width
            widths.append(w)
            bodies.append(_pack(adj + [0] * (mb_vals - len(adj)), w))
        out += bytes(widths) + b"".join(bodies)
    return bytes(out)


def delta_length_byte_array(strs, **kw):
    return dbp([len(s) for s in strs], **kw) + b"".join(strs)


def delta_byte_array(strs, prefix_lens=None):
    """DELTA_BYTE_ARRAY: DBP prefix lengths, then the suffixes as
    DELTA_LENGTH_BYTE_ARRAY.  `prefix_lens` overrides the longest-common-
    prefix choice (shorter prefixes are legal; longer ones are malformed)."""
    pre, suf, prev = [], [], b""
    for i, s in enumerate(strs):
        if prefix_lens is not None:
            p = prefix_lens[i]
        else:
            p = 0
            while p < min(len(s), len(prev)) and s[p] == prev[p]:
                p += 1
        pre.append(p)
        suf.append(s[min(p, len(s)):])
        prev = s
    return dbp(pre) + delta_length_byte_array(suf)


def plain_byte_array(strs):
    return b"".join(struct.pack("<I", len(s)) + s for s in strs)


def byte_stream_split(arr):
    a = np.ascontiguousarray(arr)
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize).T.tobytes()


def plain_fixed(arr):
    return np.ascontiguousarray(arr).astype(
        np.asarray(arr).dtype.newbyteorder("<")).tobytes()


def flba_be(ints, width):
    return b"".join(int(v).to_bytes(width, "big", signed=True) for v in ints)


def with_def_levels(levels_bytes, body):
    return struct.pack("<I", len(levels_bytes)) + levels_bytes + body


def list_page(rep, deff, max_def, body, plan="alternate"):
    r = rle_hybrid(rep, 1, plan)
    d = rle_hybrid(deff, max(1, int(max_def).bit_length()), plan)
    return struct.pack("<I", len(r)) + r + struct.pack("<I", len(d)) + d + body


# ===========================================================================
# reference decoders (own cursor + bit reader; nothing shared with the above)
# ===========================================================================
class _Cur:
    def __init__(self, buf, pos=0):
        self.buf, self.pos = bytes(buf), pos

    def take(self, n):
        if n < 0 or self.pos + n > len(self.buf):
            raise ValueError("read past the end of the page")
        s = self.buf[self.pos:self.pos + n]
        self.pos += n
        return s

    def varint(self):
        shift = result = 0
        for _ in range(10):
            (b,) = self.take(1)
            result += (b % 128) * 2 ** shift
            if b < 128:
                return result
            shift += 7
        raise ValueError("varint longer than 10 bytes")

    def svarint(self):
        u = self.varint()
        return u // 2 if u % 2 == 0 else -(u + 1) // 2


def _unpack(chunk, bw, count):
    """`count` bw-bit values from `chunk`, read bit by bit, LSB first."""
    bits = np.unpackbits(np.frombuffer(chunk, dtype=np.uint8),
                         bitorder="little")
    if count * bw > len(bits):
        raise ValueError("bit-packed data shorter than declared")
    out = []
    for i in range(count):
        v = 0
        for k in reversed(range(bw)):
            v = 2 * v + int(bits[i * bw + k])
        out.append(v)
    return out


def decode_rle_hybrid(buf, bw, nvals, pos=0):
    """-> (values[:nvals], position after the last run that was needed)."""
    cur = _Cur(buf, pos)
    out = []
    while len(out) < nvals:
        h = cur.varint()
        if h % 2:
            groups = h // 2
            out += _unpack(cur.take(groups * bw), bw, groups * 8)
        else:
            raw = cur.take((bw + 7) // 8)
            out += [int.from_bytes(raw, "little")] * (h // 2)
    return out[:nvals], cur.pos


def decode_dbp(buf, pos=0, bits=64):
    """-> (all `total` values wrapped to signed `bits`, end position).  Only
    the miniblocks that hold values are looked at, width bytes included."""
    cur = _Cur(buf, pos)
    block_size, nmb, total = cur.varint(), cur.varint(), cur.varint()
    first = cur.svarint()
    if nmb == 0 or block_size == 0 or block_size % nmb:
        raise ValueError("bad block geometry")
    per_mb = block_size // nmb
    if per_mb % 32:
        raise ValueError("miniblock size is no multiple of 32")
    if total == 0:
        return [], cur.pos
    half, mod = 2 ** (bits - 1), 2 ** bits
    vals = [(first + half) % mod - half]
    while len(vals) < total:
        min_delta = cur.svarint()
        widths = cur.take(nmb)
        for w in widths:
            left = total - len(vals)
            if left == 0:
                break
            if w > 64:
                raise ValueError(f"miniblock width {w}")
            packed = _unpack(cur.take(per_mb * w // 8), w, min(left, per_mb))
            for a in packed:
                vals.append((vals[-1] + min_delta + a + half) % mod - half)
    return vals, cur.pos


def decode_delta_length_byte_array(buf, pos=0):
    lens, p = decode_dbp(buf, pos)
    cur = _Cur(buf, p)
    if any(ln < 0 for ln in lens):
        raise ValueError("negative length")
    return [cur.take(ln) for ln in lens], cur.pos


def decode_delta_byte_array(buf, pos=0):
    pre, p = decode_dbp(buf, pos)
    suf, p = decode_delta_length_byte_array(buf, p)
    if len(pre) != len(suf):
        raise ValueError("prefix/suffix counts differ")
    out, last = [], b""
    for k, (n, s) in enumerate(zip(pre, suf)):
        if n < 0 or n > len(last) or (k == 0 and n):
            raise ValueError("prefix longer than the previous value")
        last = last[:n] + s
        out.append(last)
    return out, p


def decode_plain_byte_array(buf, n, pos=0):
    cur = _Cur(buf, pos)
    out = []
    for _ in range(n):
        (ln,) = struct.unpack("<I", cur.take(4))
        out.append(cur.take(ln))
    return out, cur.pos


def decode_byte_stream_split(buf, n, esz, pos=0):
    """-> n*esz little-endian value bytes."""
    raw = _Cur(buf, pos).take(n * esz)
    return bytes(raw[k * n + i] for i in range(n) for k in range(esz))


def decode_plain_fixed(buf, n, esz, pos=0):
    raw = _Cur(buf, pos).take(n * esz)
    return [raw[i * esz:(i + 1) * esz] for i in range(n)]


def decode_flba_be(buf, n, width, pos=0):
    """Big-endian two's-complement FLBA -> Python ints."""
    out = []
    for raw in decode_plain_fixed(buf, n, width, pos):
        v = 0
        for b in raw:
            v = v * 256 + b
        out.append(v - 256 ** width if raw[0] >= 128 else v)
    return out


def split_def_levels(page):
    """[u32 dlen][levels][body] -> (levels bytes, body bytes)."""
    cur = _Cur(page)
    (dlen,) = struct.unpack("<I", cur.take(4))
    lv = cur.take(dlen)
    return lv, page[cur.pos:]


def split_list_page(page):
    cur = _Cur(page)
    (rlen,) = struct.unpack("<I", cur.take(4))
    rep = cur.take(rlen)
    (dlen,) = struct.unpack("<I", cur.take(4))
    deff = cur.take(dlen)
    return rep, deff, page[cur.pos:]


# ---- what the level kernels must produce, by a direct walk ----
def walk_def_levels(levels):
    """-> (vidx list with 0xFFFFFFFF for NULL, n_present)."""
    vidx, cnt = [], 0
    for lv in levels:
        if lv:
            vidx.append(cnt)
            cnt += 1
        else:
            vidx.append(0xFFFFFFFF)
    return vidx, cnt


def bitmap_words(bits, nwords):
    """LSB-first u32 words of a list of 0/1."""
    w = np.zeros(nwords, dtype=np.uint32)
    for i, b in enumerate(bits):
        if b:
            w[i >> 5] |= np.uint32(1 << (i & 31))
    return w


def rows_to_levels(rows, list_nullable, elem_nullable):
    """rows: None | [] | [int or None, ...] -> (rep, def, max_def, values)."""
    ln, en = int(list_nullable), int(elem_nullable)
    max_def = 1 + ln + en
    rep, deff, vals = [], [], []
    for row in rows:
        if row is None:
            assert ln
            rep.append(0), deff.append(0)
        elif not row:
            rep.append(0), deff.append(ln)
        else:
            for k, e in enumerate(row):
                rep.append(1 if k else 0)
                if e is None:
                    assert en
                    deff.append(ln + 1)
                else:
                    deff.append(max_def)
                    vals.append(e)
    return rep, deff, max_def, vals


def walk_list_levels(rep, deff, max_def, def_entry, def_valid):
    """-> dict(rows, entries, present, row_sizes, list_valid bits,
    elem_valid bits, vidx)."""
    sizes, lvalid, evalid, vidx, present = [], [], [], [], 0
    for r, d in zip(rep, deff):
        if r == 0:
            sizes.append(0)
            lvalid.append(1 if d >= def_valid else 0)
        if d >= def_entry:
            sizes[-1] += 1
            evalid.append(1 if d == max_def else 0)
            vidx.append(present if d == max_def else 0xFFFFFFFF)
        if d == max_def:
            present += 1
    return dict(rows=len(sizes), entries=len(evalid), present=present,
                row_sizes=sizes, list_valid=lvalid, elem_valid=evalid,
                vidx=vidx)


# ===========================================================================
# case tables (shared by the host and the GPU tests; seeded, deterministic)
# ===========================================================================
DBP_LAYOUTS = [(128, 4), (256, 4), (128, 1), (512, 8)]
DBP_COUNTS = [1, 2, 32, 33, 128, 129, 257, 300]


def width_values(rng, bw, n, bits):
    """n values whose deltas, less their minimum, use every bit of a bw-bit
    field (some are all-ones, some 0); bw == bits forces deltas that span
    the whole signed range, so the running value wraps."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if bw == bits:
        min_delta = lo
    else:
        span = (1 << bw) - 1
        min_delta = int(rng.integers(max(lo, -1000), min(1000, hi - span) + 1))
    adj = [int(rng.integers(0, 1 << min(bw, 62))) << max(0, bw - 62)
           if bw else 0 for _ in range(max(n - 1, 0))]
    for i in range(0, len(adj), 8):       # both extremes in every miniblock
        adj[i] = 0
        if i + 1 < len(adj):
            adj[i + 1] = (1 << bw) - 1
    vals = [int(rng.integers(-1000, 1000))]
    for a in adj:
        vals.append(_wrap_signed(vals[-1] + min_delta + a, bits))
    return vals


@functools.lru_cache(maxsize=None)
def dbp_cases(esz):
    """[dict(name, values, nvals, page, bits, kw)] for one element size.
    `values` are the expected first `nvals` outputs."""
    bits = 8 * esz
    rng = np.random.default_rng(500 + esz)
    cases = []

    def add(name, values, nvals=None, **kw):
        kw.setdefault("wrap_bits", bits)
        nvals = len(values) if nvals is None else nvals
        cases.append(dict(name=name, values=list(values[:nvals]), nvals=nvals,
                          page=dbp(values, **kw), bits=bits, kw=kw,
                          all_values=list(values)))

    for bw in range(bits + 1):
        picks = [(DBP_LAYOUTS[bw % 4], 33), (DBP_LAYOUTS[(bw + 1) % 4], 257),
                 (DBP_LAYOUTS[(bw + 2) % 4], DBP_COUNTS[bw % 8])]
        for (bs, mb), n in picks:
            add(f"bw={bw} layout={bs}/{mb} n={n}",
                width_values(rng, bw, n, bits), block_size=bs,
                miniblocks=mb, width=bw if n > 1 else None)
    v33 = width_values(rng, 9, 33, bits)
    add("junk widths n=33", v33, junk_unused_widths=True)
    add("junk widths n=129 512/8", width_values(rng, 20, 129, bits),
        block_size=512, miniblocks=8, junk_unused_widths=True)
    add("total>nvals", width_values(rng, 13, 300, bits), nvals=100)
    add("total==1", [int(rng.integers(-99, 99))])
    add("total==1 extreme", [-(1 << (bits - 1))])
    add("n=2", [5, -7])
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    add("wrap max->min", [hi - 1, hi, lo, lo + 1, hi, lo])
    add("alternating min/max", [lo, hi] * 70)
    add("alternating max/min 256/4", [hi, lo] * 129, block_size=256)
    if esz == 4:
        seq = [hi, lo, hi - 3, lo + 3, 0, hi, lo] * 20
        add("int32 wrap, 32-bit deltas", seq, wrap_bits=32)
        add("int32 wrap, 64-bit deltas", seq, wrap_bits=64)
    return cases


DICT_NVALS = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1000]


def _runny(rng, bw, n):
    """Values in [0, 2^bw) laid out in stretches of 1..12 equal values,
    the all-ones index among them."""
    out = []
    top = (1 << bw) - 1
    while len(out) < n:
        v = top if rng.integers(0, 4) == 0 else int(rng.integers(0, top + 1))
        out += [v] * int(rng.integers(1, 13))
    return out[:n]


@functools.lru_cache(maxsize=None)
def dict_cases():
    """[dict(name, bw, values, body)]: body = [u8 bw][hybrid runs]."""
    rng = np.random.default_rng(77)
    cases = []

    def add(name, bw, values, plan, pad_bits=0):
        body = bytes([bw]) + rle_hybrid(values, bw, plan, pad_bits)
        cases.append(dict(name=name, bw=bw, values=list(values), body=body,
                          plan=plan))

    plans = ["rle", "packed", "alternate"]
    for bw in range(33):
        for k in range(3):
            n = DICT_NVALS[(bw + 4 * k) % len(DICT_NVALS)]
            plan = plans[(bw + k) % 3]
            add(f"bw={bw} n={n} {plan}", bw, _runny(rng, bw, n), plan,
                pad_bits=0xFFFFFFFF)
    for bw in (1, 2, 15, 17, 31, 32):
        add(f"bw={bw} n=1000 one packed run >64 groups", bw,
            _runny(rng, bw, 1000), "packed")
        add(f"bw={bw} n=513 padded group, non-zero padding", bw,
            _runny(rng, bw, 513), "packed", pad_bits=0xFFFFFFFF)
    for n in DICT_NVALS:
        add(f"bw=32 max index n={n}", 32, [0xFFFFFFFF] * n,
            "packed" if n % 2 else "rle")
        add(f"bw=5 n={n} alternate, every count", 5, _runny(rng, 5, n), "alternate",
            pad_bits=0x15)
    add("bw=7 rle run of 1000 (2-byte header)", 7, [99] * 1000, "rle")
    add("bw=9 rle run longer than nvals", 9, [300] * 20, [("rle", 5000)])
    add("bw=9 packed 64 then rle past nvals", 9, _runny(rng, 9, 64) + [5] * 3,
        [("packed", 64), ("rle", 900)])
    add("bw=12 packed 16 then rle 1", 12, _runny(rng, 12, 16) + [7],
        [("packed", 16), ("rle", 1)])
    return cases


DEF_NVALS = [1, 31, 32, 33, 45, 100]
# consecutive pages of one column: neighbours share a validity word
DEF_BATCHES = [(45, 45, 38), (31, 2, 33), (33, 100, 32, 1)]


def _def_pattern(kind, n, rng):
    if kind == "valid":
        return [1] * n
    if kind == "null":
        return [0] * n
    if kind == "alternating":
        return [i & 1 for i in range(n)]
    if kind == "long runs":
        return ([1] * 17 + [0] * 23 + [1] * 40 + [0] * 9 + [1] * 64)[:n]
    return [int(b) for b in rng.integers(0, 2, n)]


@functools.lru_cache(maxsize=None)
def def_cases():
    """[dict(name, levels, plan, page)] for max_def == 1; the page is
    [u32 dlen][levels] with an empty body.  The DEF_BATCHES entries come
    first, in order, so cumulative bit offsets put them in shared words."""
    rng = np.random.default_rng(11)
    cases = []

    def add(name, levels, plan):
        cases.append(dict(name=name, levels=levels, plan=plan,
                          page=with_def_levels(rle_hybrid(levels, 1, plan),
                                               b"")))

    for batch in DEF_BATCHES:
        for k, n in enumerate(batch):
            add(f"shared word {batch}[{k}]", _def_pattern("random", n, rng),
                ["alternate", "packed", "rle"][k % 3])
    for kind in ("valid", "null", "alternating", "long runs", "random"):
        for n in DEF_NVALS:
            for plan in ("rle", "packed", "alternate"):
                add(f"{kind} n={n} {plan}", _def_pattern(kind, n, rng), plan)
    return cases


def def_bit_offsets():
    """bit_off of every def_cases() page when they are laid out back to
    back as the pages of one column (how the GPU test runs them)."""
    offs, at = [], 0
    for c in def_cases():
        offs.append(at)
        at += len(c["levels"])
    return offs, at


NULL_PATTERNS = ["leading", "trailing", "alternating", "all-null", "none"]


def null_pattern(kind, n):
    """Definition levels (1 = present) for n slots."""
    k = max(1, n // 3)
    if kind == "leading":
        return [0] * k + [1] * (n - k)
    if kind == "trailing":
        return [1] * (n - k) + [0] * k
    if kind == "alternating":
        return [(i + 1) & 1 for i in range(n)]
    if kind == "all-null":
        return [0] * n
    return [1] * n


FIXED_COUNTS = [1, 63, 64, 65, 257]


@functools.lru_cache(maxsize=None)
def flba_cases():
    """[dict(name, width, ints)]: width 1..16, extremes first."""
    rng = np.random.default_rng(5)
    cases = []
    for w in range(1, 17):
        n = FIXED_COUNTS[w % len(FIXED_COUNTS)]
        lo, hi = -(1 << (8 * w - 1)), (1 << (8 * w - 1)) - 1
        base = [lo, hi, -1, 0, 1]
        rnd = [int.from_bytes(rng.bytes(w), "big", signed=True)
               for _ in range(max(n, 6))]
        ints = (base + rnd)[:n] if n >= 5 else [lo][:n]
        cases.append(dict(name=f"flba width={w} n={len(ints)}", width=w,
                          ints=ints))
        if n < 5:  # the extremes still get their turn at this width
            cases.append(dict(name=f"flba width={w} n=6 extremes", width=w,
                              ints=base + rnd[:1]))
    return cases


@functools.lru_cache(maxsize=None)
def fixed_cases():
    """[dict(name, esz, raw)]: raw = n*esz little-endian value bytes, for
    PLAIN and BYTE_STREAM_SPLIT.  Float specials are raw bit patterns."""
    rng = np.random.default_rng(6)
    special = {
        4: [0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000,
            0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000],
        8: [0x7FF8000000000001, 0xFFF8DEADBEEF0001, 0x7FF0000000000001,
            0x0000000000000000, 0x8000000000000000, 0x0000000000000001,
            0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000],
    }
    cases = []
    for esz in (4, 8):
        for n in FIXED_COUNTS:
            pats = [special[esz][i % 9] if i < 9 or i % 7 == 0 else
                    int.from_bytes(rng.bytes(esz), "little")
                    for i in range(n)]
            raw = b"".join(p.to_bytes(esz, "little") for p in pats)
            cases.append(dict(name=f"esz={esz} n={n}", esz=esz, n=n, raw=raw))
    return cases


@functools.lru_cache(maxsize=None)
def ba_cases():
    """[dict(name, pages)]: a column = list of pages, a page = list of
    bytes or None (NULL slot).  Offsets continue across a column's pages;
    the DELTA_BYTE_ARRAY chain restarts at each page."""
    long_s = bytes(range(256)) + b"tail-" * 20
    cases = [
        ("single value", [[b"x"]]),
        ("single empty", [[b""]]),
        ("all empty", [[b""] * 9]),
        ("all equal lengths (width-0 miniblocks)",
         [[b"abcd", b"abce", b"abzz", b"qrst"] * 9]),
        ("whole-previous prefix, empty suffix",
         [[b"prefix", b"prefix", b"prefix", b"prefixed", b"prefixed"]]),
        ("prefix 0 after a long string",
         [[long_s, b"", b"zebra", long_s, long_s[:300], b"\x00"]]),
        ("non-ASCII", [["grüße".encode(), "grün".encode(), b"\xff\xfe\x00",
                        b"\xff\xfe\x00\x80", "日本語".encode(),
                        "日本".encode()]]),
        ("nulls between strings",
         [[None, b"apple", None, None, b"applesauce", b"apply", None,
           b"ap", None]]),
        ("all null", [[None] * 5]),
        ("two pages", [[b"alpha", b"alphabet", None, b"alpine"],
                       [b"alpaca", None, b"alp", b"", b"alps" * 70]]),
        ("133 strings, two blocks of lengths",
         [[(b"k%03d-" % (i // 3)) + b"v" * (i % 11) for i in range(133)]]),
    ]
    return [dict(name=n, pages=p) for n, p in cases]


@functools.lru_cache(maxsize=None)
def list_cases():
    """[dict(name, list_nullable, elem_nullable, pages=[rows...])]."""
    def rows(ln, en, seed, n):
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n):
            k = int(rng.integers(0, 6))
            if k == 0 and ln:
                out.append(None)
            elif k <= 1:
                out.append([])
            elif k == 2:
                out.append([int(rng.integers(0, 100))])
            else:
                out.append([None if en and rng.integers(0, 3) == 0
                            else int(rng.integers(0, 100))
                            for _ in range(int(rng.integers(2, 7)))])
        return out
    cases = []
    for ln, en in ((0, 0), (0, 1), (1, 0), (1, 1)):
        fixed = [[1, 2, 3], [], [4]]
        if ln:
            fixed = [None] + fixed + [None]
        if en:
            fixed += [[None], [5, None, None, 6], [None, None]]
        # the second page's row and entry bases are no multiples of 32
        first = fixed + rows(ln, en, 40 + 2 * ln + en, 37 - len(fixed))
        if sum(len(r or []) for r in first) % 32 == 0:
            first.append([7])
        cases.append(dict(
            name=f"list_nullable={ln} elem_nullable={en}",
            list_nullable=ln, elem_nullable=en,
            pages=[first, rows(ln, en, 50 + 2 * ln + en, 23)]))
    return cases


SLACK = 256  # zero bytes uploaded after every malformed page


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """[dict(name, entry, page, nvals, kw)]: each page has ONE named defect.
    entry: which bg_*_batch call takes it; kw: has_def / esz / enc / src_esz.
    Any corrupt length stays within SLACK bytes past the page."""
    good_vals = [100 + i * i for i in range(40)]  # widths 6 and 7
    good_dbp = dbp(good_vals)
    lv_all = rle_hybrid([1] * 40, 1, "rle")
    eleven = b"\x80" * 11 + b"\x01"
    out = []

    def add(name, entry, page, nvals, **kw):
        out.append(dict(name=name, entry=entry, page=bytes(page), nvals=nvals,
                        kw=kw))

    # ---- DELTA_BINARY_PACKED ----
    add("dbp: truncated in the header", "delta_bp", good_dbp[:2], 40, esz=8)
    add("dbp: truncated after the header", "delta_bp", good_dbp[:6], 40,
        esz=8)
    add("dbp: truncated in the width bytes", "delta_bp", good_dbp[:8], 40,
        esz=8)
    add("dbp: truncated in a miniblock", "delta_bp", good_dbp[:-1], 40, esz=8)
    add("dbp: has_def page shorter than 4", "delta_bp", b"\x02\x00", 40,
        esz=8, has_def=1)
    add("dbp: dlen past page_len", "delta_bp",
        struct.pack("<I", len(lv_all) + len(good_dbp) + 5) + lv_all + good_dbp,
        40, esz=8, has_def=1)
    w65 = bytearray(dbp(good_vals, width=7))
    hdr = len(uvarint(128) + uvarint(4) + uvarint(40) + uvarint(zigzag(100))
              + uvarint(zigzag(1)))
    assert w65[hdr] == 7
    w65[hdr] = 65
    add("dbp: width byte 65", "delta_bp", w65, 40, esz=8)
    add("dbp: miniblocks = 0", "delta_bp",
        uvarint(128) + uvarint(0) + good_dbp[3:], 40, esz=8)
    add("dbp: block size not divisible by miniblocks", "delta_bp",
        uvarint(128) + uvarint(3) + good_dbp[3:], 40, esz=8)
    add("dbp: miniblocks of 4 values", "delta_bp",
        uvarint(16) + good_dbp[2:], 40, esz=8)
    add("dbp: total smaller than nvals", "delta_bp", dbp(good_vals, total=39),
        40, esz=8)
    add("dbp: varint of 11 continuation bytes", "delta_bp",
        eleven + good_dbp[2:], 40, esz=8)
    add("dbp: min_delta varint of 11 continuation bytes", "delta_bp",
        good_dbp[:6] + eleven + good_dbp[7:], 40, esz=8)
    # ---- dictionary indices ----
    idx = _runny(np.random.default_rng(3), 6, 40)
    good_dict = bytes([6]) + rle_hybrid(idx, 6, "packed")
    add("dict: empty page", "dict", b"", 40)
    add("dict: bit width 33", "dict", bytes([33]) + good_dict[1:], 40)
    add("dict: truncated after the width byte", "dict", good_dict[:1], 40)
    add("dict: truncated final bit-packed group", "dict", good_dict[:-1], 40)
    add("dict: bit-packed byte count past the page", "dict",
        bytes([6]) + uvarint((30 << 1) | 1) + good_dict[2:], 40)
    add("dict: rle value cut off", "dict",
        bytes([20]) + uvarint(40 << 1) + b"\x01\x02", 40)
    add("dict: run header of 11 continuation bytes", "dict",
        bytes([6]) + eleven + good_dict[2:], 40)
    add("dict: runs end before nvals", "dict",
        bytes([6]) + rle_hybrid(idx[:16], 6, "packed"), 40)
    add("dict: has_def page shorter than 4", "dict", b"\x01", 40, has_def=1)
    add("dict: dlen past page_len", "dict",
        struct.pack("<I", len(lv_all) + len(good_dict) + 3) + lv_all
        + good_dict, 40, has_def=1)
    add("dict: level header of 11 continuation bytes", "dict",
        with_def_levels(eleven, good_dict), 40, has_def=1)
    # ---- definition levels ----
    add("def: page shorter than 4", "def", b"\x01\x00\x00", 40)
    add("def: dlen past page_len", "def",
        struct.pack("<I", len(lv_all) + 7) + lv_all, 40)
    add("def: levels end before nvals", "def",
        with_def_levels(rle_hybrid([1] * 30, 1, "rle"), b""), 40)
    add("def: truncated bit-packed run", "def",
        with_def_levels(rle_hybrid([1, 0] * 20, 1, "packed")[:-2], b""), 40)
    add("def: rle value missing", "def", with_def_levels(uvarint(80), b""),
        40)
    add("def: header of 11 continuation bytes", "def",
        with_def_levels(eleven, b""), 40)
    # ---- list levels ----
    rep, deff = [0, 1, 1, 0, 0, 1], [2, 2, 2, 1, 2, 2]
    good_list = list_page(rep, deff, 2, b"")
    add("list: page shorter than 8", "list", good_list[:7], 6, max_def=2)
    add("list: rlen past page_len", "list",
        struct.pack("<I", len(good_list) + 9) + good_list[4:], 6, max_def=2)
    r = rle_hybrid(rep, 1, "packed")
    d = rle_hybrid(deff, 2, "packed")
    add("list: dlen past page_len", "list",
        struct.pack("<I", len(r)) + r + struct.pack("<I", len(d) + 6) + d, 6,
        max_def=2)
    add("list: def levels truncated", "list",
        struct.pack("<I", len(r)) + r + struct.pack("<I", len(d) - 1)
        + d[:-1], 6, max_def=2)
    add("list: rep header of 11 continuation bytes", "list",
        struct.pack("<I", 12) + eleven + struct.pack("<I", len(d)) + d, 6,
        max_def=2)
    add("list: def level above max_def", "list",
        list_page(rep, [3] + deff[1:], 3, b""), 6, max_def=2)
    # ---- PLAIN fixed width / BYTE_STREAM_SPLIT ----
    vals8 = plain_fixed(np.arange(40, dtype=np.int64))
    add("plain: value bytes truncated", "extract", vals8[:-1], 40, src_esz=8)
    add("plain: has_def page shorter than 4", "extract", b"\x00\x00", 40,
        src_esz=8, has_def=1)
    add("plain: dlen past page_len", "extract",
        struct.pack("<I", len(lv_all) + len(vals8) + 8) + lv_all + vals8, 40,
        src_esz=8, has_def=1)
    add("plain: level header of 11 continuation bytes", "extract",
        with_def_levels(eleven, vals8), 40, src_esz=8, has_def=1)
    add("plain: values truncated after levels", "extract",
        with_def_levels(lv_all, vals8[:-8]), 40, src_esz=8, has_def=1)
    add("bss: value bytes truncated", "bss", vals8[:-1], 40, src_esz=8)
    add("bss: dlen past page_len", "bss",
        struct.pack("<I", len(lv_all) + len(vals8) + 8) + lv_all + vals8, 40,
        src_esz=8, has_def=1)
    # ---- BYTE_ARRAY ----
    strs = [b"alpha", b"alphabet", b"alpine", b"beta"]
    pba = plain_byte_array(strs)
    add("ba: truncated in a length word", "ba", pba[:11], 4)
    add("ba: truncated in the bytes", "ba", pba[:-1], 4)
    add("ba: length past page_len", "ba",
        pba[:9] + struct.pack("<I", 40) + pba[13:], 4)
    add("ba: dlen past page_len", "ba",
        struct.pack("<I", len(pba) + 10) + pba, 4, has_def=1)
    d6 = delta_length_byte_array(strs)
    add("enc6: truncated in the lengths", "delta_ba", d6[:4], 4, enc=6)
    add("enc6: truncated in the bytes", "delta_ba", d6[:-1], 4, enc=6)
    add("enc6: total smaller than nvals", "delta_ba",
        dbp([len(s) for s in strs], total=3) + b"".join(strs), 4, enc=6)
    add("enc6: negative length", "delta_ba",
        dbp([5, -3, 6, 4]) + b"".join(strs), 4, enc=6)
    d7 = delta_byte_array(strs)
    add("enc7: non-zero first prefix", "delta_ba",
        delta_byte_array(strs, prefix_lens=[2, 5, 3, 0]), 4, enc=7)
    add("enc7: prefix longer than the previous string", "delta_ba",
        delta_byte_array(strs, prefix_lens=[0, 5, 9, 0]), 4, enc=7)
    add("enc7: truncated in the prefix lengths", "delta_ba", d7[:3], 4, enc=7)
    add("enc7: truncated between the two length streams", "delta_ba",
        d7[:len(dbp([0, 5, 3, 0]))], 4, enc=7)
    add("enc7: truncated in the suffix bytes", "delta_ba", d7[:-1], 4, enc=7)
    add("enc7: suffix width byte 65", "delta_ba",
        _poke(d7, len(dbp([0, 5, 3, 0])) + 6, 65, was=2), 4, enc=7)
    return out


def _poke(buf, at, byte, was):
    b = bytearray(buf)
    assert b[at] == was
    b[at] = byte
    return bytes(b)
