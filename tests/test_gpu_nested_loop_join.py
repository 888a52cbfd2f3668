"""Nested-loop joins (DataFusion NestedLoopJoinExec: no equi-key, the
residual filter alone decides): bg_nljoin_* at the C ABI and the
nested_loop_join node through bg_execute_stage, on all eight join types.
Every comparison is exact, against a plain-Python double loop: every (build
row, probe row) pair is a candidate, it passes when the filter is TRUE (NULL
counts as FALSE, no filter passes everything), and each join type reads
"match" as "passing candidate".  Pairs come in ascending probe row and,
within one, ascending build row."""
import contextlib
import ctypes
import decimal
import gc
from collections import Counter, defaultdict

import numpy as np
import pyarrow as pa
import pytest

from datafusion_ballista_amd import gpu, stage
from join_filter_helpers import (
    ANTI, ANTI_BUILD, BG_ERR_INVALID, BG_OK, CMP_CODE, I64, INNER, NULL_IDX,
    OPS, OUTER_BUILD, OUTER_FULL, OUTER_PROBE, SEMI, SEMI_BUILD, SENTINEL,
    bits, scan_of, term, terms_array)

pytestmark = pytest.mark.gpu

D = decimal.Decimal
CTX = decimal.Context(prec=60)


@pytest.fixture(scope="module")
def ctx():
    c = gpu.GpuStageContext(0)
    yield c
    c.close()


@pytest.fixture()
def reg(ctx):
    keep, names = [], []

    def _reg(name, table):
        keep.append(stage.register_table(ctx, name, table))
        names.append(name)
        return table

    yield _reg
    for n in names:
        stage.unregister_table(n)


# ---------------------------------------------------------------------------
# ABI level: data, reference, device side
# ---------------------------------------------------------------------------
class Case:
    """Both sides carry x over {0..3} with ~10 % NULLs; the build side also a
    band [lo, hi) with lo in {0..3}, hi = lo + {0..2} and ~10 % NULL lo; two
    random masks per side."""

    def __init__(self, n_build, n_probe, seed):
        rng = np.random.default_rng(seed)
        self.nb, self.np_ = n_build, n_probe
        lo = rng.integers(0, 4, size=n_build, dtype=np.int64)
        self.b = {"x": (rng.integers(0, 4, size=n_build, dtype=np.int64),
                        rng.random(n_build) >= 0.1),
                  "lo": (lo, rng.random(n_build) >= 0.1),
                  "hi": (lo + rng.integers(0, 3, size=n_build, dtype=np.int64),
                         np.ones(n_build, dtype=bool))}
        self.px = rng.integers(0, 4, size=n_probe, dtype=np.int64)
        self.pxv = rng.random(n_probe) >= 0.1
        self.bm = [rng.random(n_build) < 0.6 for _ in range(2)]
        self.pm = [rng.random(n_probe) < 0.6 for _ in range(2)]


# a filter: list of groups {"bm": mask index, "pm": mask index, "cross":
# [(build column, cmp, encoding)]}; every cross term compares against the
# probe side's x
SHAPES = {
    "none": [],
    "dec_gt": [{"cross": [("x", "gt", "dec")]}],
    "band": [{"cross": [("lo", "le", "i64"), ("hi", "gt", "i64")]}],
    "two_groups": [{"bm": 0, "pm": 0, "cross": [("x", "lt", "i64")]},
                   {"bm": 1, "pm": 1, "cross": [("x", "eq", "dec")]}],
    "masks_only": [{"bm": 0, "pm": 1}],
}


def passes_fn(case, shape):
    if not shape:
        return lambda b, p: True

    def passes(b, p):
        for g in shape:
            if "bm" in g and not case.bm[g["bm"]][b]:
                continue
            if "pm" in g and not case.pm[g["pm"]][p]:
                continue
            if all(case.b[c][1][b] and case.pxv[p] and
                   OPS[cmp](int(case.b[c][0][b]), int(case.px[p]))
                   for c, cmp, _ in g.get("cross", [])):
                return True
        return False
    return passes


def reference(case, passes, lo=0, hi=None):
    """The double loop over probe rows [lo, hi); probe indices relative to
    lo.  -> pair lists in the stated order, and the marked build rows."""
    hi = case.np_ if hi is None else hi
    r = {"inner": [], "semi": [], "anti": [], "left": [], "marked": set()}
    for p in range(lo, hi):
        ok = [b for b in range(case.nb) if passes(b, p)]
        q = p - lo
        r["marked"].update(ok)
        r["inner"] += [(q, b) for b in ok]
        r["left"] += [(q, b) for b in ok] or [(q, NULL_IDX)]
        if ok:
            r["semi"].append((q, ok[0]))        # the lowest passing build row
        else:
            r["anti"].append((q, NULL_IDX))
    return r


# cross-column encodings: monotone maps of the small domain, negative values
# included; the Decimal128 ones are wider than 64 bits
def enc_i64(v):
    return (v - 2) * 10**12


def enc_dec(v):
    out = bytearray()
    for x in v:
        out += ((int(x) - 2) * (2**70 + 12345)).to_bytes(16, "little",
                                                         signed=True)
    return np.frombuffer(bytes(out), dtype=np.uint8)


ENC = {"i64": (gpu.BG_DT_INT64, enc_i64), "dec": (gpu.BG_DT_DECIMAL128, enc_dec)}


def up(ctx, arr):
    """Upload with a tail, so an empty side still has a buffer."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    return ctx.upload(np.concatenate([raw, np.zeros(16, dtype=np.uint8)]))


class Dev:
    """The case's build side on the device, and probe slices on demand."""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        self.b = {(c, e): up(ctx, ENC[e][1](case.b[c][0]))
                  for c, e in (("x", "i64"), ("x", "dec"), ("lo", "i64"),
                               ("hi", "i64"))}
        self.bv = {c: up(ctx, bits(case.b[c][1])) for c in case.b}
        self.bm = [up(ctx, bits(m)) for m in case.bm]

    def probe(self, shape, lo=0, hi=None):
        """-> (terms array, nterms, keep-alive) for probe rows [lo, hi)."""
        c, ctx = self.case, self.ctx
        hi = c.np_ if hi is None else hi
        px = {e: up(ctx, ENC[e][1](c.px[lo:hi])) for e in ENC}
        pxv = up(ctx, bits(c.pxv[lo:hi]))
        pm = [up(ctx, bits(m[lo:hi])) for m in c.pm]
        terms = []
        for gi, g in enumerate(shape):
            if "bm" in g:
                terms.append(term(gpu.BG_JF_BUILD_MASK, gi, b=self.bm[g["bm"]]))
            if "pm" in g:
                terms.append(term(gpu.BG_JF_PROBE_MASK, gi, p=pm[g["pm"]]))
            for col, cmp, e in g.get("cross", []):
                terms.append(term(gpu.BG_JF_CROSS, gi, ENC[e][0],
                                  CMP_CODE[cmp], self.b[(col, e)],
                                  self.bv[col], px[e], pxv))
        return terms_array(terms), len(terms), (px, pxv, pm)


class Join:
    """One bg_nljoin_open handle."""

    def __init__(self, ctx, n_build):
        self.ctx, self.n_build = ctx, n_build
        self.h = ctypes.c_void_p()
        assert ctx.L.bg_nljoin_open(n_build, ctypes.byref(self.h)) == BG_OK
        assert self.h.value

    # the handle's five entries after open; HashJoin swaps in the general
    # hash join's
    def _count(self, n, jt, terms, nterms, m):
        return self.ctx.L.bg_nljoin_count(self.h, n, jt, terms, nterms, m)

    def _fill(self, n, jt, terms, nterms, op, ob):
        return self.ctx.L.bg_nljoin_fill(self.h, n, jt, terms, nterms, op, ob)

    def _mark(self, n, terms, nterms):
        return self.ctx.L.bg_nljoin_mark(self.h, n, terms, nterms)

    def _build_rows(self, matched, cnt, out):
        return self.ctx.L.bg_nljoin_build_rows(self.h, matched, cnt, out)

    def _free(self):
        return self.ctx.L.bg_nljoin_free(self.h)

    def mark(self, n, terms, nterms):
        assert self._mark(n, terms, nterms) == BG_OK

    def rows(self, matched):
        out = self.ctx.alloc(4 * self.n_build + 4)
        cnt = I64(-1)
        assert self._build_rows(matched, ctypes.byref(cnt), out.ptr) == BG_OK
        return out.download(np.uint32, cnt.value).astype(np.int64).tolist()

    def pairs(self, n, jt, terms, nterms):
        """Count, then fill into buffers pre-filled with a sentinel: nothing
        may be written past the reported count.  -> list of (probe, build)
        in the order written."""
        m, pad = I64(-1), 8
        assert self._count(n, jt, terms, nterms, ctypes.byref(m)) == BG_OK
        m = m.value
        bufs = []
        for _ in range(2):
            b = self.ctx.alloc(4 * (m + pad))
            b.upload(np.full(m + pad, SENTINEL, dtype=np.uint32))
            bufs.append(b)
        assert self._fill(n, jt, terms, nterms, bufs[0].ptr,
                          bufs[1].ptr) == BG_OK
        got = [b.download(np.uint32, m + pad) for b in bufs]
        for g in got:
            assert np.all(g[m:] == SENTINEL)
        return list(zip(got[0][:m].tolist(), got[1][:m].tolist()))

    def free(self):
        assert self._free() == BG_OK
        self.h = ctypes.c_void_p()


def check_all_types(ctx, dev, shape, want):
    """All eight types of one filter against the reference `want`; pair
    arrays element for element."""
    case = dev.case
    terms, nt, _keep = dev.probe(shape)
    n, nb = case.np_, case.nb
    marked = sorted(want["marked"])
    unmarked = sorted(set(range(nb)) - want["marked"])
    j = Join(ctx, nb)
    try:
        assert j.pairs(n, INNER, terms, nt) == want["inner"]
        assert j.pairs(n, SEMI, terms, nt) == want["semi"]
        assert j.pairs(n, ANTI, terms, nt) == want["anti"]
        assert j.pairs(n, OUTER_PROBE, terms, nt) == want["left"]
        assert j.rows(1) == []                          # nothing marked yet
        assert j.rows(0) == list(range(nb))
        assert j.pairs(n, OUTER_BUILD, terms, nt) == want["inner"]
        assert j.rows(1) == marked
        assert j.rows(0) == unmarked
    finally:
        j.free()
    j = Join(ctx, nb)
    try:
        assert j.pairs(n, OUTER_FULL, terms, nt) == want["left"]
        assert j.rows(1) == marked
        assert j.rows(0) == unmarked
    finally:
        j.free()
    # semi_build / anti_build: mark, then list the build rows
    j = Join(ctx, nb)
    try:
        j.mark(n, terms, nt)
        assert j.rows(1) == marked
        assert j.rows(0) == unmarked
    finally:
        j.free()


# 64 is the bitmap-word and wave edge; 4 * n_build + 50 leaves a ragged tail
N_BUILD = [0, 1, 63, 64, 65, 200]
GRID = [(nb, np_) for nb in N_BUILD for np_ in (0, 1, 64, 4 * nb + 50)]
_CASES = {}


def case_of(n_build, n_probe):
    key = (n_build, n_probe)
    if key not in _CASES:
        _CASES[key] = Case(n_build, n_probe, seed=1000 * n_build + n_probe)
    return _CASES[key]


@pytest.mark.parametrize("n_build,n_probe", GRID)
def test_all_types_at_the_abi(ctx, n_build, n_probe):
    case = case_of(n_build, n_probe)
    dev = Dev(ctx, case)
    wants = {}
    for name, shape in SHAPES.items():
        wants[name] = reference(case, passes_fn(case, shape))
        check_all_types(ctx, dev, shape, wants[name])
    if (n_build, n_probe) == (200, 850):
        # on the reference alone: the filters differ from one another and
        # from the cross join, and each leaves rows matched and unmatched
        # on both sides
        inner = [tuple(w["inner"]) for w in wants.values()]
        assert len(set(inner)) == len(SHAPES)
        assert len(wants["none"]["inner"]) == 200 * 850
        for name, w in wants.items():
            if name != "none":
                assert w["semi"] and w["anti"], name
                assert 0 < len(w["marked"]) < 200, name


def test_chunks_accumulate_one_bitmap(ctx):
    """Two probe slices that split at row 128 leave the visited bits one
    call over all rows leaves, by mark and by an OUTER_BUILD fill, and the
    bitmap is allocated by the first marking call only."""
    case = case_of(200, 850)
    dev = Dev(ctx, case)
    shape = SHAPES["two_groups"]
    passes = passes_fn(case, shape)
    whole = reference(case, passes)
    slices = [(0, 128), (128, case.np_)]
    for use_fill in (False, True):
        j = Join(ctx, case.nb)
        try:
            seen = set()
            for k, (lo, hi) in enumerate(slices):
                terms, nt, keep = dev.probe(shape, lo, hi)
                want = reference(case, passes, lo, hi)
                gc.collect()
                before = ctx.pool_stats()[1]
                if use_fill:
                    assert j.pairs(hi - lo, OUTER_BUILD, terms, nt) == \
                        want["inner"]
                    gc.collect()
                    # the handle keeps its offsets (first slice) and its
                    # bitmap (first slice), nothing else
                    assert ctx.pool_stats()[1] == before + (2 if k == 0 else 0)
                else:
                    j.mark(hi - lo, terms, nt)
                    assert ctx.pool_stats()[1] == before + (1 if k == 0 else 0)
                seen |= want["marked"]
                assert j.rows(1) == sorted(seen)
                del terms, keep
            assert seen == whole["marked"] and 0 < len(seen) < case.nb
            one = Join(ctx, case.nb)
            try:
                terms, nt, _keep = dev.probe(shape)
                one.mark(case.np_, terms, nt)
                assert one.rows(1) == j.rows(1)
                assert one.rows(0) == j.rows(0)
            finally:
                one.free()
        finally:
            j.free()


def test_open_and_free_with_an_empty_build_side(ctx):
    L = ctx.L
    gc.collect()
    base = ctx.pool_stats()[:2]
    j = Join(ctx, 0)
    assert j.rows(0) == [] and j.rows(1) == []
    j.free()
    assert L.bg_nljoin_free(None) == BG_OK
    gc.collect()
    assert ctx.pool_stats()[:2] == base


def test_refusals_and_pool_balance(ctx):
    case = case_of(65, 310)
    dev = Dev(ctx, case)
    terms, nt, _keep = dev.probe(SHAPES["dec_gt"])
    other, nt2, _keep2 = dev.probe(SHAPES["band"])
    out = ctx.alloc(4 * 65 * 310)
    L, n, m = ctx.L, case.np_, I64()
    h = ctypes.c_void_p()
    gc.collect()
    base = ctx.pool_stats()[:2]

    def refused(rc, needle=None):
        assert rc == BG_ERR_INVALID
        if needle:
            assert needle in L.bg_last_error(), L.bg_last_error()

    # open: negative and too large a build side (u32 indices, NULL_IDX taken)
    refused(L.bg_nljoin_open(-1, ctypes.byref(h)), b"negative")
    refused(L.bg_nljoin_open(2**32 - 1, ctypes.byref(h)), b"2^32 - 1")
    refused(L.bg_nljoin_open(2**40, ctypes.byref(h)), b"2^32 - 1")
    assert not h.value
    # a NULL handle, everywhere but free
    refused(L.bg_nljoin_count(None, n, INNER, terms, nt, ctypes.byref(m)),
            b"null")
    refused(L.bg_nljoin_fill(None, n, INNER, terms, nt, out.ptr, out.ptr),
            b"null")
    refused(L.bg_nljoin_mark(None, n, terms, nt), b"null")
    refused(L.bg_nljoin_build_rows(None, 1, ctypes.byref(m), out.ptr),
            b"null")
    assert L.bg_nljoin_free(None) == BG_OK

    j = Join(ctx, case.nb)
    # negative probe row counts
    refused(L.bg_nljoin_count(j.h, -1, INNER, terms, nt, ctypes.byref(m)),
            b"negative")
    refused(L.bg_nljoin_fill(j.h, -1, INNER, terms, nt, out.ptr, out.ptr),
            b"negative")
    refused(L.bg_nljoin_mark(j.h, -1, terms, nt), b"negative")
    # join types outside 0..7; 4 and 5 have no pairs
    for jt in (-1, 8, 100):
        refused(L.bg_nljoin_count(j.h, n, jt, terms, nt, ctypes.byref(m)),
                b"join_type")
        refused(L.bg_nljoin_fill(j.h, n, jt, terms, nt, out.ptr, out.ptr),
                b"join_type")
    for jt in (SEMI_BUILD, ANTI_BUILD):
        refused(L.bg_nljoin_count(j.h, n, jt, terms, nt, ctypes.byref(m)),
                b"bg_nljoin_mark")
        refused(L.bg_nljoin_fill(j.h, n, jt, terms, nt, out.ptr, out.ptr),
                b"bg_nljoin_mark")
    # terms go through the hash joins' checks: same limits, same messages
    five = terms_array([terms[0]] * 5)
    refused(L.bg_nljoin_count(j.h, n, INNER, five, 5, ctypes.byref(m)),
            b"more than 4 cross terms")
    bad_group = terms_array([term(gpu.BG_JF_CROSS, 4, gpu.BG_DT_INT64, 0,
                                  dev.b[("x", "i64")], None,
                                  dev.b[("x", "i64")])])
    refused(L.bg_nljoin_mark(j.h, n, bad_group, 1), b"group id")
    f64 = terms_array([term(gpu.BG_JF_CROSS, 0, gpu.BG_DT_FLOAT64, 0,
                            dev.b[("x", "i64")], None, dev.b[("x", "i64")])])
    assert L.bg_nljoin_count(j.h, n, INNER, f64, 1, ctypes.byref(m)) < 0
    assert b"Float64" in L.bg_last_error()
    refused(L.bg_nljoin_count(j.h, n, INNER, None, 1, ctypes.byref(m)))
    # a fill before any count, then fills that do not repeat the count
    refused(L.bg_nljoin_fill(j.h, n, INNER, terms, nt, out.ptr, out.ptr),
            b"bg_nljoin_count")
    assert L.bg_nljoin_count(j.h, n, INNER, terms, nt,
                             ctypes.byref(m)) == BG_OK
    assert 0 < m.value < 65 * 310
    refused(L.bg_nljoin_fill(j.h, n - 1, INNER, terms, nt, out.ptr, out.ptr),
            b"bg_nljoin_count")
    refused(L.bg_nljoin_fill(j.h, n, OUTER_PROBE, terms, nt, out.ptr,
                             out.ptr), b"bg_nljoin_count")
    refused(L.bg_nljoin_fill(j.h, n, INNER, other, nt2, out.ptr, out.ptr),
            b"bg_nljoin_count")
    refused(L.bg_nljoin_fill(j.h, n, INNER, None, 0, out.ptr, out.ptr),
            b"bg_nljoin_count")
    assert L.bg_nljoin_fill(j.h, n, INNER, terms, nt, out.ptr,
                            out.ptr) == BG_OK
    # nothing above marked anything
    assert j.rows(1) == []
    refused(L.bg_nljoin_build_rows(j.h, 2, ctypes.byref(m), out.ptr),
            b"matched")
    j.free()
    gc.collect()
    assert ctx.pool_stats()[:2] == base


# ---------------------------------------------------------------------------
# the two handles against each other
# ---------------------------------------------------------------------------
class HashJoin(Join):
    """One bg_hashjoin_build2 handle over a constant Int64 key, through the
    _filtered entries: every key is equal, so every build row is a candidate
    of every probe row, as in the nested loop.  bkey / pkey: key_column()."""

    def __init__(self, ctx, n_build, bkey, pkey):
        self.ctx, self.n_build = ctx, n_build
        self.bkey, self.pkey = bkey[0], pkey[0]
        self.h = ctypes.c_void_p()
        assert ctx.L.bg_hashjoin_build2(self.bkey, 1, n_build,
                                        ctypes.byref(self.h)) == BG_OK
        assert self.h.value

    def _count(self, n, jt, terms, nterms, m):
        return self.ctx.L.bg_hashjoin_probe_count2_filtered(
            self.h, self.pkey, 1, n, jt, terms, nterms, m)

    def _fill(self, n, jt, terms, nterms, op, ob):
        return self.ctx.L.bg_hashjoin_probe_fill2_filtered(
            self.h, self.pkey, 1, n, jt, terms, nterms, op, ob)

    def _mark(self, n, terms, nterms):
        return self.ctx.L.bg_hashjoin_probe_mark2_filtered(
            self.h, self.pkey, 1, n, terms, nterms)

    def _build_rows(self, matched, cnt, out):
        return self.ctx.L.bg_hashjoin_build_rows2(self.h, matched, cnt, out)

    def _free(self):
        return self.ctx.L.bg_hashjoin_free2(self.h)


def key_column(ctx, n):
    """-> (one all-zero Int64 key column of n rows, its buffer)."""
    buf = up(ctx, np.zeros(n, dtype=np.int64))
    return (gpu.BgColumn * 1)(ctx.column(gpu.BG_DT_INT64, buf, n)), buf


@contextlib.contextmanager
def both_handles(ctx, n_build, bkey, pkey):
    """-> (nested-loop handle, hash handle), both freed on every path."""
    nl = Join(ctx, n_build)
    try:
        hj = HashJoin(ctx, n_build, bkey, pkey)
        try:
            yield nl, hj
        finally:
            hj.free()
    finally:
        nl.free()


def by_probe_row(pairs):
    """Probe-major pairs -> {probe row: its build rows, sorted}."""
    rows = [p for p, _ in pairs]
    assert rows == sorted(rows)
    out = defaultdict(list)
    for p, b in pairs:
        out[p].append(b)
    return {p: sorted(bs) for p, bs in out.items()}


# a lone lane, a full wave, a wave plus one, a block (BG_BLOCK in kernels.hip,
# 256) plus one: where a whole-block loop and its active flag can go wrong
WALK_N_PROBE = [0, 1, 64, 65, 256 + 1]
PAIR_TYPES = [INNER, SEMI, ANTI, OUTER_PROBE, OUTER_BUILD, OUTER_FULL]


@pytest.mark.parametrize("n_build", [0, 1, 63, 64, 65])
def test_both_handles_agree(ctx, n_build):
    """The general hash join on a constant key and the nested-loop join run
    the same probe kernels over two walks: under one filter (build mask,
    probe mask, Int64 `lt` with NULLs on both sides) they must report the
    same totals, the same build rows per probe row and the same visited
    bits, for every pair type and for mark alone.  Within a probe row the
    orders differ (chain order against ascending), so rows are compared
    sorted.  SEMI is the one type where the two may differ by design: each
    emits the FIRST passing build row of its own order, so there the probe
    rows must agree, the nested loop's build row must be the lowest passing
    one and the hash join's some passing one."""
    b = np.arange(n_build)
    bx, bxv, bm = (b * 7) % 11, b % 5 != 3, b % 4 != 1
    dbx, dbxv, dbm = up(ctx, bx), up(ctx, bits(bxv)), up(ctx, bits(bm))
    bkey = key_column(ctx, n_build)
    probes = {}
    for n in WALK_N_PROBE:
        p = np.arange(n)
        px, pxv, pm = (p * 5 + 3) % 13, p % 7 != 5, p % 3 != 2
        if n == 65:
            # the second wave has exactly one live lane
            assert pm[64] and pxv[64] and pm[64:].sum() == 1
        bufs = up(ctx, px), up(ctx, bits(pxv)), up(ctx, bits(pm))
        terms = [term(gpu.BG_JF_BUILD_MASK, 0, b=dbm),
                 term(gpu.BG_JF_PROBE_MASK, 0, p=bufs[2]),
                 term(gpu.BG_JF_CROSS, 0, gpu.BG_DT_INT64, CMP_CODE["lt"],
                      dbx, dbxv, bufs[0], bufs[1])]
        passes = ((bm & bxv)[:, None] & (pm & pxv)[None, :] &
                  (bx[:, None] < px[None, :]))
        probes[n] = (terms_array(terms), len(terms), key_column(ctx, n),
                     passes, bufs)
    gc.collect()
    base = ctx.pool_stats()[:2]

    for n, (terms, nt, pkey, passes, _keep) in probes.items():
        ok = {p: np.flatnonzero(passes[:, p]).tolist() for p in range(n)}
        marked = np.flatnonzero(passes.any(axis=1)).tolist()
        for jt in PAIR_TYPES:
            with both_handles(ctx, n_build, bkey, pkey) as (nl, hj):
                got_nl = nl.pairs(n, jt, terms, nt)
                got_hj = hj.pairs(n, jt, terms, nt)
                assert len(got_nl) == len(got_hj), (n, jt)
                rows_nl, rows_hj = by_probe_row(got_nl), by_probe_row(got_hj)
                if jt == SEMI:
                    assert list(rows_nl) == list(rows_hj)
                    for p in rows_nl:
                        assert rows_nl[p] == ok[p][:1]
                        assert len(rows_hj[p]) == 1 and rows_hj[p][0] in ok[p]
                else:
                    assert rows_nl == rows_hj, (n, jt)
                if jt == INNER:     # and both are the filter's pairs
                    assert got_nl == [(p, b) for p in range(n) for b in ok[p]]
                fill_marks = jt in (OUTER_BUILD, OUTER_FULL)
                assert nl.rows(1) == hj.rows(1) == \
                    (marked if fill_marks else [])
                nl.mark(n, terms, nt)
                hj.mark(n, terms, nt)
                assert nl.rows(1) == hj.rows(1) == marked
                assert nl.rows(0) == hj.rows(0) == \
                    sorted(set(range(n_build)) - set(marked))
        # SEMI_BUILD / ANTI_BUILD: mark alone, then list the build rows
        with both_handles(ctx, n_build, bkey, pkey) as (nl, hj):
            nl.mark(n, terms, nt)
            hj.mark(n, terms, nt)
            assert nl.rows(1) == hj.rows(1) == marked
            assert nl.rows(0) == hj.rows(0)
    if n_build == 65:
        # on the reference alone: at the largest size the filter leaves rows
        # matched and unmatched on both sides
        passes = probes[257][3]
        assert 0 < passes.any(axis=1).sum() < 65
        assert 0 < passes.any(axis=0).sum() < 257
    gc.collect()
    assert ctx.pool_stats()[:2] == base


# ---------------------------------------------------------------------------
# stage level
# ---------------------------------------------------------------------------
def _doc(plan):
    return {"job_id": "job-nlj", "stage_id": 1, "task_id": 0,
            "work_dir": "/tmp/stage-tests", "plan": plan}


def run(plan):
    return [tuple(r) for r in stage.execute(_doc(plan))["rows"]]


def dec_array(unscaled, p, s, mask=None):
    vals = [None if mask is not None and mask[i]
            else D(int(v)).scaleb(-s, context=CTX)
            for i, v in enumerate(unscaled)]
    return pa.array(vals, type=pa.decimal128(p, s))


def cast(arg, dtype, p=None, s=None):
    to = {"dtype": dtype}
    if p is not None:
        to.update(precision=p, scale=s)
    return {"cast": {"arg": arg, "to": to}}


def cross_filter(*terms):
    return {"any": [{"cross": [{"build": b, "cmp": c, "probe": p}
                               for b, c, p in terms]}]}


def round_half_away(num, den):
    """round-half-away-from-zero(num / den) over integers, den > 0."""
    q, r = divmod(abs(num), den)
    q += 2 * r >= den
    return q if num >= 0 else -q


Q22_CODES = ["13", "31", "23", "29", "30", "18", "17"]


def q22_plan(cust, orders, subquery_floor):
    """approved/q22.txt stage 3 over device tables: the customers of the
    seven country codes without an order, NestedLoopJoin'ed to the average
    positive balance of all customers of those codes."""
    code = {"substr": {"arg": {"col": "c_phone"}, "start": 1, "count": 2}}
    in_codes = {"expr": code, "in": Q22_CODES}
    avg = {"op": "hash_aggregate", "mode": "single", "group_by": [],
           "aggs": [{"fn": "avg", "as": "avg_bal",
                     "expr": {"col": "c_acctbal"}}],
           "input": {"op": "filter", "input": scan_of(cust, "nlj_cust"),
                     "predicates": [{"col": "c_acctbal", "cmp": "gt",
                                     "lo": subquery_floor}, in_codes]}}
    no_orders = {
        "op": "hash_join", "join_type": "anti_build",
        "build": {"op": "filter", "input": scan_of(cust, "nlj_cust"),
                  "predicates": [in_codes]},
        "probe": scan_of(orders, "nlj_orders"),
        "build_keys": ["c_custkey"], "probe_keys": ["o_custkey"],
        "output": [{"side": "build", "col": "c_phone"},
                   {"side": "build", "col": "c_acctbal"}]}
    probe = {"op": "project", "input": no_orders, "exprs": [
        {"as": "c_phone", "expr": {"col": "c_phone"}},
        {"as": "c_acctbal", "expr": {"col": "c_acctbal"}},
        {"as": "bal19", "expr": cast({"col": "c_acctbal"}, "decimal128", 19,
                                     6)}]}
    nlj = {"op": "nested_loop_join", "join_type": "inner", "build": avg,
           "probe": probe,
           "filter": cross_filter(("avg_bal", "lt", "bal19")),
           "output": [{"side": "build", "col": "avg_bal"},
                      {"side": "probe", "col": "c_phone"},
                      {"side": "probe", "col": "c_acctbal"}]}
    return {"op": "collect", "input": {
        "op": "hash_aggregate", "mode": "single", "group_by": ["cntrycode"],
        "aggs": [{"fn": "count", "as": "numcust"},
                 {"fn": "sum", "as": "totacctbal",
                  "expr": {"col": "c_acctbal"}}],
        "input": {"op": "project", "input": nlj, "exprs": [
            {"as": "cntrycode", "expr": code},
            {"as": "c_acctbal", "expr": {"col": "c_acctbal"}}]}}}


@pytest.fixture()
def q22_tables(reg):
    rng = np.random.default_rng(2201)
    n = 300
    codes = rng.choice(Q22_CODES + ["10", "11", "12"], size=n)
    phones = [f"{c}-{int(a):03d}-{int(b):04d}"
              for c, a, b in zip(codes, rng.integers(0, 1000, size=n),
                                 rng.integers(0, 10000, size=n))]
    bal = rng.integers(-99999, 999999, size=n)
    bmask = rng.random(n) < 0.05
    cust = reg("nlj_cust", pa.table({
        "c_custkey": pa.array(np.arange(n, dtype=np.int64)),
        "c_phone": pa.array(phones, type=pa.string()),
        "c_acctbal": dec_array(bal, 15, 2, bmask)}))
    okeys = rng.integers(0, n, size=200, dtype=np.int64)
    orders = reg("nlj_orders", pa.table({"o_custkey": pa.array(okeys)}))
    rows = [(i, phones[i], None if bmask[i] else int(bal[i]))
            for i in range(n)]
    return cust, orders, rows, set(okeys.tolist())


def test_stage_q22_shape(ctx, q22_tables):
    cust, orders, rows, ordered = q22_tables
    got = run(q22_plan(cust, orders, 0))
    in_codes = [r for r in rows if r[1][:2] in Q22_CODES]
    pos = [r[2] for r in in_codes if r[2] is not None and r[2] > 0]
    # Decimal128(15,2) avg -> Decimal128(19,6): half away from zero
    avg19 = round_half_away(sum(pos) * 10**4, len(pos))
    kept = [r for r in in_codes if r[0] not in ordered and r[2] is not None
            and r[2] * 10**4 > avg19]
    want = {}
    for _, phone, b in kept:
        cnt, tot = want.get(phone[:2], (0, 0))
        want[phone[:2]] = (cnt + 1, tot + b)
    assert sorted((r[0], r[1], int(r[2])) for r in got) == \
        sorted((c, cnt, tot) for c, (cnt, tot) in want.items())
    # the join is no no-op: some customers fall below the average
    candidates = [r for r in in_codes if r[0] not in ordered]
    assert 0 < len(kept) < len(candidates)
    assert set(want) == set(Q22_CODES)


def test_stage_q22_shape_with_an_empty_subquery(ctx, q22_tables):
    """No customer passes the subquery's filter: avg is NULL (or absent),
    NULL compares as not-greater, the join emits nothing."""
    cust, orders, _, _ = q22_tables
    assert run(q22_plan(cust, orders, 10**12)) == []


def test_stage_q11_shape(ctx, reg):
    """approved/q11.txt stage 11: per-key sums against
    CAST(CAST(total AS Float64) * 0.0001 AS Decimal128(38,15)), sorted by
    value descending."""
    rng = np.random.default_rng(1101)
    nkeys, n = 200, 1000
    key = np.concatenate([np.arange(nkeys), rng.integers(0, nkeys,
                                                         size=n - nkeys)])
    # values over nine decades, so 0.0001 of the total splits the keys
    val = (10 ** rng.uniform(0, 9, size=n)).astype(np.int64)
    t = reg("nlj_ps", pa.table({"ps_partkey": pa.array(key.astype(np.int64)),
                                "v": dec_array(val, 15, 2)}))
    total = {"op": "hash_aggregate", "mode": "single", "group_by": [],
             "aggs": [{"fn": "sum", "as": "total", "expr": {"col": "v"}}],
             "input": scan_of(t, "nlj_ps")}
    build = {"op": "project", "input": total, "exprs": [
        {"as": "thr", "expr": cast(
            {"mul": [cast({"col": "total"}, "float64"), {"lit_f64": 0.0001}]},
            "decimal128", 38, 15)}]}
    per_key = {"op": "hash_aggregate", "mode": "single",
               "group_by": ["ps_partkey"],
               "aggs": [{"fn": "sum", "as": "value", "expr": {"col": "v"}}],
               "input": scan_of(t, "nlj_ps")}
    probe = {"op": "project", "input": per_key, "exprs": [
        {"as": "ps_partkey", "expr": {"col": "ps_partkey"}},
        {"as": "value", "expr": {"col": "value"}},
        {"as": "value38", "expr": cast({"col": "value"}, "decimal128", 38,
                                       15)}]}
    nlj = {"op": "nested_loop_join", "join_type": "inner", "build": build,
           "probe": probe, "filter": cross_filter(("thr", "lt", "value38")),
           "output": [{"side": "build", "col": "thr"},
                      {"side": "probe", "col": "ps_partkey"},
                      {"side": "probe", "col": "value"}]}
    got = run({"op": "collect", "input": {
        "op": "sort", "keys": [{"col": "value", "desc": True}],
        "input": {"op": "project", "input": nlj, "exprs": [
            {"as": "ps_partkey", "expr": {"col": "ps_partkey"}},
            {"as": "value", "expr": {"col": "value"}}]}}})

    sums = Counter()
    for k, v in zip(key.tolist(), val.tolist()):
        sums[k] += v
    grand = sum(sums.values())
    # Decimal128 -> Float64 is (double)x / 1e2; the product goes back to
    # Decimal128(38,15) half away from zero
    prod = D((float(grand) / 1e2) * 0.0001) * D(10**15)
    thr = int(prod.quantize(D(1), rounding=decimal.ROUND_HALF_UP, context=CTX))
    want = [(k, v) for k, v in sums.items() if v * 10**13 > thr]
    assert 0 < len(want) < nkeys
    got = [(r[0], int(r[1])) for r in got]
    assert Counter(got) == Counter(want) and len(got) == len(want)
    values = [v for _, v in got]
    assert values == sorted(values, reverse=True)


JOIN_TYPES = ["inner", "semi", "anti", "left", "semi_build", "anti_build",
              "outer_build", "full"]
NONE2 = (None, None)


def make_sides(nb, np_, seed):
    """-> (build table, probe table, build rows, probe rows).  Build rows
    are (bid, lo, hi, bdec), probe rows (pid, x, pstr), as bg_execute_stage
    reports them (decimals as unscaled integer strings, NULL as None).  x
    runs over {0..9}; [lo, hi) is up to 3 wide; ~10 % of lo and x are
    NULL."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 10, size=nb, dtype=np.int64)
    hi = lo + rng.integers(0, 4, size=nb, dtype=np.int64)
    lom = rng.random(nb) < 0.1
    bdec = rng.integers(-10**6, 10**6, size=nb)
    bdm = rng.random(nb) < 0.2
    x = rng.integers(0, 10, size=np_, dtype=np.int64)
    xm = rng.random(np_) < 0.1
    pstr = [None if i % 7 == 3 else f"p{i % 97}" * (i % 3) for i in range(np_)]
    build = pa.table({
        "bid": pa.array(np.arange(nb, dtype=np.int64)),
        "b_lo": pa.array(lo, mask=lom), "b_hi": pa.array(hi),
        "bdec": dec_array(bdec, 15, 2, bdm)})
    probe = pa.table({
        "pid": pa.array(np.arange(np_, dtype=np.int64)),
        "p_x": pa.array(x, mask=xm),
        "pstr": pa.array(pstr, type=pa.string())})
    brows = [(i, None if lom[i] else int(lo[i]), int(hi[i]),
              None if bdm[i] else str(int(bdec[i]))) for i in range(nb)]
    prows = [(i, None if xm[i] else int(x[i]), pstr[i]) for i in range(np_)]
    return build, probe, brows, prows


BAND = cross_filter(("b_lo", "le", "p_x"), ("b_hi", "gt", "p_x"))


def band_passes(b, p):
    return b[1] is not None and p[1] is not None and b[1] <= p[1] < b[2]


def stage_reference(brows, prows, passes):
    """-> {join type: list of output rows}; outputs are bid, bdec and/or
    pid, pstr as stage_plan() asks for them."""
    bout = lambda b: (b[0], b[3])                               # noqa: E731
    pout = lambda p: (p[0], p[2])                               # noqa: E731
    inner, semi, anti, lone_probe, hit = [], [], [], [], set()
    for p in prows:
        ok = [b for b in brows if passes(b, p)]
        hit.update(b[0] for b in ok)
        inner += [bout(b) + pout(p) for b in ok]
        (semi if ok else anti).append(pout(p))
        if not ok:
            lone_probe.append(NONE2 + pout(p))
    lone_build = [bout(b) + NONE2 for b in brows if b[0] not in hit]
    return {"inner": inner, "semi": semi, "anti": anti,
            "left": inner + lone_probe,
            "semi_build": [bout(b) for b in brows if b[0] in hit],
            "anti_build": [bout(b) for b in brows if b[0] not in hit],
            "outer_build": inner + lone_build,
            "full": inner + lone_probe + lone_build}


def stage_plan(bscan, pscan, jt, filt, chunk=0):
    bout = [{"side": "build", "col": c} for c in ("bid", "bdec")]
    pout = [{"side": "probe", "col": c} for c in ("pid", "pstr")]
    output = (pout if jt in ("semi", "anti") else
              bout if jt in ("semi_build", "anti_build") else bout + pout)
    plan = {"op": "nested_loop_join", "build": bscan, "probe": pscan,
            "join_type": jt, "output": output}
    if filt:
        plan["filter"] = filt
    if chunk:
        plan["probe_chunk_rows"] = chunk
    return {"op": "collect", "input": plan}


@pytest.fixture(scope="module")
def band_sides():
    build, probe, brows, prows = make_sides(37, 300, seed=3701)
    want = stage_reference(brows, prows, band_passes)
    cross = stage_reference(brows, prows, lambda b, p: True)
    # on the reference alone: the band changes every type's result and
    # leaves rows matched and unmatched on both sides
    for jt in JOIN_TYPES:
        assert Counter(want[jt]) != Counter(cross[jt]), jt
    assert want["semi"] and want["anti"]
    assert want["semi_build"] and want["anti_build"]
    return build, probe, want


def test_stage_band_join_all_types_chunked_and_unchunked(ctx, reg, band_sides):
    build, probe, want = band_sides
    reg("nlj_b", build)
    reg("nlj_p", probe)
    bscan, pscan = scan_of(build, "nlj_b"), scan_of(probe, "nlj_p")
    for jt in JOIN_TYPES:
        whole, chunked = (run(stage_plan(bscan, pscan, jt, BAND, chunk))
                          for chunk in (0, 64))
        assert Counter(whole) == Counter(want[jt]), jt
        assert Counter(chunked) == Counter(want[jt]), jt
        assert len(whole) == len(chunked) == len(want[jt])
        if jt in ("semi_build", "anti_build", "semi", "anti"):
            assert whole == chunked == want[jt]      # that side's row order


def test_stage_cross_join_without_a_filter(ctx, reg):
    build, probe, brows, prows = make_sides(3, 130, seed=313)
    reg("nlj_cb", build)
    reg("nlj_cp", probe)
    got = run(stage_plan(scan_of(build, "nlj_cb"), scan_of(probe, "nlj_cp"),
                         "inner", None))
    # probe-major, ascending build row within a probe row
    assert got == [(b[0], b[3], p[0], p[2]) for p in prows for b in brows]
    assert len(got) == 3 * 130


@pytest.mark.parametrize("filt", [BAND, None], ids=["band", "cross"])
@pytest.mark.parametrize("empty", ["probe", "build"])
def test_stage_empty_side(ctx, reg, empty, filt):
    """The empty side is a filter node that keeps no row: `left` and `full`
    over an empty build NULL-extend every probe row, `outer_build` over an
    empty probe emits every build row."""
    build, probe, brows, prows = make_sides(20, 150, seed=929)
    reg("nlj_eb", build)
    reg("nlj_ep", probe)
    bscan, pscan = scan_of(build, "nlj_eb"), scan_of(probe, "nlj_ep")
    none = lambda scan, col: {"op": "filter", "input": scan, "predicates": [  # noqa: E731
        {"col": col, "cmp": "lt", "hi": -1}]}
    if empty == "probe":
        pscan, prows = none(pscan, "pid"), []
    else:
        bscan, brows = none(bscan, "bid"), []
    want = stage_reference(brows, prows,
                           band_passes if filt else lambda b, p: True)
    if empty == "probe":
        assert want["outer_build"] == [(b[0], b[3]) + NONE2 for b in brows]
        assert want["semi_build"] == [] and len(want["anti_build"]) == 20
    else:
        assert want["full"] == want["left"] == \
            [NONE2 + (p[0], p[2]) for p in prows]
    for jt in JOIN_TYPES:
        got = run(stage_plan(bscan, pscan, jt, filt))
        assert Counter(got) == Counter(want[jt]), jt
        assert len(got) == len(want[jt])
