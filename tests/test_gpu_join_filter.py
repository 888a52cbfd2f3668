"""Join residual filters (DataFusion HashJoinExec with filter: Some(..)):
bg_hashjoin_probe_count2_filtered / _fill2_filtered / _mark2_filtered at the
C ABI, and hash_join's "filter" through bg_execute_stage, on all eight join
types.  Every comparison is exact, against a plain-Python nested-loop
recomputation: a candidate is a key-equal pair of non-NULL keys, it passes
when the filter is TRUE (NULL counts as FALSE), and each join type reads
"match" as "passing candidate"."""
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
def cols(*cs):
    return (gpu.BgColumn * len(cs))(*cs)


class Case:
    """Duplicate build keys over a domain of 2n/3, ~10 % NULL keys on both
    sides, cross columns over {0..3} with ~10 % NULLs, two random masks per
    side; the last build row is valid, probed by probe row 0 and passes the
    q21 filter there."""

    def __init__(self, n_build, seed):
        rng = np.random.default_rng(seed)
        self.nb, self.np_ = n_build, 4 * n_build + 50
        domain = max(2, n_build * 2 // 3)
        self.bkeys = rng.integers(0, domain, size=self.nb, dtype=np.int64)
        self.bvalid = rng.random(self.nb) >= 0.1
        self.pkeys = rng.integers(0, domain + 5, size=self.np_,
                                  dtype=np.int64)
        self.pvalid = rng.random(self.np_) >= 0.1
        self.bx = rng.integers(0, 4, size=self.nb, dtype=np.int64)
        self.bxv = rng.random(self.nb) >= 0.1
        self.px = rng.integers(0, 4, size=self.np_, dtype=np.int64)
        self.pxv = rng.random(self.np_) >= 0.1
        self.bm = [rng.random(self.nb) < 0.6 for _ in range(2)]
        self.pm = [rng.random(self.np_) < 0.6 for _ in range(2)]
        self.bkeys[-1], self.bvalid[-1] = 0, True
        self.pkeys[0], self.pvalid[0] = 0, True
        self.bx[-1], self.bxv[-1], self.px[0], self.pxv[0] = 0, True, 1, True


# a filter: list of groups {"bm": mask index, "pm": mask index, "cross":
# [cmp names]}; every cross term compares the case's bx with its px
SHAPES = {
    "q21": [{"cross": ["ne"]}],
    "two_groups": [{"bm": 0, "pm": 0, "cross": ["lt"]},
                   {"bm": 1, "pm": 1, "cross": ["eq"]}],
    "masks_only": [{"bm": 0, "pm": 1}],
}


def passes_fn(case, shape):
    def passes(b, p):
        for g in shape:
            if "bm" in g and not case.bm[g["bm"]][b]:
                continue
            if "pm" in g and not case.pm[g["pm"]][p]:
                continue
            if all(case.bxv[b] and case.pxv[p] and
                   OPS[c](int(case.bx[b]), int(case.px[p]))
                   for c in g.get("cross", [])):
                return True
        return False
    return passes


def reference(case, passes, lo=0, hi=None):
    """Nested-loop join of probe rows [lo, hi) under `passes` (None: no
    filter).  Probe indices are relative to lo."""
    hi = case.np_ if hi is None else hi
    index = defaultdict(list)
    for b in range(case.nb):
        if case.bvalid[b]:
            index[int(case.bkeys[b])].append(b)
    r = {"inner": [], "semi": [], "anti": [], "left": [], "ok": {},
         "marked": set(), "key_matched": set(), "mixed": 0, "all_fail": 0}
    for p in range(lo, hi):
        cand = index.get(int(case.pkeys[p]), []) if case.pvalid[p] else []
        ok = [b for b in cand if passes is None or passes(b, p)]
        q = p - lo
        r["key_matched"].update(cand)
        r["marked"].update(ok)
        r["inner"] += [(q, b) for b in ok]
        r["left"] += [(q, b) for b in ok] or [(q, NULL_IDX)]
        (r["semi"] if ok else r["anti"]).append(q)
        r["ok"][q] = set(ok)
        r["mixed"] += bool(ok) and len(ok) < len(cand)
        r["all_fail"] += bool(cand) and not ok
    return r


def by_type(r, nb):
    """One comparable value per join type."""
    unmarked = sorted(set(range(nb)) - r["marked"])
    return {"inner": sorted(r["inner"]), "semi": r["semi"], "anti": r["anti"],
            "left": sorted(r["left"]), "semi_build": sorted(r["marked"]),
            "anti_build": unmarked,
            "outer_build": (sorted(r["inner"]), unmarked),
            "full": (sorted(r["left"]), unmarked)}


def assert_meaningful(filtered, plain, nb):
    """On the reference alone: the case separates a filtered join from an
    unfiltered one for every type."""
    assert filtered["mixed"] >= 1          # passing and failing candidates
    assert filtered["all_fail"] >= 1       # candidates, all failing
    assert filtered["key_matched"] - filtered["marked"]
    f, u = by_type(filtered, nb), by_type(plain, nb)
    for jt in f:
        assert f[jt] != u[jt], jt


# cross-column encodings: monotone maps of {0..3}, negative values included
def enc_int64(v):
    return (v - 2) * 10**12


def enc_date32(v):
    return ((v - 2) * 1000).astype(np.int32)


def enc_dict8(v):
    return v.astype(np.uint8)


def enc_dec128(v):
    out = bytearray()
    for x in v:
        out += ((int(x) - 2) * (2**70 + 12345)).to_bytes(16, "little",
                                                         signed=True)
    return np.frombuffer(bytes(out), dtype=np.uint8)


DTYPES = {"int64": (gpu.BG_DT_INT64, enc_int64),
          "date32": (gpu.BG_DT_DATE32, enc_date32),
          "dict8": (gpu.BG_DT_DICT8, enc_dict8),
          "decimal128": (gpu.BG_DT_DECIMAL128, enc_dec128)}


class Dev:
    """The case's build side on the device, and probe slices on demand."""

    def __init__(self, ctx, case, dtype="int64"):
        self.ctx, self.case = ctx, case
        self.dt, self.enc = DTYPES[dtype]
        self.bcol, _ = ctx.upload_column(case.bkeys, gpu.BG_DT_INT64,
                                         validity=bits(case.bvalid))
        self.bx = ctx.upload(self.enc(case.bx))
        self.bxv = ctx.upload(bits(case.bxv))
        self.bm = [ctx.upload(bits(m)) for m in case.bm]

    def probe(self, shape, lo=0, hi=None):
        """-> (probe key column, terms array, nterms, keep-alive)."""
        c, ctx = self.case, self.ctx
        hi = c.np_ if hi is None else hi
        pcol, _ = ctx.upload_column(c.pkeys[lo:hi], gpu.BG_DT_INT64,
                                    validity=bits(c.pvalid[lo:hi]))
        px = ctx.upload(self.enc(c.px[lo:hi]))
        pxv = ctx.upload(bits(c.pxv[lo:hi]))
        pm = [ctx.upload(bits(m[lo:hi])) for m in c.pm]
        terms = []
        for gi, g in enumerate(shape):
            if "bm" in g:
                terms.append(term(gpu.BG_JF_BUILD_MASK, gi, b=self.bm[g["bm"]]))
            if "pm" in g:
                terms.append(term(gpu.BG_JF_PROBE_MASK, gi, p=pm[g["pm"]]))
            for cmp in g.get("cross", []):
                terms.append(term(gpu.BG_JF_CROSS, gi, self.dt, CMP_CODE[cmp],
                                  self.bx, self.bxv, px, pxv))
        return pcol, terms_array(terms), len(terms), (px, pxv, pm)


class Join:
    """One bg_hashjoin_build2 handle over a single Int64 key column."""

    def __init__(self, ctx, bcol, n_build):
        self.ctx, self.bcol, self.n_build = ctx, bcol, n_build
        self.h = ctypes.c_void_p()
        assert ctx.L.bg_hashjoin_build2(cols(bcol), 1, n_build,
                                        ctypes.byref(self.h)) == BG_OK

    def mark(self, pcol, n, terms, nterms):
        assert self.ctx.L.bg_hashjoin_probe_mark2_filtered(
            self.h, cols(pcol), 1, n, terms, nterms) == BG_OK

    def rows(self, matched):
        out = self.ctx.alloc(4 * self.n_build + 4)
        cnt = I64(-1)
        assert self.ctx.L.bg_hashjoin_build_rows2(
            self.h, matched, ctypes.byref(cnt), out.ptr) == BG_OK
        return out.download(np.uint32, cnt.value).astype(np.int64).tolist()

    def _filled(self, m, fill):
        """Pair buffers pre-filled with a sentinel; nothing may be written
        past the reported count."""
        pad = 8
        bufs = []
        for _ in range(2):
            b = self.ctx.alloc(4 * (m + pad))
            b.upload(np.full(m + pad, SENTINEL, dtype=np.uint32))
            bufs.append(b)
        assert fill(bufs[0].ptr, bufs[1].ptr) == BG_OK
        got = [b.download(np.uint32, m + pad) for b in bufs]
        for g in got:
            assert np.all(g[m:] == SENTINEL)
        return got[0][:m], got[1][:m]

    def pairs(self, pcol, n, jt, terms, nterms):
        L, m = self.ctx.L, I64(-1)
        assert L.bg_hashjoin_probe_count2_filtered(
            self.h, cols(pcol), 1, n, jt, terms, nterms,
            ctypes.byref(m)) == BG_OK
        return self._filled(m.value, lambda op, ob:
                            L.bg_hashjoin_probe_fill2_filtered(
                                self.h, cols(pcol), 1, n, jt, terms, nterms,
                                op, ob))

    def pairs_unfiltered(self, pcol, n, jt):
        L, m = self.ctx.L, I64(-1)
        assert L.bg_hashjoin_probe_count2(self.h, cols(pcol), 1, n, jt,
                                          ctypes.byref(m)) == BG_OK
        return self._filled(m.value, lambda op, ob:
                            L.bg_hashjoin_probe_fill2(
                                self.h, cols(pcol), 1, n, jt, op, ob))

    def free(self):
        assert self.ctx.L.bg_hashjoin_free2(self.h) == BG_OK
        self.h = ctypes.c_void_p()


def as_pairs(op, ob):
    assert np.all(np.diff(op.astype(np.int64)) >= 0)   # probe-major
    return sorted(zip(op.tolist(), ob.tolist()))


def check_all_types(ctx, dev, shape, want):
    """All eight types of one filter against the reference `want`."""
    case = dev.case
    pcol, terms, nt, _keep = dev.probe(shape)
    n, nb = case.np_, case.nb
    unmarked = sorted(set(range(nb)) - want["marked"])
    j = Join(ctx, dev.bcol, nb)
    try:
        assert as_pairs(*j.pairs(pcol, n, INNER, terms, nt)) == \
            sorted(want["inner"])
        op, ob = j.pairs(pcol, n, SEMI, terms, nt)
        assert op.tolist() == want["semi"]              # once each, ascending
        for p, b in zip(op.tolist(), ob.tolist()):
            assert b in want["ok"][p]                   # some passing one
        op, ob = j.pairs(pcol, n, ANTI, terms, nt)
        assert op.tolist() == want["anti"]
        assert np.all(ob == NULL_IDX)
        assert as_pairs(*j.pairs(pcol, n, OUTER_PROBE, terms, nt)) == \
            sorted(want["left"])
        assert j.rows(1) == []                          # nothing marked yet
        assert as_pairs(*j.pairs(pcol, n, OUTER_BUILD, terms, nt)) == \
            sorted(want["inner"])
        assert j.rows(1) == sorted(want["marked"])      # only passing pairs
        assert j.rows(0) == unmarked
    finally:
        j.free()
    j = Join(ctx, dev.bcol, nb)
    try:
        assert as_pairs(*j.pairs(pcol, n, OUTER_FULL, terms, nt)) == \
            sorted(want["left"])
        assert j.rows(1) == sorted(want["marked"])
        assert j.rows(0) == unmarked
    finally:
        j.free()
    # semi_build / anti_build: mark, then list the build rows
    j = Join(ctx, dev.bcol, nb)
    try:
        j.mark(pcol, n, terms, nt)
        assert j.rows(1) == sorted(want["marked"])
        assert j.rows(0) == unmarked
    finally:
        j.free()


_CASES = {}


def case_of(n_build):
    if n_build not in _CASES:
        _CASES[n_build] = Case(n_build, seed=100 + n_build)
    return _CASES[n_build]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n_build", [1, 63, 64, 65, 1000])
def test_all_types_at_the_abi(ctx, n_build, shape):
    case = case_of(n_build)
    want = reference(case, passes_fn(case, SHAPES[shape]))
    if n_build == 1000:
        assert_meaningful(want, reference(case, None), n_build)
    check_all_types(ctx, Dev(ctx, case), SHAPES[shape], want)


@pytest.mark.parametrize("dtype", ["date32", "dict8", "decimal128"])
def test_cross_term_dtypes(ctx, dtype):
    """The cross term's other dtypes (Int64 is above); Decimal128 values
    are negative and wider than 64 bits, so both words and the sign count."""
    case = case_of(1000)
    dev = Dev(ctx, case, dtype)
    for shape in ("q21", "two_groups"):
        want = reference(case, passes_fn(case, SHAPES[shape]))
        check_all_types(ctx, dev, SHAPES[shape], want)
    four = [{"cross": ["le", "ge", "ne", "gt"]}, {"pm": 0, "cross": ["eq"]}]
    check_all_types(ctx, dev, four, reference(case, passes_fn(case, four)))


def const_terms(ctx, case, build_bit, probe_bit):
    """One group: a build mask and a probe mask of constant bits."""
    bm = ctx.upload(bits(np.full(case.nb, build_bit, dtype=bool)))
    pm = ctx.upload(bits(np.full(case.np_, probe_bit, dtype=bool)))
    return terms_array([term(gpu.BG_JF_BUILD_MASK, 0, b=bm),
                        term(gpu.BG_JF_PROBE_MASK, 0, p=pm)]), 2, (bm, pm)


def test_pass_everything_equals_the_unfiltered_entries(ctx):
    case = case_of(1000)
    dev = Dev(ctx, case)
    pcol, _, _, _keep = dev.probe([])
    terms, nt, _keep2 = const_terms(ctx, case, True, True)
    j, u = Join(ctx, dev.bcol, case.nb), Join(ctx, dev.bcol, case.nb)
    try:
        for jt in (INNER, SEMI, ANTI, OUTER_PROBE, OUTER_BUILD, OUTER_FULL):
            got = j.pairs(pcol, case.np_, jt, terms, nt)
            want = j.pairs_unfiltered(pcol, case.np_, jt)
            # element for element: same table, same walk, same chain order
            assert np.array_equal(got[0], want[0]), jt
            assert np.array_equal(got[1], want[1]), jt
            assert len(got[0]) > 0
        # marks do not depend on chain order: a table that only ever saw
        # the unfiltered entries carries the same ones
        u.pairs_unfiltered(pcol, case.np_, OUTER_FULL)
        assert j.rows(1) == u.rows(1) != []
    finally:
        j.free()
        u.free()
    j, u = Join(ctx, dev.bcol, case.nb), Join(ctx, dev.bcol, case.nb)
    try:
        j.mark(pcol, case.np_, terms, nt)
        assert ctx.L.bg_hashjoin_probe_mark2(u.h, cols(pcol), 1,
                                             case.np_) == BG_OK
        assert j.rows(1) == u.rows(1) != []
        assert j.rows(0) == u.rows(0)
    finally:
        j.free()
        u.free()


@pytest.mark.parametrize("dead", ["probe_mask", "build_mask"])
def test_pass_nothing(ctx, dead):
    """All-zero probe mask: no row has a live group, nothing is hashed.
    All-zero build mask: every chain is walked and every candidate fails."""
    case = case_of(1000)
    dev = Dev(ctx, case)
    pcol, _, _, _keep = dev.probe([])
    terms, nt, _keep2 = const_terms(ctx, case, dead != "build_mask",
                                    dead != "probe_mask")
    n, every = case.np_, list(range(case.np_))
    j = Join(ctx, dev.bcol, case.nb)
    try:
        for jt in (INNER, SEMI):
            op, ob = j.pairs(pcol, n, jt, terms, nt)
            assert len(op) == len(ob) == 0
        for jt in (ANTI, OUTER_PROBE, OUTER_FULL):
            op, ob = j.pairs(pcol, n, jt, terms, nt)
            assert op.tolist() == every and np.all(ob == NULL_IDX)
        op, ob = j.pairs(pcol, n, OUTER_BUILD, terms, nt)
        assert len(op) == 0
        j.mark(pcol, n, terms, nt)
        assert j.rows(1) == []                            # semi_build
        assert j.rows(0) == list(range(case.nb))          # anti_build, tails
    finally:
        j.free()


def test_marks_accumulate_and_the_bitmap_is_allocated_once(ctx):
    case = case_of(1000)
    dev = Dev(ctx, case)
    shape = SHAPES["two_groups"]
    passes = passes_fn(case, shape)
    j = Join(ctx, dev.bcol, case.nb)
    try:
        gc.collect()
        built = ctx.pool_stats()[1]
        seen = set()
        for k, (lo, hi) in enumerate([(0, 1300), (1300, case.np_)]):
            pcol, terms, nt, keep = dev.probe(shape, lo, hi)
            gc.collect()
            before = ctx.pool_stats()[1]
            j.mark(pcol, hi - lo, terms, nt)
            # the first call adds the bitmap, the second adds nothing
            assert ctx.pool_stats()[1] == before + (1 if k == 0 else 0)
            seen |= reference(case, passes, lo, hi)["marked"]
            assert j.rows(1) == sorted(seen)
            del pcol, terms, keep
        gc.collect()
        assert ctx.pool_stats()[1] == built + 1
        assert sorted(seen) == sorted(reference(case, passes)["marked"])
    finally:
        j.free()


def test_refusals_and_pool_balance(ctx):
    case = case_of(65)
    dev = Dev(ctx, case)
    pcol, terms, nt, _keep = dev.probe(SHAPES["q21"])
    other, nt2, _keep2 = const_terms(ctx, case, True, True)
    out = ctx.alloc(4 * 4096)
    L, n, m = ctx.L, case.np_, I64()
    gc.collect()
    base = ctx.pool_stats()[:2]
    j = Join(ctx, dev.bcol, case.nb)
    # zero terms: the unfiltered entries are the ones to call
    for none in (None, terms):
        assert L.bg_hashjoin_probe_count2_filtered(
            j.h, cols(pcol), 1, n, INNER, none, 0,
            ctypes.byref(m)) == BG_ERR_INVALID
        assert b"unfiltered" in L.bg_last_error()
        assert L.bg_hashjoin_probe_fill2_filtered(
            j.h, cols(pcol), 1, n, INNER, none, 0, out.ptr,
            out.ptr) == BG_ERR_INVALID
        assert L.bg_hashjoin_probe_mark2_filtered(
            j.h, cols(pcol), 1, n, none, 0) == BG_ERR_INVALID
    # build-rows-only types have no pairs, filtered or not
    for jt in (SEMI_BUILD, ANTI_BUILD):
        assert L.bg_hashjoin_probe_count2_filtered(
            j.h, cols(pcol), 1, n, jt, terms, nt,
            ctypes.byref(m)) == BG_ERR_INVALID
        assert b"bg_hashjoin_probe_mark2" in L.bg_last_error()
    # malformed terms
    bad = [term(gpu.BG_JF_CROSS, 4, gpu.BG_DT_INT64, 0, dev.bx, None, dev.bx),
           term(gpu.BG_JF_CROSS, 0, gpu.BG_DT_INT64, 6, dev.bx, None, dev.bx),
           term(gpu.BG_JF_CROSS, 0, gpu.BG_DT_UTF8, 0, dev.bx, None, dev.bx),
           term(gpu.BG_JF_CROSS, 0, gpu.BG_DT_FLOAT64, 0, dev.bx, None,
                dev.bx),
           term(gpu.BG_JF_CROSS, 1, gpu.BG_DT_INT64, 0, dev.bx, None, dev.bx),
           term(7, 0), term(gpu.BG_JF_BUILD_MASK, 0)]
    for t in bad:
        assert L.bg_hashjoin_probe_count2_filtered(
            j.h, cols(pcol), 1, n, INNER, terms_array([t]), 1,
            ctypes.byref(m)) < 0
    five = terms_array([terms[0]] * 5)
    assert L.bg_hashjoin_probe_count2_filtered(
        j.h, cols(pcol), 1, n, INNER, five, 5,
        ctypes.byref(m)) == BG_ERR_INVALID
    # a fill must repeat the count's type and terms: its offsets are only
    # good for those
    assert L.bg_hashjoin_probe_count2_filtered(
        j.h, cols(pcol), 1, n, INNER, terms, nt, ctypes.byref(m)) == BG_OK
    assert 0 < m.value <= 4096
    assert L.bg_hashjoin_probe_fill2_filtered(
        j.h, cols(pcol), 1, n, INNER, other, nt2, out.ptr,
        out.ptr) == BG_ERR_INVALID
    assert L.bg_hashjoin_probe_fill2_filtered(
        j.h, cols(pcol), 1, n, OUTER_PROBE, terms, nt, out.ptr,
        out.ptr) == BG_ERR_INVALID
    assert L.bg_hashjoin_probe_fill2(
        j.h, cols(pcol), 1, n, INNER, out.ptr, out.ptr) == BG_ERR_INVALID
    assert L.bg_hashjoin_probe_fill2_filtered(
        j.h, cols(pcol), 1, n, INNER, terms, nt, out.ptr, out.ptr) == BG_OK
    j.mark(pcol, n, terms, nt)
    j.free()
    gc.collect()
    assert ctx.pool_stats()[:2] == base


# ---------------------------------------------------------------------------
# stage level
# ---------------------------------------------------------------------------
def _doc(plan):
    return {"job_id": "job-jf", "stage_id": 1, "task_id": 0,
            "work_dir": "/tmp/stage-tests", "plan": plan}


def run(plan):
    return [tuple(r) for r in stage.execute(_doc(plan))["rows"]]


NAMES = ["FRANCE", "GERMANY", "PERU"]


def make_sides(nb, np_, seed):
    """-> (build table, probe table, build rows, probe rows); a row is
    (k1, k2, id, x, name, dec, str) in the form bg_execute_stage reports
    (decimals as unscaled integer strings, NULL as None).  k1 has duplicates
    and ~10 % NULLs, k2 is drawn independently so the composite key rejects
    k1-only matches; x in {0..3} with ~10 % NULLs and name feed the filter
    and are never output."""
    rng = np.random.default_rng(seed)
    out = []
    for n, tag, extra in ((nb, "b", 0), (np_, "p", 40)):
        k = rng.integers(0, nb // 2 + extra, size=n, dtype=np.int64)
        km = rng.random(n) < 0.1
        k2 = [f"s{v}" for v in rng.integers(0, 3, size=n)]
        x = rng.integers(0, 4, size=n, dtype=np.int64)
        xm = rng.random(n) < 0.1
        name = [NAMES[v] for v in rng.integers(0, 3, size=n)]
        dec = rng.integers(-10**6, 10**6, size=n)
        dm = rng.random(n) < 0.2
        st = [None if i % 7 == 3 else f"{tag}{i % 97}" * (i % 3)
              for i in range(n)]
        t = pa.table({
            f"{tag}k1": pa.array(k, mask=km),
            f"{tag}k2": pa.array(k2),
            f"{tag}id": pa.array(np.arange(n, dtype=np.int64)),
            f"{tag}x": pa.array(x, mask=xm),
            f"{tag}name": pa.array(name),
            f"{tag}dec": pa.array(
                [None if m else decimal.Decimal(int(v)) / 100
                 for v, m in zip(dec, dm)], type=pa.decimal128(15, 2)),
            f"{tag}str": pa.array(st, type=pa.string()),
        })
        rows = [(None if km[i] else int(k[i]), k2[i], i,
                 None if xm[i] else int(x[i]), name[i],
                 None if dm[i] else str(int(dec[i])), st[i])
                for i in range(n)]
        out.append((t, rows))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# (bname in FRANCE/GERMANY and bx != px) or (pname = FRANCE and bx < px)
STAGE_FILTER = {"any": [
    {"build": [{"col": "bname", "in": ["FRANCE", "GERMANY"]}],
     "cross": [{"build": "bx", "cmp": "ne", "probe": "px"}]},
    {"probe": [{"col": "pname", "like": "FRANCE"}],
     "cross": [{"build": "bx", "cmp": "lt", "probe": "px"}]}]}


def stage_passes(b, p):
    x, y = b[3], p[3]
    if x is None or y is None:
        return False
    return (b[4] in ("FRANCE", "GERMANY") and x != y) or \
        (p[4] == "FRANCE" and x < y)


JOIN_TYPES = ["inner", "semi", "anti", "left", "semi_build", "anti_build",
              "outer_build", "full"]
NONE3 = (None, None, None)


def out_of(r):
    return (r[2], r[5], r[6])               # id, dec, str


def stage_reference(brows, prows, nkeys, passes):
    """-> ({join type: list of output rows}, stats); outputs are bid, bdec,
    bstr and/or pid, pdec, pstr as stage_plan() asks for them."""
    def key(r):
        return None if r[0] is None else r[:nkeys]

    index = defaultdict(list)
    for r in brows:
        if key(r) is not None:
            index[key(r)].append(r)
    inner, semi, anti, lone_probe, hit, touched = [], [], [], [], set(), set()
    mixed = all_fail = 0
    for p in prows:
        cand = index.get(key(p), []) if key(p) is not None else []
        ok = [b for b in cand if passes is None or passes(b, p)]
        touched.update(b[2] for b in cand)
        hit.update(b[2] for b in ok)
        inner += [out_of(b) + out_of(p) for b in ok]
        (semi if ok else anti).append(out_of(p))
        if not ok:
            lone_probe.append(NONE3 + out_of(p))
        mixed += bool(ok) and len(ok) < len(cand)
        all_fail += bool(cand) and not ok
    lone_build = [out_of(b) + NONE3 for b in brows if b[2] not in hit]
    res = {"inner": inner, "semi": semi, "anti": anti,
           "left": inner + lone_probe,
           "semi_build": [out_of(b) for b in brows if b[2] in hit],
           "anti_build": [out_of(b) for b in brows if b[2] not in hit],
           "outer_build": inner + lone_build,
           "full": inner + lone_probe + lone_build}
    return res, {"mixed": mixed, "all_fail": all_fail,
                 "never_passed": len(touched - hit)}


def stage_plan(bscan, pscan, nkeys, jt, filt, chunk=0):
    bout = [{"side": "build", "col": c} for c in ("bid", "bdec", "bstr")]
    pout = [{"side": "probe", "col": c} for c in ("pid", "pdec", "pstr")]
    output = (pout if jt in ("semi", "anti") else
              bout if jt in ("semi_build", "anti_build") else bout + pout)
    plan = {"op": "hash_join", "build": bscan, "probe": pscan,
            "build_keys": ["bk1", "bk2"][:nkeys],
            "probe_keys": ["pk1", "pk2"][:nkeys],
            "join_type": jt, "output": output}
    if filt:
        plan["filter"] = filt
    if chunk:
        plan["probe_chunk_rows"] = chunk
    return {"op": "collect", "input": plan}


@pytest.fixture(scope="module")
def sides_500():
    build, probe, brows, prows = make_sides(500, 20_000, seed=61)
    refs = {}
    for nkeys in (1, 2):
        want, stats = stage_reference(brows, prows, nkeys, stage_passes)
        plain, _ = stage_reference(brows, prows, nkeys, None)
        # on the reference alone: the filter changes every type's result
        assert stats["mixed"] and stats["all_fail"] and stats["never_passed"]
        for jt in JOIN_TYPES:
            assert Counter(want[jt]) != Counter(plain[jt]), (nkeys, jt)
        refs[nkeys] = want
    return build, probe, refs


@pytest.mark.parametrize("nkeys", [1, 2], ids=["int64", "int64+utf8"])
def test_stage_all_types_chunked_and_unchunked(ctx, reg, sides_500, nkeys):
    build, probe, refs = sides_500
    reg("jf_b", build)
    reg("jf_p", probe)
    bscan, pscan = scan_of(build, "jf_b"), scan_of(probe, "jf_p")
    for jt in JOIN_TYPES:
        want = refs[nkeys][jt]
        whole, chunked = (run(stage_plan(bscan, pscan, nkeys, jt,
                                         STAGE_FILTER, chunk))
                          for chunk in (0, 4096))
        assert Counter(whole) == Counter(want), jt
        assert Counter(chunked) == Counter(want), jt
        assert len(whole) == len(chunked) == len(want)
        if jt in ("semi_build", "anti_build"):
            assert whole == chunked == want             # ascending build order
        if jt in ("semi", "anti"):
            assert whole == chunked == want             # probe order


@pytest.mark.parametrize("empty", ["probe", "build"])
def test_stage_empty_side(ctx, reg, empty):
    """The empty side is a filter node that keeps no row; `full` over an
    empty build side NULL-extends every probe row."""
    build, probe, brows, prows = make_sides(300, 1_000, seed=71)
    reg("jfe_b", build)
    reg("jfe_p", probe)
    bscan, pscan = scan_of(build, "jfe_b"), scan_of(probe, "jfe_p")
    none = lambda scan, col: {"op": "filter", "input": scan, "predicates": [  # noqa: E731
        {"col": col, "cmp": "lt", "hi": -1}]}
    if empty == "probe":
        pscan, prows = none(pscan, "pid"), []
    else:
        bscan, brows = none(bscan, "bid"), []
    want, _ = stage_reference(brows, prows, 1, stage_passes)
    if empty == "probe":
        assert want["semi_build"] == [] and len(want["anti_build"]) == 300
    else:
        assert want["full"] == [NONE3 + out_of(p) for p in prows]
    for jt in JOIN_TYPES:
        got = run(stage_plan(bscan, pscan, 1, jt, STAGE_FILTER))
        assert Counter(got) == Counter(want[jt]), jt
        assert len(got) == len(want[jt])


def test_q21_shape(ctx, reg):
    """l1 (late) semi_build lineitem on l_orderkey with l_suppkey !=
    l_suppkey, feeding anti_build against the late lineitems with the same
    filter (approved/q21.txt): late lines of multi-supplier orders where no
    OTHER supplier was late."""
    rng = np.random.default_rng(83)
    n = 2_000
    okey = rng.integers(0, 500, size=n, dtype=np.int64)
    supp = rng.integers(0, 6, size=n, dtype=np.int64)
    late = (rng.random(n) < 0.4).astype(np.int64)
    li = pa.table({"l_orderkey": pa.array(okey), "l_suppkey": pa.array(supp),
                   "l_late": pa.array(late),
                   "l_id": pa.array(np.arange(n, dtype=np.int64))})
    reg("q21_l", li)
    scan = scan_of(li, "q21_l")
    late_only = {"op": "filter", "input": scan, "predicates": [
        {"col": "l_late", "cmp": "eq", "lo": 1, "hi": 1}]}
    ne = {"any": [{"cross": [{"build": "l_suppkey", "cmp": "ne",
                              "probe": "l_suppkey"}]}]}
    semi = {"op": "hash_join", "join_type": "semi_build",
            "build": late_only, "probe": scan, "filter": ne,
            "build_keys": ["l_orderkey"], "probe_keys": ["l_orderkey"],
            "output": [{"side": "build", "col": c}
                       for c in ("l_orderkey", "l_suppkey", "l_id")]}
    anti = {"op": "hash_join", "join_type": "anti_build",
            "build": semi, "probe": late_only, "filter": ne,
            "build_keys": ["l_orderkey"], "probe_keys": ["l_orderkey"],
            "probe_chunk_rows": 256,
            "output": [{"side": "build", "col": "l_id"}]}
    got = [r[0] for r in run({"op": "collect", "input": anti})]

    lines_of = defaultdict(list)
    for i in range(n):
        lines_of[int(okey[i])].append(i)

    def other(i, only_late):
        return any(supp[j] != supp[i] and (late[j] or not only_late)
                   for j in lines_of[int(okey[i])])

    lates = [i for i in range(n) if late[i]]
    after_semi = [i for i in lates if other(i, False)]
    want = [i for i in after_semi if not other(i, True)]
    assert got == want
    # neither join is a no-op, and dropping the filters changes the result
    assert 0 < len(want) < len(after_semi) < len(lates)
    semi.pop("filter")
    anti.pop("filter")
    assert [r[0] for r in run({"op": "collect", "input": anti})] != want


def test_q7_shape(ctx, reg):
    """Inner join with (n1 = FRANCE and n2 = GERMANY) or (n1 = GERMANY and
    n2 = FRANCE), one literal per side in each group (approved/q7.txt)."""
    rng = np.random.default_rng(89)
    nb, np_ = 300, 6_000
    bkey = rng.integers(0, 150, size=nb, dtype=np.int64)
    pkey = rng.integers(0, 170, size=np_, dtype=np.int64)
    n1 = [NAMES[v] for v in rng.integers(0, 3, size=nb)]
    n2 = [None if i % 11 == 0 else NAMES[v]
          for i, v in enumerate(rng.integers(0, 3, size=np_))]
    b = pa.table({"s_key": pa.array(bkey), "n1": pa.array(n1),
                  "s_id": pa.array(np.arange(nb, dtype=np.int64))})
    p = pa.table({"c_key": pa.array(pkey),
                  "n2": pa.array(n2, type=pa.string()),
                  "c_id": pa.array(np.arange(np_, dtype=np.int64))})
    reg("q7_b", b)
    reg("q7_p", p)
    filt = {"any": [
        {"build": [{"col": "n1", "in": ["FRANCE"]}],
         "probe": [{"col": "n2", "in": ["GERMANY"]}]},
        {"build": [{"col": "n1", "like": "GERMANY"}],
         "probe": [{"col": "n2", "like": "FRANCE"}]}]}
    plan = {"op": "collect", "input": {
        "op": "hash_join", "join_type": "inner", "filter": filt,
        "build": scan_of(b, "q7_b"), "probe": scan_of(p, "q7_p"),
        "build_keys": ["s_key"], "probe_keys": ["c_key"],
        "output": [{"side": "build", "col": "s_id"},
                   {"side": "build", "col": "n1"},
                   {"side": "probe", "col": "c_id"},
                   {"side": "probe", "col": "n2"}]}}
    got = run(plan)
    pairs = {("FRANCE", "GERMANY"), ("GERMANY", "FRANCE")}
    want = [(i, n1[i], j, n2[j]) for j in range(np_) for i in range(nb)
            if bkey[i] == pkey[j] and (n1[i], n2[j]) in pairs]
    assert Counter(got) == Counter(want) and len(got) == len(want)
    assert {(r[1], r[3]) for r in got} == pairs
    plan["input"].pop("filter")
    assert len(run(plan)) > len(want) > 0
