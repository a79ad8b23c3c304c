"""tests/_pagecheck.py pinned in both directions, on the CPU.

Accepts: everything pyrj.pages' packers produce (the grid of tests/test_pages.py) and the C oracle's
pages (results of the golden unit cases, of generated plans, tables read from CSV), decoded to the very
content pyrj.pages decodes.  Rejects: one hand-made mutation of a valid page per rule, each raising
with exactly that rule's name; test_every_rule_has_a_rejecting_case keeps the list complete.

One known exception on the accepting side is pinned rather than hidden: the reference's
ColumnInserter<T>::insert tests the fit of an 8-byte value with a literal 4 (include/plan.h:205), so a
NULL-bearing INT64 / FP64 page read from CSV may end with a value whose last bytes the bitmap then
overwrites (tests/test_ingest_oracle.py clobbered_cells).  Such a page breaks `fit`, and the strict
reader says so for exactly those pages."""
import time

import numpy as np
import pytest

import _aggref
import _csvgen as g
import _golden
import _oracle
import _pagecheck as pc
import test_gpu_fuzz as fz
import test_ingest_oracle as io
import test_mixed_plan_ref as mr
from _pagecheck import PageFormatError, check_column
from pyrj import pages as pg
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
PS = pg.PAGE_SIZE
GRID = [(0, 0.0), (1, 0.0), (1984, 0.0), (1985, 0.0), (5000, 0.0), (5000, 0.3), (30000, 0.97), (70000, 1.0), (3, 1.0)]


def accept_table(t, what=""):
    """every column passes, and decodes to what pyrj.pages decodes"""
    got = pc.check_table(t)
    assert pc.same_as(got, pl.decode_table(t)), what
    return got


def fixed_values(rng, dtype, n):
    if dtype == F64:
        v = rng.standard_normal(n)
        v[: min(n, 4)] = [np.nan, -0.0, np.inf, 5e-324][: min(n, 4)]
        return v
    info = np.iinfo(pg.NP_DTYPE[dtype])
    return rng.integers(info.min, info.max, n, dtype=pg.NP_DTYPE[dtype], endpoint=True)


# ------------------------------------------------------------------------------------ accepts
@pytest.mark.parametrize("dtype", [I32, I64, F64])
@pytest.mark.parametrize("n,null_frac", GRID)
def test_accepts_pack_fixed(dtype, n, null_frac):
    rng = np.random.default_rng(n * 7 + dtype)
    vals = fixed_values(rng, dtype, n)
    valid = rng.random(n) >= null_frac
    for pages in (pg.pack_fixed(vals, valid, dtype), _oracle.encode_fixed(dtype, vals, valid).pages):
        v, m = check_column(pl.Column(dtype, pages), n)
        assert np.array_equal(m, valid)
        assert v[valid].tobytes() == vals[valid].tobytes()
        assert not v[~valid].view(np.uint8).any()
        accept_table(pl.ColumnarTable(n, [pl.Column(dtype, pages)]))


def test_accepts_pack_varchar():
    rng = np.random.default_rng(3)
    strings = []
    for i in range(600):
        r = rng.random()
        if r < 0.15:
            strings.append(None)
        elif r < 0.17:
            strings.append(bytes(rng.integers(97, 123, int(rng.integers(8186, 30000)), dtype=np.uint8)))
        else:
            strings.append(bytes(rng.integers(32, 127, int(rng.integers(0, 200)), dtype=np.uint8)))
    strings += [b"", None, b"x" * 8185, b"y" * 8186, b"z" * 8188, b"w" * 8189]
    for pages in (pg.pack_varchar(strings), _oracle.encode_varchar(strings).pages):
        assert check_column(pl.Column(VC, pages), len(strings)) == strings
    for strs in ([], [None], [b""], [None] * 70_000, [b""] * 5_000, [b"q" * 8185] * 3, [b"L" * (3 * 8188)]):
        assert check_column(pl.Column(VC, pg.pack_varchar(strs)), len(strs)) == strs


@pytest.mark.parametrize("n,digits,prefix", [(0, 10, b""), (1, 1, b""), (703, 10, b""), (704, 10, b"tt"), (20_000, 7, b"name-"), (5, 4000, b"x")])
def test_accepts_pack_varchar_fixed(n, digits, prefix):
    codes = np.arange(n, dtype=np.uint64) * 977
    t = pl.ColumnarTable(n, [pl.Column(VC, pg.pack_varchar_fixed(codes, digits, prefix))])
    got = accept_table(t)[0]
    assert got == [prefix + (b"%0*d" % (digits, int(c) % 10**digits)) for c in codes]


def test_accepts_the_oracle_on_the_golden_unit_cases():
    cases = _golden.load_cases()
    assert cases
    for case in cases:
        p = _golden.build_plan(case)
        for t in p.inputs:
            accept_table(t, case.get("name"))
        accept_table(_oracle.execute(p), case.get("name"))


def test_accepts_the_oracle_and_the_references_on_generated_plans():
    # the C oracle runs scans and inner joins: the random plans of tests/test_gpu_fuzz.py, and the
    # plans of the mixed generator that hold nothing else; every mixed plan's inputs and numpy
    # reference result (packed by pyrj.pages) pass as well
    n_cols = 0
    for seed in range(20):
        res = _oracle.execute(fz.random_plan(seed))
        n_cols += len(accept_table(res, ("fuzz", seed)))
    for seed in range(20):
        p = mr.plan_of("small", seed)
        for t in p.inputs:
            accept_table(t, ("mixed input", seed))
        accept_table(_aggref.execute(p), ("mixed ref", seed))
    inner = [s for s in mr.SMALL if set(mr.kinds_of("small", s)) <= {"scan", "join"}]
    for seed in inner:
        accept_table(_oracle.execute(mr.plan_of("small", seed)), ("mixed oracle", seed))
    assert n_cols >= 20 and len(inner) >= 3, (n_cols, inner)


@pytest.mark.parametrize("seed", range(6))
def test_the_oracle_s_csv_tables(seed):
    """NULLs, long strings; INT64 / FP64 columns too: a page the reference's inserter clobbered breaks
    `fit` and no other page does."""
    rng = np.random.default_rng(100 + seed)
    types = [[I32, VC, I64], [VC, I32], [I32, I32, VC, VC], [I64, I32], [F64, I32], [VC, F64, F64]][seed]
    n = int(rng.integers(3000, 9000))
    rows = g.random_rows(rng, n, types, null_p=0.15, long_p=0.003)
    t = _oracle.from_csv(g.to_csv(rng, rows), types)
    assert t.num_rows == n
    clobbered = {ci for _, ci in io.clobbered_cells(t)}
    for ci, c in enumerate(t.columns):
        one = pl.ColumnarTable(n, [c])
        if ci in clobbered:
            with pytest.raises(PageFormatError) as e:
                check_column(c, n)
            assert e.value.rule_name == "fit"
        else:
            accept_table(one, (seed, ci))
    if VC in types:
        hdr = np.concatenate([c.pages[:, :2].copy().view(np.uint16)[:, 0] for c in t.columns if c.type == VC])
        assert (hdr == 0xFFFF).any() and (hdr == 0xFFFE).any()


def test_the_inserter_s_clobbered_page_is_the_one_named():
    # k NULL rows, then values: the inserter lets value m in while 8 * m + 5 + (k + m - 1) / 8 <= 8192,
    # and value m reaches into the bitmap when 8 * m + 8 + ceil((k + m) / 8) > 8192.  For m = 1007
    # both hold with 18 <= k <= 49.
    k, m = 20, 1007
    assert 8 * m + 5 + (k + m - 1) // 8 <= PS < 8 * m + 8 + -(-(k + m) // 8)
    text = b"\n".join([b","] * k + [b"%d,1" % i for i in range(1, 3000)]) + b"\n"
    t = _oracle.from_csv(text, [I64, I32])
    assert t.num_rows == k + 2999
    cells = io.clobbered_cells(t)
    assert cells and {ci for _, ci in cells} == {0}
    with pytest.raises(PageFormatError) as e:
        check_column(t.columns[0], t.num_rows)
    assert e.value.rule_name == "fit" and e.value.page_index == 0
    accept_table(pl.ColumnarTable(t.num_rows, [t.columns[1]]))


def test_empty_pages_are_legal_and_counted():
    vals = np.arange(3000, dtype=np.int32)
    valid = vals % 3 != 0
    pages = pg.pack_fixed(vals, valid, I32)
    blank = np.zeros((1, PS), np.uint8)
    with_blank = np.concatenate([blank, pages[:1], blank, blank, pages[1:]])
    (v, m), empty = pc.scan_column(pl.Column(I32, with_blank), 3000)
    assert empty == 3 and np.array_equal(m, valid) and np.array_equal(v[valid], vals[valid])
    assert pc.scan_column(pl.Column(I32, pages), 3000)[1] == 0
    strs = [b"a", None, b"bcd"]
    vp = pg.pack_varchar(strs)
    got, empty = pc.scan_column(pl.Column(VC, np.concatenate([vp, blank])), 3)
    assert got == strs and empty == 1
    # a column of nothing but empty pages is a table of no rows
    assert pc.scan_column(pl.Column(I64, np.concatenate([blank, blank])), 0)[1] == 2


def test_unspecified_bytes_are_not_checked():
    vals = np.arange(11, dtype=np.int64)
    valid = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1], bool)
    pages = pg.pack_fixed(vals, valid, I64)
    pages[0, PS - 1] |= 0xF8                      # bits above nr = 11 in the last bitmap byte
    pages[0, 8 + 8 * 8: PS - 2] = 0xAB            # between the values and the bitmap
    pages[0, 4:8] = 0xCD                          # the header's padding of an 8-byte column
    v, m = check_column(pl.Column(I64, pages), 11)
    assert np.array_equal(m, valid) and np.array_equal(v[valid], vals[valid])
    vp = pg.pack_varchar([b"ab", None, b"c"])
    vp[0, 4 + 4 + 3: PS - 1] = 0xEE
    vp[0, PS - 1] |= 0xF8
    assert check_column(pl.Column(VC, vp), 3) == [b"ab", None, b"c"]


def test_a_million_rows_in_well_under_a_second():
    rng = np.random.default_rng(1)
    n = 1_000_000
    vals = rng.integers(-2**62, 2**62, n)
    valid = rng.random(n) >= 0.2
    cols = [pl.Column(I64, pg.pack_fixed(vals, valid, I64)), pl.Column(I32, pg.pack_fixed(vals.astype(np.int32), None, I32))]
    for c in cols:
        dt = float("inf")
        for _ in range(4):  # the best of four: what the reader needs, not what else the machine does
            t0 = time.perf_counter()
            v, m = check_column(c, n)
            dt = min(dt, time.perf_counter() - t0)
        print(f"check_column, 1 M rows of type {c.type}: {dt * 1e3:.0f} ms over {c.pages.shape[0]} pages")
        assert dt < 1.0, dt
    assert np.array_equal(m, np.ones(n, bool))


# ------------------------------------------------------------------------------------ rejects
def u16(page, at):
    return int(page[at]) | int(page[at + 1]) << 8


def put16(page, at, v):
    page[at], page[at + 1] = v & 0xFF, v >> 8


def ones_bitmap(page, nr):
    nb = (nr + 7) // 8
    page[PS - nb:] = 0xFF
    if nr % 8:
        page[PS - 1] = (1 << (nr % 8)) - 1


def small_fixed(dtype=I32):
    """10 rows, NULL at rows 3 and 9"""
    valid = np.ones(10, bool)
    valid[[3, 9]] = False
    return pg.pack_fixed(np.arange(10), valid, dtype), 10


def m_fixed_nnn(delta, dtype=I32):
    def make():
        pages, n = small_fixed(dtype)
        put16(pages[0], 2, 8 + delta)
        return dtype, pages, n
    return make


def m_varchar_nnn(delta):
    def make():
        pages = pg.pack_varchar([b"a", None, b"bc", b""])
        put16(pages[0], 2, 3 + delta)
        return VC, pages, 4
    return make


def m_overlap_full(dtype):
    def make():
        rf = pg.rows_per_full_page(dtype)
        pages = pg.pack_fixed(np.arange(rf), None, dtype)
        nr = rf + 8  # one more bitmap byte and eight more values than the page has room for
        put16(pages[0], 0, nr)
        put16(pages[0], 2, nr)
        ones_bitmap(pages[0], nr)
        return dtype, pages, nr
    return make


def m_overlap_by_one_byte():
    # 1984 values and then NULL rows up to the last bit of room: 4 + 7936 + 252 = 8192.  One row more
    # and the bitmap starts on the last byte of the last value (a zero byte here, so that the count of
    # set bits still agrees with the header: only `fit` is broken)
    valid = np.concatenate([np.ones(1984, bool), np.zeros(32, bool)])
    pages = pg.pack_fixed(np.arange(2016), valid, I32)
    assert pages.shape[0] == 1 and u16(pages[0], 0) == 2016 and pages[0, 4 + 7936 - 1] == 0
    put16(pages[0], 0, 2017)
    return I32, pages, 2017


def m_rows(dtype, header_delta, declared_delta):
    """the last page's row count changed (the row that comes or goes is NULL), or num_rows"""
    def make():
        if dtype == VC:
            pages, n = pg.pack_varchar([b"k%d" % i for i in range(3000)] + [b"z", None]), 3002
        else:
            valid = np.ones(3002, bool)
            valid[-1] = False
            pages, n = pg.pack_fixed(np.arange(3002), valid, dtype), 3002
        last = pages[-1]
        nr = u16(last, 0)
        assert (nr + header_delta + 7) // 8 == (nr + 7) // 8  # the bitmap stays where it is
        put16(last, 0, nr + header_delta)
        return dtype, pages, n + declared_delta
    return make


def m_descending_offset():
    pages = pg.pack_varchar([b"aaa", b"bb", b"c"])
    assert [u16(pages[0], 4 + 2 * k) for k in range(3)] == [3, 5, 6]
    put16(pages[0], 6, 2)
    return VC, pages, 3


def m_offset_into_bitmap():
    pages = pg.pack_varchar([b"abc"])
    put16(pages[0], 4, PS - 4 - 2 - 1 + 1)  # 4 + 2 + 8186 + 1 = 8193
    return VC, pages, 1


def m_offsets_alone_reach_the_bitmap():
    # an all-NULL page of 32 768 rows has 4096 bitmap bytes; claim as many values as set bits: the
    # offset array alone (2 * 4000 bytes) then overlaps the bitmap
    pages = pg.pack_varchar([None] * 32_768)
    assert pages.shape[0] == 1
    pages[0, PS - 4096: PS - 4096 + 500] = 0xFF
    put16(pages[0], 2, 4000)
    return VC, pages, 32_768


def long_pages(n_chars):
    pages = pg.pack_varchar([b"x" * n_chars])
    assert u16(pages[0], 0) == 0xFFFF and all(u16(p, 0) == 0xFFFE for p in pages[1:])
    return pages


def m_orphan_first():
    return VC, long_pages(9000)[1:], 0


def m_orphan_behind_a_normal_page():
    return VC, np.concatenate([pg.pack_varchar([b"short", None]), long_pages(9000)[1:]]), 2


def m_long_length(v, page=0):
    def make():
        pages = long_pages(2 * 8188 + 5)
        put16(pages[page], 2, v)
        return VC, pages, 1
    return make


def m_short_piece(page):
    def make():
        pages = long_pages(2 * 8188 + 5)
        assert pages.shape[0] == 3
        put16(pages[page], 2, 8187)
        return VC, pages, 1
    return make


def m_short_chain(n_chars):
    def make():
        pages = long_pages(8186)[:1].copy()
        put16(pages[0], 2, n_chars)
        return VC, np.concatenate([pages, pg.pack_varchar([b"next"])]), 2
    return make


def m_row_limit(dtype):
    def make():
        if dtype == VC:
            pages = pg.pack_varchar([None] * 65_504)
        else:
            pages = pg.pack_fixed(np.zeros(65_504), np.zeros(65_504, bool), dtype)
            assert pages.shape[0] == (1 if dtype == I32 else 2)
            pages = pages[:1]
        put16(pages[0], 0, 65_505)
        return dtype, pages, 65_505
    return make


# (id, the rule that must be named, the page that must be named, mutation)
REJECTS = [
    ("fixed-nnn-plus-one", "nnn_popcount", 0, m_fixed_nnn(+1)),
    ("fixed-nnn-minus-one", "nnn_popcount", 0, m_fixed_nnn(-1)),
    ("fixed64-nnn-plus-one", "nnn_popcount", 0, m_fixed_nnn(+1, F64)),
    ("varchar-nnn-plus-one", "nnn_popcount", 0, m_varchar_nnn(+1)),
    ("varchar-nnn-minus-one", "nnn_popcount", 0, m_varchar_nnn(-1)),
    ("int32-values-overlap-bitmap", "fit", 0, m_overlap_full(I32)),
    ("int64-values-overlap-bitmap", "fit", 0, m_overlap_full(I64)),
    ("bitmap-starts-on-the-last-value-byte", "fit", 0, m_overlap_by_one_byte),
    ("int32-last-page-short-by-one", "row_total", 1, m_rows(I32, -1, 0)),
    ("int32-last-page-long-by-one", "row_total", 1, m_rows(I32, +1, 0)),
    ("int64-last-page-short-by-one", "row_total", 2, m_rows(I64, -1, 0)),
    ("fp64-last-page-long-by-one", "row_total", 2, m_rows(F64, +1, 0)),
    ("int32-table-declares-one-more", "row_total", 1, m_rows(I32, 0, +1)),
    ("int32-table-declares-one-less", "row_total", 1, m_rows(I32, 0, -1)),
    ("varchar-last-page-short-by-one", "row_total", None, m_rows(VC, -1, 0)),
    ("varchar-last-page-long-by-one", "row_total", None, m_rows(VC, +1, 0)),
    ("varchar-table-declares-one-more", "row_total", None, m_rows(VC, 0, +1)),
    ("descending-offset", "offsets_ordered", 0, m_descending_offset),
    ("last-offset-reaches-into-the-bitmap", "fit", 0, m_offset_into_bitmap),
    ("offset-array-reaches-into-the-bitmap", "fit", 0, m_offsets_alone_reach_the_bitmap),
    ("fffe-first-in-the-column", "long_orphan", 0, m_orphan_first),
    ("fffe-behind-a-normal-page", "long_orphan", 1, m_orphan_behind_a_normal_page),
    ("long-length-0", "long_length", 0, m_long_length(0)),
    ("long-length-8189", "long_length", 0, m_long_length(8189)),
    ("continuation-length-0", "long_length", 2, m_long_length(0, page=2)),
    ("continuation-length-8189", "long_length", 1, m_long_length(8189, page=1)),
    ("short-middle-piece", "long_piece", 1, m_short_piece(1)),
    ("short-first-piece", "long_piece", 0, m_short_piece(0)),
    ("chain-of-8185-characters", "long_total", 0, m_short_chain(8185)),
    ("chain-of-1-character", "long_total", 0, m_short_chain(1)),
    ("int32-65505-rows", "row_limit", 0, m_row_limit(I32)),
    ("int64-65505-rows", "row_limit", 0, m_row_limit(I64)),
    ("varchar-65505-rows", "row_limit", 0, m_row_limit(VC)),
]


@pytest.mark.parametrize("name,rule,page,make", REJECTS, ids=[r[0] for r in REJECTS])
def test_rejects(name, rule, page, make):
    dtype, pages, n = make()
    with pytest.raises(PageFormatError) as e:
        check_column(pl.Column(dtype, pages), n)
    assert e.value.rule_name == rule, str(e.value)
    if page is not None:
        assert e.value.page_index == page, str(e.value)
    assert e.value.args[0].startswith(f"page {e.value.page_index}: rule {rule}")


def test_every_rule_has_a_rejecting_case():
    assert {r[1] for r in REJECTS} == set(pc.RULES)


def test_the_unmutated_pages_pass():
    """the mutations start from pages the reader accepts, and stop being rejected at the boundary"""
    pages, n = small_fixed()
    check_column(pl.Column(I32, pages), n)
    vp = pg.pack_varchar([b"abc"])
    put16(vp[0], 4, PS - 4 - 2 - 1)  # 4 + 2 + 8185 + 1 = 8192: legal, whatever the characters are
    assert len(check_column(pl.Column(VC, vp), 1)[0]) == 8185
    lp = long_pages(8186)
    assert check_column(pl.Column(VC, lp), 1) == [b"x" * 8186]
    lp3 = long_pages(2 * 8188 + 5)
    assert check_column(pl.Column(VC, lp3), 1) == [b"x" * (2 * 8188 + 5)]
    full = pg.pack_fixed(np.zeros(65_504), np.zeros(65_504, bool), I32)
    assert full.shape[0] == 1 and not check_column(pl.Column(I32, full), 65_504)[1].any()
    # an all-NULL VARCHAR page of 65 504 rows, and 1984 values + 32 NULL rows: both exactly full
    assert check_column(pl.Column(VC, pg.pack_varchar([None] * 65_504)), 65_504) == [None] * 65_504
    valid = np.concatenate([np.ones(1984, bool), np.zeros(32, bool)])
    assert check_column(pl.Column(I32, pg.pack_fixed(np.arange(2016), valid, I32)), 2016)[1].sum() == 1984
