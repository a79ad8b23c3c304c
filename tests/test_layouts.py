"""tests/_layouts.py pinned on the CPU: every layout it makes is a legal column (the strict reader
tests/_pagecheck.py), decodes to the logical column with pyrj.pages as well, and means the same to the C
oracle as the canonical packing of the column, in a join and in a root scan.  tests/test_gpu_layouts.py
feeds these layouts to the library."""
import numpy as np
import pytest

import _layouts as lo
import _oracle
import _pagecheck as pc
from pyrj import pages as pg
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
FIXED = [I32, I64, F64]
SEEDS = [0, 1, 2]


def words(n, seed=0, nulls=True):
    """short strings of mixed lengths: about 150 rows per page"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        r = rng.random()
        if nulls and r < 0.07:
            out.append(None)
        elif r < 0.1:
            out.append(b"")
        else:
            out.append((b"r%d:" % i) + b"y" * int(rng.integers(0, 90)))
    return out


def fixed_col(name, dt, seed):
    n = lo.fixed_rows(name, dt)
    valid = lo.fixed_valid(name, dt, n, seed)
    if valid is None and seed:  # the layouts that need no NULLs take a few all the same
        valid = np.random.default_rng(seed).random(n) > 0.03
    vals = lo.typed(dt, np.random.default_rng(seed + 50).integers(0, 3000, n))
    return lo.Col(dt, vals, valid, name, seed)


# ------------------------------------------------------------------------------- the helper itself
def test_capacities_and_branches():
    assert (lo.rows_full(I32), lo.rows_full(I64), lo.rows_full(F64)) == (1984, 1007, 1007)
    assert (lo.max_null_rows(I32), lo.max_null_rows(I64)) == (65_504, 65_472) and pc.MAX_ROWS == 65_504
    assert [(dt, nr, lo.bitmap_branch(nr)) for dt, nr, _ in lo.SINGLE_NULL_SHAPES] == list(lo.SINGLE_NULL_SHAPES)
    assert {b for _, _, b in lo.SINGLE_NULL_SHAPES} == {"dword", "halfword", "byte"}
    assert lo.single_null_positions(I32, 1984) == [0, 1, 7, 8, 15, 16, 31, 32, 63, 64, 255, 256, 1967, 1968, 1975, 1976, 1983]
    assert lo.single_null_positions(I32, 20) == [0, 1, 3, 4, 7, 8, 11, 12, 15, 16, 19]


@pytest.mark.parametrize("dt", FIXED)
@pytest.mark.parametrize("name", sorted(lo.LAYOUTS))
def test_fixed_layout_shapes(name, dt):
    """what each name promises about its cuts"""
    n, cap = lo.fixed_rows(name, dt), lo.rows_full(dt)
    valid = lo.fixed_valid(name, dt, n)
    cuts = lo.LAYOUTS[name](n, dt, valid, 3)
    assert sum(cuts) == n
    if name not in ("one_row_per_page", "all_null_max", "random_cuts"):
        assert 2 <= len([c for c in cuts if c]) <= 7, cuts
    full = [c for c in cuts if c == cap]
    if name == "canonical":
        assert lo.is_regular(cuts, valid, dt, n)
    else:
        assert not lo.is_regular(cuts, valid, dt, n)
    if name == "one_short_middle":
        assert cuts[1] == cap - 1 and len(full) == len(cuts) - 2 and cuts[-1] < cap
    if name == "last_exactly_full":
        assert cuts[-1] == cap and cuts[0] < cap and full == cuts[1:]
    if name == "last_one_row":
        assert cuts[-1] == 1
    if name == "last_empty":
        assert cuts[-1] == 0 and cuts[-2] > 0
    if name == "empty_first":
        assert cuts[0] == 0
    if name == "empty_middle_twice":
        assert cuts[1:3] == [0, 0] and cuts[0] and cuts[3]
    if name == "one_row_per_page":
        assert cuts == [1] * n
    if name == "random_cuts":
        assert 0 in cuts and all(c <= cap for c in cuts) and cuts != lo.LAYOUTS[name](n, dt, valid, 4)
    if name == "overfull_with_nulls":
        assert cuts[0] > cap and cuts[1] == 7 and max(cuts[2:]) > cap
    if name == "all_null_max":
        assert cuts == [cap, lo.max_null_rows(dt), cap]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dt", FIXED)
@pytest.mark.parametrize("name", sorted(lo.LAYOUTS))
def test_fixed_layouts_are_legal_and_decode_to_the_column(name, dt, seed):
    c = fixed_col(name, dt, seed)
    n = len(c)
    col = c.cut_column()  # asserts check_column == the logical column
    vals, valid = pg.unpack_fixed(col.pages, n, dt)
    m = np.ones(n, bool) if c.valid is None else c.valid
    assert np.array_equal(valid, m) and vals[m].tobytes() == np.ascontiguousarray(c.values[m]).tobytes()
    ovals, ovalid = _oracle.decode_fixed(col, n)
    assert np.array_equal(ovalid, m) and ovals[m].tobytes() == vals[m].tobytes()
    _, empty = pc.scan_column(col, n)
    assert empty == c.cuts.count(0)
    # the scribbled regions really differ from what the packer leaves there, and only there
    plain = lo.cut_fixed(c.values, c.valid, dt, c.cuts)
    assert pc.same_as([pc.check_column(pl.Column(dt, plain), n)], [pc.check_column(col, n)])
    assert not np.array_equal(plain, col.pages)
    assert np.array_equal(plain[:, :4], col.pages[:, :4])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", lo.VARCHAR_LAYOUTS)
def test_varchar_layouts_are_legal_and_decode_to_the_column(name, seed):
    c = lo.Col(VC, words(400, seed), None, name, seed)
    n = len(c)
    col = c.cut_column()
    assert pg.unpack_varchar(col.pages, n) == c.values
    assert _oracle.decode_varchar(col, n) == c.values
    hdr = col.pages[:, :2].copy().view(np.uint16)[:, 0]
    chains = int((hdr == 0xFFFF).sum())
    assert chains == {"two_chains_adjacent": 2}.get(name, 1 if name in lo.VARCHAR_ONLY else 0)
    if name in lo.VARCHAR_ONLY:
        assert (hdr == 0xFFFE).any()
    if name == "chain_first":
        assert hdr[0] == 0xFFFF
    if name == "chain_last":
        assert hdr[-3:].tolist() == [0xFFFF, 0xFFFE, 0xFFFE]
    if name == "chain_between_empty_pages":
        k = int(np.nonzero(hdr == 0xFFFF)[0][0])
        assert hdr[k - 1] == 0 and hdr[k + 1] == 0xFFFE and hdr[k + 2] == 0
    if name == "two_chains_adjacent":
        a, b = np.nonzero(hdr == 0xFFFF)[0]
        assert b == a + 2 and hdr[a + 1] == 0xFFFE
    if name == "chain_then_one_row_page":
        k = int(np.nonzero(hdr == 0xFFFF)[0][0])
        assert hdr[k + 2] == 1
    assert pc.scan_column(col, n)[1] == c.cuts.count(0)
    spans = lo.page_first_last_rows(col)
    assert spans[0][0] == 0 and spans[-1][1] == n - 1 and all(a[1] + 1 == b[0] for a, b in zip(spans, spans[1:]))


def test_a_cut_that_does_not_fit_is_refused():
    with pytest.raises(AssertionError):
        lo.cut_fixed(np.arange(2000, dtype=np.int32), None, I32, [1985, 15])
    with pytest.raises(AssertionError):
        lo.cut_varchar([b"x" * 5000, b"y" * 5000], [2])
    with pytest.raises(AssertionError):
        lo.cut_varchar([lo.long_string(b"a"), b"b"], [2])


# ------------------------------------------------------------------------------- the oracle's view
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dt", FIXED)
@pytest.mark.parametrize("name", sorted(lo.LAYOUTS))
def test_oracle_joins_a_cut_column_like_the_canonical_one(name, dt, seed):
    p, p0, _ = lo.layout_join_case(name, dt, seed)
    got, want = _oracle.execute(p), _oracle.execute(p0)
    assert got.num_rows == want.num_rows > 0
    assert pl.canonical_rows(got) == pl.canonical_rows(want)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", lo.VARCHAR_LAYOUTS)
def test_oracle_joins_a_cut_varchar_column_like_the_canonical_one(name, seed):
    """the cut column as join key and, a second column of other strings in the same layout, as payload;
    the other side's key holds the strings at the edges of the cut pages, every chain, misses and NULLs,
    cut at random"""
    key = lo.Col(VC, words(400, seed + 30), None, name, seed)
    pay = lo.Col(VC, [None if s is None else b"p:" + s[:60] for s in words(400, seed + 40)], None, name, seed)
    n = len(key)
    assert len(pay) == n
    left, left0 = lo.tables([key, pay, lo.Col(I32, np.arange(n, dtype=np.int32), None, "last_one_row")])
    rng = np.random.default_rng(seed + 60)
    edges = {r for a, b in lo.page_first_last_rows(left.columns[0]) for r in (a, b)}
    long_pay = [r for r, v in enumerate(pay.values) if v is not None and len(v) > pc.MAX_INLINE]  # the payload's chains
    pool = [key.values[r] for r in sorted(edges) + long_pay] + [key.values[int(i)] for i in rng.integers(0, n, 300)]
    pool += [b"miss%d:" % i + b"z" * (i % 70) for i in range(200)] + [None] * 10 + [lo.long_string(b"nobody")]
    other = lo.Col(VC, [pool[int(i)] for i in rng.permutation(len(pool))], None, "random_cuts", seed + 1)
    right, right0 = lo.tables([other, lo.Col(I64, np.arange(len(other), dtype=np.int64), None)])
    for build_left in (True, False):
        p = lo.join_plan(left, right, build_left=build_left)
        got, want = _oracle.execute(p), _oracle.execute(lo.with_inputs(p, [left0, right0]))
        assert got.num_rows == want.num_rows > len(edges) // 2
        rows = pl.canonical_rows(got)
        assert rows == pl.canonical_rows(want)
        if name in lo.VARCHAR_ONLY:  # the key's chains met their partners; the payload's came along with their rows
            assert any(len(r[0]) > pc.MAX_INLINE for r in rows)
            if any(key.values[r] is not None for r in long_pay):
                assert any(r[1] is not None and len(r[1]) > pc.MAX_INLINE for r in rows)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name,dt", [(n, dt) for dt in FIXED for n in sorted(lo.LAYOUTS)] + [(n, VC) for n in lo.VARCHAR_LAYOUTS])
def test_oracle_root_scan_of_a_cut_column(name, dt, seed):
    cols = [lo.Col(VC, words(400, seed + 5), None, name, seed)] if dt == VC else [fixed_col(name, dt, seed)]
    cut, canon = lo.tables(cols)
    got, want = _oracle.execute(lo.scan_plan(cut)), _oracle.execute(lo.scan_plan(canon))
    assert got.num_rows == want.num_rows == len(cols[0])
    assert pc.strict_rows(got) == pl.canonical_rows(want)


@pytest.mark.parametrize("dt", FIXED + [VC])
def test_oracle_reads_rows_the_pages_do_not_cover_as_null(dt):
    """pages of n rows under num_rows = n + 10: ten NULL rows at the end, in a join and in a root scan,
    whose result the oracle encodes at n + 10 rows"""
    n = 2 * lo.rows_full(I32) + 50
    key = lo.Col(I32, np.arange(n + 10, dtype=np.int32), None, cuts=lo.one_short_middle(n + 10, I32, None))
    if dt == VC:
        strs = words(n, 9, nulls=False)
        col = lo.Col(VC, strs + [None] * 10, cuts=lo._vc_greedy(strs, 0, n))
    else:
        col = lo.Col(dt, lo.typed(dt, np.arange(n + 10)), np.arange(n + 10) < n, cuts=lo.random_cuts(n, dt, None, 7))
    assert sum(col.cuts) == n
    t = pl.ColumnarTable(n + 10, [key.cut_column(), col.cut_column()])
    canon = pl.make_table([key.canonical_spec(), col.canonical_spec()])
    with pytest.raises(pc.PageFormatError) as e:
        pc.check_column(t.columns[1], n + 10)
    assert e.value.rule_name == "row_total"
    got = _oracle.execute(lo.scan_plan(t))
    assert got.num_rows == n + 10
    rows = pc.strict_rows(got)
    assert rows == pl.canonical_rows(_oracle.execute(lo.scan_plan(canon)))
    assert sum(r[1] is None for r in rows) == 10 and all(r[1] is None for r in rows if r[0] >= n)
    other = pl.make_table([(I32, np.arange(n - 5, n + 10, dtype=np.int32))])
    j = lo.join_plan(t, other, 0, 0, build_left=False)
    rows = pl.canonical_rows(_oracle.execute(j))
    assert len(rows) == 15 and rows == pl.canonical_rows(_oracle.execute(lo.with_inputs(j, [canon, other])))
    assert [r[1] is None for r in rows] == [False] * 5 + [True] * 10
