"""One logical column, many legal paginations: the result must not depend on how an input column is cut
into pages.

tests/_layouts.py re-paginates a column (short pages anywhere, pages with nr == 0, pages that NULLs let
hold more rows than a full page, one all-NULL page of 65 504 rows, long-string chains between any of
these, 0xA5 in every byte and bit the format leaves unspecified); tests/test_layouts.py pins it on the
CPU.  Here those columns go to the six places that read input pages:
  1. the header walk of an upload (table_fill / bitmap_all_ones, csrc/rj_table.hip),
  2. host_column_regular, which gates the row cuts of rj_execute on several devices,
  3. k_page_headers / k_rows_beyond / k_scan_bins<0> behind rj_table_adopt_device,
  4. k_decode_pages<4|8> (K1),
  5. the host VARCHAR directory and gather (csrc/rj_varchar.cpp),
  6. vc_resolve_row behind k_vc_resolve and k_vc_hash (csrc/rj_varchar_dev.hip).
The expected value is always the reference result of the plan over the CANONICAL packing of the same
columns (the C oracle for inner joins and scans, tests/_selectref.py, which evaluates every node kind,
for the others), compared row-exact; every result column goes through the strict reader.  Every column
is proven legal (check_column, in _layouts.column / varchar_column) before it reaches the library; the
two error cases at the end are the only pages that are not."""
import numpy as np
import pytest

import _layouts as lo
import _oracle
import _pagecheck as pc
import _selectref
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import pages as pg
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
FIXED = [I32, I64, F64]
TN = {I32: "i32", I64: "i64", F64: "f64", VC: "vc"}
VDEV = {"RJ_TUNE_VARCHAR_DEV": "1"}  # every VARCHAR result column is gathered and encoded on the device
KEY, STAR, COUNT, SUM, MIN = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN

# ------------------------------------------------------------------------------------ running
_contexts = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _contexts.values():
        c.destroy()
    _contexts.clear()


def context(env=None, **kw):
    """one context per configuration, shared by the cases (the launch log is cleared for each run)"""
    key = (tuple(sorted((env or {}).items())), tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _contexts:
        _contexts[key] = fm.tuned_context(env or {}, **kw)
    return _contexts[key]


def all_fixed(p):
    return all(c.type != VC for t in p.inputs for c in t.columns)


def run(p, path="host", env=None, **kw):
    """-> (result table, {kernel: launches}) of the plan through one entry path: host pages through
    rj_execute, rj_table_upload + rj_execute_resident, or rj_table_adopt_device of torch tensors"""
    c = context(env, **kw)
    c.launch_log(True)
    try:
        if path == "host":
            got = capi.execute(p, c)
        else:
            keep, tabs = [], []
            try:
                for t in p.inputs:
                    if path == "upload":
                        tabs.append(c.upload(t))
                    else:
                        import torch

                        dev = [torch.from_numpy(np.ascontiguousarray(col.pages).reshape(-1, pg.PAGE_SIZE).copy()).cuda() for col in t.columns]
                        keep.append(dev)
                        tabs.append(c.adopt_device(t.num_rows, [col.type for col in t.columns], [d.data_ptr() if d.shape[0] else None for d in dev],
                                                   [d.shape[0] for d in dev], keep=dev))
                res = c.execute_resident(p, tabs)
                try:
                    got = res.to_table()
                finally:
                    res.free()
            finally:
                for t in tabs:
                    t.release()
        ran = km.launched(c)
    finally:
        c.launch_log(False)
    return got, ran


def launches(ran, family):
    return sum(n for name, n in ran.items() if name.split("<")[0] == family)


def strict(got, want, what=""):
    """the format of every result column, then the rows"""
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    rows = pc.strict_rows(got)
    assert rows == pl.canonical_rows(want), what
    return rows


def paths_of(p):
    return ("host", "upload", "adopt") if all_fixed(p) else ("host", "upload")


def irregular(cols, num_rows=None):
    return sum(1 for c in cols if c.dtype != VC and not c.regular(len(c) if num_rows is None else num_rows))


# ------------------------------------------------- 1. every layout x every entry path x both roles
@pytest.mark.parametrize("dt", FIXED, ids=[TN[d] for d in FIXED])
@pytest.mark.parametrize("name", sorted(lo.LAYOUTS))
def test_layout_as_join_key_and_payload(name, dt):
    """The probe side's key and payload are cut with the layout, the build side's payload too; every
    other column with another layout, so that the row bases differ from column to column.  Through the
    broadcast join (4000 build rows) and a forced two-pass plan, by all three entry paths, each pinned
    by the launch log.  K1 runs once for every column that cannot be addressed in place, and not at all
    for the canonical control."""
    p, p0, (build, probe) = lo.layout_join_case(name, dt)
    want = _oracle.execute(p0)
    assert want.num_rows > 500
    k1 = irregular(build) + irregular(probe)
    assert (k1 == 0) == (name == "canonical")
    for bits in (0, 12):
        for path in paths_of(p):
            got, ran = run(p, path, radix_bits=bits)
            what = (name, TN[dt], bits, path)
            print(what, "rows", got.num_rows, "decode_pages", launches(ran, "k_decode_pages"), "expected", k1)
            strict(got, want, what)
            assert launches(ran, "k_decode_pages") == k1, (what, sorted(ran))
            if path == "adopt":
                assert launches(ran, "k_page_headers") == 6, (what, sorted(ran))
            # the two settings really are two join paths: the broadcast kernel and no radix pass, or the
            # partitioned join behind two scatter passes over each side
            scatters = launches(ran, "k_pass_scatter") + launches(ran, "k_pass_scatter_packed")
            if bits == 0:
                assert launches(ran, "k_join_bcast") > 0 and launches(ran, "k_join") == 0 and scatters == 0, (what, sorted(ran))
            else:
                assert launches(ran, "k_join") > 0 and launches(ran, "k_join_bcast") == 0 and scatters >= 4, (what, sorted(ran.items()))


# ------------------------------------------------------------- 2. one cleared bit, and none
def single_null_table(dt, nr, key_null, pay_null, garbage=True):
    """pages [full, nr] of a key and of a payload column, each all valid but for one row of the last
    page (None: none), and row ids; -> (cut table, canonical table, the columns)"""
    cap = lo.rows_full(dt)
    n = cap + nr

    def valid(at):
        v = np.ones(n, bool)
        if at is not None:
            v[cap + at] = False
        return v if at is not None else None

    cols = [lo.Col(dt, lo.typed(dt, np.arange(n)), valid(key_null), cuts=[cap, nr]),
            lo.Col(dt, lo.typed(dt, np.arange(n) + 5), valid(pay_null), cuts=[cap, nr]),
            lo.Col(I32, np.arange(n, dtype=np.int32), None)]
    cut = pl.ColumnarTable(n, [lo.column(c.values, c.valid, c.dtype, c.cuts, garbage=garbage) for c in cols])
    return cut, pl.make_table([c.canonical_spec() for c in cols]), cols


@pytest.mark.parametrize("dt,nr,branch", lo.SINGLE_NULL_SHAPES, ids=["%s-%d-%s" % (TN[d], n, b) for d, n, b in lo.SINGLE_NULL_SHAPES])
def test_single_cleared_bit_flips_regular(dt, nr, branch):
    """A column that is all valid except ONE bit: "regular" must flip on exactly that bit, wherever in
    the bitmap it sits.  The row is NULL: as a key it matches nothing, as a payload it comes out NULL.
    (A 1001-row page has 126 bitmap bytes at an even offset and so takes k_page_headers' halfword
    loads like the 1007-row one; the 999-row page, 125 bytes, is the one that goes byte by byte.)"""
    assert lo.bitmap_branch(nr) == branch
    cap = lo.rows_full(dt)
    n = cap + nr
    other = pl.make_table([(dt, lo.typed(dt, np.arange(n))), (I32, np.arange(n, dtype=np.int32))])
    pos = lo.single_null_positions(dt, nr)
    assert len(pos) == 17
    for i, at in enumerate(pos):
        pay_at = pos[(i + 5) % len(pos)]
        cut, canon, _ = single_null_table(dt, nr, at, pay_at)
        p = lo.join_plan(other, cut)
        want = _oracle.execute(lo.with_inputs(p, [other, canon]))
        assert want.num_rows == n - 1
        for path in ("upload", "adopt"):
            got, ran = run(p, path)
            rows = strict(got, want, (TN[dt], nr, at, path))
            assert launches(ran, "k_decode_pages") == 2, (at, path, sorted(ran))
            # columns: other's key, other's row id, the key, the payload, the row id
            assert all(r[4] != cap + at for r in rows)
            assert [r[3] is None for r in rows if r[4] == cap + pay_at] == [True]
            assert sum(r[3] is None for r in rows) == 1


@pytest.mark.parametrize("garbage", [False, True], ids=["padding-zero", "padding-garbage"])
@pytest.mark.parametrize("dt,nr,branch", lo.SINGLE_NULL_SHAPES, ids=["%s-%d-%s" % (TN[d], n, b) for d, n, b in lo.SINGLE_NULL_SHAPES])
def test_all_valid_column_stays_regular_whatever_the_padding_holds(dt, nr, branch, garbage):
    """the converse: no bit cleared; the bits above nr in the last bitmap byte are zero or garbage"""
    cap = lo.rows_full(dt)
    n = cap + nr
    other = pl.make_table([(dt, lo.typed(dt, np.arange(n))), (I32, np.arange(n, dtype=np.int32))])
    cut, canon, _ = single_null_table(dt, nr, None, None, garbage=garbage)
    last = int(cut.columns[0].pages[1, -1])
    if nr % 8:
        assert (last >> (nr % 8)) == ((lo.FILL >> (nr % 8)) if garbage else 0)
    p = lo.join_plan(other, cut)
    want = _oracle.execute(lo.with_inputs(p, [other, canon]))
    for path in ("upload", "adopt"):
        got, ran = run(p, path)
        rows = strict(got, want, (TN[dt], nr, garbage, path))
        assert len(rows) == n and launches(ran, "k_decode_pages") == 0, (path, sorted(ran))


# ------------------------------------------------- 3. a hard layout under every node kind's scan
def kind_tables(name, seed=0):
    """the cut table (INT32 key of few distinct values, INT64 payload, both cut with the layout and
    both with NULLs) and a small table of keys to meet it"""
    rng = np.random.default_rng([3, seed, sorted(lo.LAYOUTS).index(name)])
    n = lo.fixed_rows(name, I32)
    if name == "overfull_with_nulls":
        kv, pv = lo.null_heavy_valid(n, 11), lo.null_heavy_valid(n, 12)
    else:
        kv, pv = rng.random(n) > 0.03, rng.random(n) > 0.05
    cols = [lo.Col(I32, rng.integers(0, 700, n).astype(np.int32), kv, name, seed),
            lo.Col(I64, rng.integers(-(1 << 20), 1 << 20, n), pv, name, seed)]
    small = [lo.Col(I32, rng.permutation(900)[:450].astype(np.int32), rng.random(450) > 0.02, "random_cuts", 5),
             lo.Col(I64, np.arange(450, dtype=np.int64), None, "last_one_row")]
    return lo.tables(cols), lo.tables(small), cols + small


KINDS = ["semi", "anti", "outer", "full", "agg", "select"]


@pytest.mark.parametrize("name", ["empty_middle_twice", "overfull_with_nulls"])
@pytest.mark.parametrize("kind", KINDS)
def test_hard_layout_under_every_node_kind(kind, name):
    """After table_col the node kinds share one dense column; what differs is the wiring of each
    kind's scan child: it has to take the decoded column AND its validity."""
    (a, a0), (b, b0), cols = kind_tables(name)
    plans = []
    if kind in ("semi", "anti"):
        plans.append(lo.join_plan(b, a, kind=kind, build_left=True, outs=[2, 3]))   # the cut table is preserved
        plans.append(lo.join_plan(b, a, kind=kind, build_left=False, outs=[0, 1]))  # ... is the filter
    elif kind in ("outer", "full"):
        plans.append(lo.join_plan(a, b, kind=kind, build_left=True))    # OUTER: the cut table is optional
        plans.append(lo.join_plan(a, b, kind=kind, build_left=False))   # ... is preserved
    elif kind == "agg":
        p = pl.Plan()
        s = lo.scan_all(p, 0, a)
        p.root = p.new_agg_node(s, 0, [(KEY, 0, I32), (STAR, 0, I64), (COUNT, 1, I64), (SUM, 1, I64), (MIN, 1, I64)])
        p.new_input(a)
        plans.append(p)
    else:
        p = pl.Plan()
        s = lo.scan_all(p, 0, a)
        p.root = p.new_select_node(s, [("LT", 0, 350), ("IS_NULL", 1), ("NOT",), ("AND",), ("IS_NULL", 0), ("OR",)], [(1, I64), (0, I32)])
        p.new_input(a)
        plans.append(p)
    for p in plans:
        canon = [a0, b0] if len(p.inputs) == 2 else [a0]
        if len(p.inputs) == 2 and p.inputs[0] is b:
            canon = [b0, a0]
        want = _selectref.execute(lo.with_inputs(p, canon))
        assert want.num_rows > 0
        for path in ("host", "adopt"):
            got, ran = run(p, path)
            strict(got, want, (kind, name, path))
            assert launches(ran, "k_decode_pages") == irregular(cols if len(p.inputs) == 2 else cols[:2]), sorted(ran)


# --------------------------------------------------------------------- 4. root scan
def words(n, seed=0, nulls=True):
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


def scan_case(name, dt, seed=1):
    if dt == VC:
        cols = [lo.Col(VC, words(400, seed), None, name, seed)]
        cols.append(lo.Col(I32, np.arange(len(cols[0]), dtype=np.int32), None, "canonical" if name == "canonical" else "random_cuts", 2))
        return cols
    n = lo.fixed_rows(name, dt)
    valid = lo.fixed_valid(name, dt, n, seed)
    rng = np.random.default_rng(seed + 70)
    return [lo.Col(dt, lo.typed(dt, rng.integers(0, 1 << 20, n)), valid, name, seed),
            lo.Col(I64, rng.integers(-(1 << 62), 1 << 62, n), None, "canonical" if name == "canonical" else "empty_first")]


@pytest.mark.parametrize("name,dt", [(n, dt) for dt in FIXED for n in sorted(lo.LAYOUTS)] + [(n, VC) for n in lo.VARCHAR_LAYOUTS],
                         ids=lambda v: TN[v] if isinstance(v, int) else v)
def test_root_scan_of_every_layout(name, dt):
    """a plan whose root is the scan: the result is a legal table of the logical rows"""
    cols = scan_case(name, dt)
    cut, canon = lo.tables(cols)
    p = lo.scan_plan(cut)
    want = _oracle.execute(lo.scan_plan(canon))
    for path in paths_of(p):
        got, ran = run(p, path)
        strict(got, want, (name, TN[dt], path))
        assert launches(ran, "k_decode_pages") == irregular(cols), (path, sorted(ran))


def short_and_long_tables(dt, n=2 * 1984 + 50):
    """-> [(what, table, canonical table, NULLs of the second column)]: tables whose second column's
    pages cover fewer rows than num_rows = n + 10, and one whose pages carry ten NULL rows past
    num_rows = n"""
    key = np.arange(n + 10, dtype=np.int32)
    out = []
    for what in ("under-covered, full pages", "under-covered, random cuts", "NULL rows past the end"):
        if what.startswith("under"):
            rows, held = n + 10, n
        else:
            rows, held = n, n + 10
        cap = lo.rows_full(dt) if dt != VC else 0
        if what == "under-covered, full pages":
            held = rows - 10 - (rows - 10) % cap if dt != VC else held  # every page full and valid: only the total tells
        if dt == VC:
            strs = words(held, 9, nulls=False)
            if held > rows:
                strs[rows:] = [None] * (held - rows)
            cuts = lo._vc_greedy(strs, 0, held) if "random" not in what else lo.varchar_layout("random_cuts", strs, 4)[1]
            col = lo.varchar_column(strs, cuts)
            logical = (VC, (strs + [None] * rows)[:rows])
        else:
            vals = lo.typed(dt, np.arange(max(rows, held)) % 5000)
            valid = np.arange(max(rows, held)) < min(rows, held)
            cuts = lo.random_cuts(held, dt, None, 7) if "random" in what else lo._full(held, dt)
            col = lo.column(vals[:held], valid[:held] if held > rows else None, dt, cuts)
            logical = (dt, vals[:rows], valid[:rows])
        kcol = lo.column(key[:rows], None, I32, lo.one_short_middle(rows, I32, None))
        out.append((what, pl.ColumnarTable(rows, [kcol, col]), pl.make_table([(I32, key[:rows]), logical]), rows - min(rows, held)))
    return out


@pytest.mark.parametrize("dt", FIXED + [VC], ids=[TN[d] for d in FIXED + [VC]])
def test_root_scan_of_pages_that_do_not_add_up_to_num_rows(dt):
    """Input pages may cover fewer rows than num_rows (the rest is NULL) or carry NULL rows past it;
    the pages of a RESULT add up to its row count (the strict reader's rule row_total).  Before root_scan
    re-encoded such columns it handed the input pages back under num_rows = t->num_rows, and the strict
    reader refused the result: "rule row_total: the pages hold 4018 rows, the table declares 4028" for the
    under-covered column, "... hold 4028 rows, the table declares 4018" for the one with trailing NULLs."""
    for what, t, canon, nulls in short_and_long_tables(dt):
        with pytest.raises(pc.PageFormatError) as e:
            pc.check_column(t.columns[1], t.num_rows)
        assert e.value.rule_name == "row_total"  # as an INPUT this is what the reference reads
        want = _oracle.execute(lo.scan_plan(canon))
        assert pl.canonical_rows(_oracle.execute(lo.scan_plan(t))) == pl.canonical_rows(want)
        p = lo.scan_plan(t)
        for path in paths_of(p):
            got, _ = run(p, path)
            rows = strict(got, want, (what, TN[dt], path))
            assert sum(r[1] is None for r in rows) == nulls, (what, path)
        # the same tables under a join: the uncovered rows are NULL there as well
        other = pl.make_table([(I32, np.arange(t.num_rows - 30, t.num_rows + 5, dtype=np.int32))])
        j = lo.join_plan(other, t)
        wantj = _oracle.execute(lo.with_inputs(j, [other, canon]))
        for path in paths_of(j):
            got, _ = run(j, path)
            strict(got, wantj, (what, TN[dt], path, "join"))


# --------------------------------------------------------------------- 5. VARCHAR layouts
def probe_rows(col, n_covered, num_rows):
    """row ids worth asking for: the first and last row of every page (which are the rows before and
    after every empty page and every chain, and the chains themselves), their neighbours, and every row
    the pages do not cover"""
    rows = set(range(n_covered, num_rows))
    for a, b in lo.page_first_last_rows(col):
        rows |= {a, b, max(a - 1, 0), min(b + 1, n_covered - 1), (a + b) // 2}
    return sorted(rows)


@pytest.mark.parametrize("env", [None, VDEV], ids=["host-encoder", "device-encoder"])
@pytest.mark.parametrize("name", lo.VARCHAR_LAYOUTS)
def test_varchar_layout_as_payload(name, env):
    """strings gathered through a join by row id, by the host gather (upper_bound over the page
    directory) and by k_vc_resolve (vc_resolve_row's search); the table declares ten rows more than its
    VARCHAR pages hold, which come out NULL"""
    c = lo.Col(VC, words(400, 21), None, name, 3)
    n = len(c)
    col = c.cut_column()
    ids = np.arange(n + 10, dtype=np.int32)
    t = pl.ColumnarTable(n + 10, [lo.column(ids, None, I32, lo.random_cuts(n + 10, I32, None, 8)), col])
    canon = pl.make_table([(I32, ids), (VC, c.values + [None] * 10)])
    ask = probe_rows(col, n, n + 10)
    assert set(range(n, n + 10)) <= set(ask) and 0 in ask and n - 1 in ask
    rng = np.random.default_rng(31)
    pk = np.concatenate([ask, rng.integers(0, n + 10, 100), ask[::3]]).astype(np.int32)
    probe = pl.make_table([(I32, rng.permutation(pk)), (I32, np.arange(pk.size, dtype=np.int32))])
    p = lo.join_plan(t, probe, outs=[1, 0, 3])
    want = _oracle.execute(lo.with_inputs(p, [canon, probe]))
    assert want.num_rows == pk.size
    for path in ("host", "upload"):
        got, ran = run(p, path, env)
        rows = strict(got, want, (name, path, env))
        assert all(r[0] is None for r in rows if r[1] >= n)
        assert (launches(ran, "k_vc_resolve") > 0) == (env is not None), sorted(ran)
        if name in lo.VARCHAR_ONLY:
            assert any(r[0] is not None and len(r[0]) > pc.MAX_INLINE for r in rows)


@pytest.mark.parametrize("build_left", [True, False], ids=["build-left", "build-right"])
@pytest.mark.parametrize("name", lo.VARCHAR_LAYOUTS)
def test_varchar_layout_as_join_key(name, build_left):
    """the same layouts as join keys on both sides (k_vc_hash -> vc_resolve_row over every row in order,
    k_vc_verify over the pairs), as tests/test_gpu_varchar_keys.py does with canonical pages; the left
    table declares ten rows more than its key pages hold: NULL keys, which match nothing"""
    c = lo.Col(VC, words(400, 22), None, name, 4)
    n = len(c)
    left = pl.ColumnarTable(n + 10, [c.cut_column(), lo.column(np.arange(n + 10, dtype=np.int32), None, I32, lo.last_one_row(n + 10, I32, None))])
    left0 = pl.make_table([(VC, c.values + [None] * 10), (I32, np.arange(n + 10, dtype=np.int32))])
    rng = np.random.default_rng(33)
    # the other side: the edge rows of the left pages and every chain, many strings several times, misses, NULLs
    edge = [c.values[r] for r in probe_rows(left.columns[0], n, n)]
    pool = edge + [c.values[int(i)] for i in rng.integers(0, n, 500)] + [b"miss%d:" % i + b"z" * (i % 70) for i in range(300)] + [None] * 10
    pool += [lo.long_string(b"nobody")]
    rs = [pool[int(i)] for i in rng.permutation(len(pool))]
    r = lo.Col(VC, rs, None, "random_cuts" if name != "canonical" else "canonical", 6)
    right, right0 = lo.tables([r, lo.Col(I64, np.arange(len(r), dtype=np.int64), None)])
    p = lo.join_plan(left, right, build_left=build_left, outs=[0, 1, 3])
    want = _oracle.execute(lo.with_inputs(p, [left0, right0]))
    assert want.num_rows > 20
    for env in (None, VDEV):
        got, ran = run(p, "host", env)
        rows = strict(got, want, (name, build_left, env))
        assert launches(ran, "k_vc_hash") == 2, sorted(ran)
        assert all(r[0] is not None and r[1] < n for r in rows)
        if name in lo.VARCHAR_ONLY:
            assert any(len(r[0]) > pc.MAX_INLINE for r in rows)


# ------------------------------------------------- 6. the strip loop of k_page_headers
def test_forty_thousand_one_row_pages_adopted():
    """k_page_headers' grid is capped at 8192 workgroups of four pages: page 39 000 is read in the
    second round of a workgroup's strip.  40 000 one-row INT32 pages, one validity bit cleared, in that
    page; the row joins as NULL, and every page's row base has to be right for the rows around it."""
    n, hole = 40_000, 39_000
    vals = lo.typed(I32, np.arange(n))
    pages = np.zeros((n, pg.PAGE_SIZE), dtype=np.uint8)
    pages[:, 0] = 1           # nr = 1
    pages[:, 2] = 1           # one value
    pages[:, 4:8] = vals.view(np.uint8).reshape(n, 4)
    pages[:, 8:-1] = lo.FILL  # unspecified
    pages[:, -1] = lo.FILL    # bit 0 set: the row is valid; garbage above it
    assert lo.FILL & 1
    pages[hole, 2] = 0
    pages[hole, 4:8] = lo.FILL
    pages[hole, -1] = lo.FILL & 0xFE
    valid = np.ones(n, bool)
    valid[hole] = False
    col = pl.Column(I32, pages)
    dec_v, dec_m = pc.check_column(col, n)
    assert np.array_equal(dec_m, valid) and np.array_equal(dec_v[valid], vals[valid])
    ids = np.arange(n, dtype=np.int32)
    t = pl.ColumnarTable(n, [col, pl.Column(I32, pg.pack_fixed(ids, None, I32))])
    canon = pl.make_table([(I32, vals, valid), (I32, ids)])
    lo_row, hi_row = 37_000, 40_000
    other = pl.make_table([(I32, vals[lo_row:hi_row].copy()), (I64, np.arange(lo_row, hi_row, dtype=np.int64))])
    p = lo.join_plan(other, t)
    want = _oracle.execute(lo.with_inputs(p, [other, canon]))
    assert want.num_rows == hi_row - lo_row - 1
    got, ran = run(p, "adopt")
    rows = strict(got, want, "40 000 one-row pages")
    assert launches(ran, "k_page_headers") == 4 and launches(ran, "k_decode_pages") == 1, sorted(ran)
    # columns: other's key, other's row number, the key, the row id: each row kept its own id
    assert all(r[1] == r[3] for r in rows) and hole not in {r[3] for r in rows}


# ------------------------------------------------- 7. above the cut of a context of two devices
def test_one_short_page_keeps_a_plan_off_the_row_cuts():
    """rj_execute on a context of two devices cuts inputs of 2 * 1984 * 1007 rows and more by row ranges,
    which needs every used column addressable in place (host_column_regular).  One page in the middle
    of the probe key holding a row less: the plan runs on the first device (K1 decodes the column);
    with canonical pages it runs sharded.  Same rows both times."""
    cap = 1984
    n = 2 * 1984 * 1007 + 17
    nb = 3 * cap + 5
    rng = np.random.default_rng(71)
    bk = lo.typed(I32, rng.permutation(nb))
    pk = np.full(n, lo.typed(I32, [nb + 7])[0], dtype=np.int32)
    pk[rng.choice(n, nb, replace=False)] = bk  # every build key is hit once, by rows of both halves
    pv = np.arange(n, dtype=np.int64)
    build = pl.make_table([(I32, bk), (I64, rng.integers(-(1 << 62), 1 << 62, nb))])
    canon = pl.make_table([(I32, pk), (I64, pv)])
    mid = (n // cap // 2) * cap
    short = np.concatenate([pg.pack_fixed(pk[:mid], None, I32), pg.pack_fixed(pk[mid:mid + cap - 1], None, I32),
                            pg.pack_fixed(pk[mid + cap - 1:], None, I32)])
    kcol = pl.Column(I32, lo.scribble(short, I32))
    counts = kcol.pages[:, :2].copy().view(np.uint16)[:, 0]
    assert (counts != cap).sum() == 2 and counts[mid // cap] == cap - 1 and counts[-1] == (n - mid - cap + 1) % cap
    dec_v, dec_m = pc.check_column(kcol, n)
    assert dec_m.all() and np.array_equal(dec_v, pk)
    cut = pl.ColumnarTable(n, [kcol, canon.columns[1]])
    p = lo.join_plan(build, cut)
    ok, why = capi.plan_shardable(p)
    assert ok, why
    want = _oracle.execute(lo.with_inputs(p, [build, canon]))
    assert want.num_rows == nb
    got_a, ran_a = run(p, "host", devices=[0, 0])
    got_b, ran_b = run(lo.with_inputs(p, [build, canon]), "host", devices=[0, 0])
    strict(got_a, want, "one short page")
    strict(got_b, want, "canonical")
    print("short page:", sorted(ran_a.items()))
    print("canonical: ", sorted(ran_b.items()))
    assert launches(ran_a, "k_decode_pages") == 1 and launches(ran_b, "k_decode_pages") == 0
    drop = ("k_decode_pages", "k_scan_bins")
    path_a = {k: v for k, v in ran_a.items() if k.split("<")[0] not in drop}
    path_b = {k: v for k, v in ran_b.items() if k.split("<")[0] not in drop}
    assert path_a != path_b, "both runs launched the same kernels: the canonical layout was not sharded"
    # the sharded run leaves a rank's last page partly filled in the middle of a result column
    rows_b = got_b.columns[0].pages[:, :2].copy().view(np.uint16)[:, 0]
    rows_a = got_a.columns[0].pages[:, :2].copy().view(np.uint16)[:, 0]
    assert (rows_a[:-1] == cap).all() and (rows_b[:-1] != cap).any(), (rows_a.tolist(), rows_b.tolist())


# --------------------------------------------------------------------- 8. error contract
def test_varchar_pages_the_reference_refuses():
    """host-side rejections, no kernel reads these pages: a VARCHAR column that starts with a 0xfffe page,
    and a non-NULL string at or past num_rows; the oracle raises the same message"""
    strs = [b"s%d" % i for i in range(300)]
    ids = np.arange(300, dtype=np.int32)
    probe = pl.make_table([(I32, ids[::7].copy())])
    chain = pg.pack_varchar([lo.long_string(b"x", 2 * pc.LONG_PIECE)])
    assert chain[:, :2].copy().view(np.uint16)[:, 0].tolist() == [0xFFFF, 0xFFFE]
    orphan = np.concatenate([chain[1:], pg.pack_varchar(strs[1:])])
    beyond = pg.pack_varchar(strs)
    for pages, num_rows, msg in ((orphan, 300, "long string page 0xfffe must follows a string"), (beyond, 290, "row_idx")):
        t = pl.ColumnarTable(num_rows, [pl.Column(I32, pg.pack_fixed(ids[:num_rows], None, I32)), pl.Column(VC, pages)])
        with pytest.raises(pc.PageFormatError):
            pc.check_column(t.columns[1], num_rows)
        for p in (lo.join_plan(t, probe, outs=[1, 2]), lo.scan_plan(t)):
            with pytest.raises(RuntimeError, match=msg):
                _oracle.execute(p)
            for env in (None, VDEV):
                with pytest.raises(capi.RjError, match=msg) as e:
                    run(p, "host", env)
                assert e.value.code == 4  # RJ_ERR_DATA
    # ... and the NULL rows a column may carry past num_rows are no error (the fixed-width twin:
    # tests/test_gpu_edges.py::test_trailing_null_rows_beyond_num_rows_are_tolerated)
    t = pl.ColumnarTable(300, [pl.Column(I32, pg.pack_fixed(ids, None, I32)), pl.Column(VC, pg.pack_varchar(strs + [None] * 5))])
    p = lo.join_plan(t, probe, outs=[1, 2])
    want = _oracle.execute(p)
    for env in (None, VDEV):
        got, _ = run(p, "host", env)
        strict(got, want, "NULL strings past the end")
