"""Sort nodes (RJ_NODE_SORT) on the device, through the C-ABI, against the numpy reference
tests/_sortref.py (tests/test_sort_plan.py ties it to a row-at-a-time comparator on the CPU).  Every
result column is read by the strict page reader tests/_pagecheck.py first.

A sort over a SCAN is fully determined (the sort is stable with respect to the table's row order) and is
compared position by position, doubles by their bits.  Over any other child the order inside a group of
equal keys is unspecified: those results go through _sortref.same_sorted(exact=False).  Below another
node a sort is the multiset of its slice; the cases there put the LIMIT at a key boundary, which makes
the slice a determined multiset.

Device path: k_sort_encode writes the keys of one column and counts every digit position, the host
launches k_sort_count / k_sort_scan / k_sort_scatter only for the digits with more than one non-empty
bin (tiles of SORT_TILE rows, read from csrc/rj_device.hpp), k_gather materialises the slice.  The
kernels take one workgroup per tile except k_sort_encode, which strides: test_more_rows_than_the_
striding_grid_covers_at_once has more rows than one sweep of its grid.  The one limit no quick test can
reach is the row limit (2^32 - 16 child rows)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _elfsyms
import _pagecheck as pc
import _sortref
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
KEY, STAR, SUM = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_SUM
_HPP = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
SORT_TILE = int(re.search(r"constexpr int SORT_TILE\s*=\s*(\d+);", _HPP).group(1))
ROWS32, ROWS64 = (int(re.search(rf"constexpr uint32_t {n}\s*=\s*(\d+);", _HPP).group(1)) for n in ("ROWS32", "ROWS64"))
VDEV = {"RJ_TUNE_VARCHAR_DEV": "1"}
POISON = [{"RJ_DEBUG_POISON": str(m)} for m in (0x15A, 0x1FF)]
rng_for, sort_plan, ALL_FLAGS = sp.rng_for, sp.sort_plan, sp.ALL_FLAGS
fam = lambda ran, family: {n: c for n, c in ran.items() if n.split("<")[0] == family}
sort_launches = lambda ran: {n: c for n, c in ran.items() if n.startswith("k_sort_")}
scatters = lambda ran: sum(fam(ran, "k_sort_scatter").values())

_contexts = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _contexts.values():
        c.destroy()
    _contexts.clear()


def context(env=None, **kw):
    """one context per configuration, shared by the cases"""
    key = (tuple(sorted((env or {}).items())), tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _contexts:
        _contexts[key] = fm.tuned_context(env or {}, **kw)
    return _contexts[key]


def run(p, env=None, **kw):
    c = context(env, **kw)
    c.launch_log(True)
    try:
        got = capi.execute(p, c)
        ran = km.launched(c)
    finally:
        c.launch_log(False)
    return got, ran


def ordered_rows(got):
    """the result's rows IN ORDER, every column through the strict page reader first"""
    dec = pc.check_table(got)
    assert pc.same_as(dec, pl.decode_table(got))
    return _sortref.decoded_rows([c.type for c in got.columns], dec, got.num_rows)


def check(p, env=None, what="", exact=None, **kw):
    """Run plan p, whose root is a sort.  exact (default: the child is a scan): position by position
    against the numpy reference and against same_sorted; else same_sorted's tie-aware rules."""
    got, ran = run(p, env, **kw)
    node = p.nodes[p.root]
    d = node.data
    assert isinstance(d, pl.SortNode)
    if exact is None:
        exact = isinstance(p.nodes[d.child].data, pl.ScanNode)
    n_child, child = _sortref.evaluate(p, d.child)
    begin, count = _sortref.slice_of(n_child, d.limit, d.offset)
    assert got.num_rows == count, (what, got.num_rows, count)
    assert [c.type for c in got.columns] == [t for _, t in node.output_attrs], what
    rows = ordered_rows(got)
    if exact:
        assert rows == _sortref.rel_rows(_sortref.evaluate(p)[1], count), what
    bad = _sortref.same_sorted(rows, _sortref.rel_rows(child, n_child), d.keys, d.limit, d.offset, exact,
                               outs=[i for i, _ in node.output_attrs])
    assert bad is None, (what, bad)
    return got, ran


def same_multiset(got, want, what=""):
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    dec = pc.check_table(got)
    assert pc.same_as(dec, pl.decode_table(got)), what
    assert pc.canonical_rows(dec) == pl.canonical_rows(want), what


def _col3(col):
    return col if len(col) == 3 else (col[0], col[1], np.ones(col[1].shape[0], bool))


def expected_passes(dt, vals, valid, flags):
    """The skip rule of include/rj.h / DESIGN.md: one pass per digit position (8 bits of the encoded
    key, the NULL flag) that has more than one non-empty bin over ALL rows — a NULL's value bits are 0."""
    nd, key = _sortref.encode(dt, vals, valid, flags)
    value = sum(np.unique((key >> np.uint64(8 * b)) & np.uint64(255)).size > 1 for b in range(4 if dt == I32 else 8))
    return int(value) + int(np.unique(nd).size > 1)


# ------------------------------------------------------------------ sizes where the kernels switch branches
SIZES = [1, 63, 64, 65, 255, 256, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 5 * SORT_TILE + 17,
         ROWS64 - 1, ROWS64, ROWS64 + 1, ROWS32 - 1, ROWS32, ROWS32 + 1]


def grid_table(n, form, rng):
    """an INT32 key that is a random permutation + an INT64 payload; form "nulls": NULLs in both"""
    cols = [(I32, rng.permutation(n).astype(np.int32)), (I64, rng.integers(-2**62, 2**62, n))]
    if form == "nulls":
        cols = [(dt, v, rng.random(n) >= 0.1) for dt, v in cols]
    return cols


def grid_case(n, form, env=None):
    cols = grid_table(n, form, rng_for("grid", n, form))
    got, ran = check(sort_plan(cols, [(0, 0)], outs=[1, 0]), env, what=(n, form))
    assert scatters(ran) == expected_passes(*_col3(cols[0]), 0), (n, form, ran)
    assert sum(fam(ran, "k_sort_encode").values()) == 1
    return got


@pytest.mark.parametrize("form", ["paged", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_size_grid(n, form):
    grid_case(n, form)


def test_more_rows_than_the_striding_grid_covers_at_once():
    """k_sort_encode strides over chunks of 256 rows with at most 8 workgroups per CU"""
    n = 8 * 256 * context().device_info()["compute_units"] + 3 * SORT_TILE + 11
    rng = rng_for("stride")
    cols = [(I32, rng.permutation(n).astype(np.int32)), (I64, np.arange(n))]
    got, ran = run(sort_plan(cols, [(0, DESC)]))
    dec = pc.check_table(got)
    assert got.num_rows == n and np.array_equal(dec[0][0], np.arange(n - 1, -1, -1, dtype=np.int32))
    assert np.array_equal(dec[1][0], np.argsort(-cols[0][1].astype(np.int64), kind="stable"))
    assert dec[0][1].all() and dec[1][1].all() and scatters(ran) == 3


# ------------------------------------------------------------------ stability and digits
def _exact(key, dt=I32, flags=0, n_scatter=None, payload=None):
    n = key.shape[0]
    cols = [(dt, key.astype(km.NP_OF[dt])), (I64, np.arange(n) if payload is None else payload)]
    got, ran = check(sort_plan(cols, [(0, flags)]), what=(dt, flags, n))
    if n_scatter is not None:
        assert scatters(ran) == n_scatter, ran
    return got, ran


def test_all_keys_equal_launch_no_scatter_and_return_the_input():
    n = 2 * SORT_TILE + 5
    got, ran = _exact(np.full(n, 77), n_scatter=0)
    assert not fam(ran, "k_sort_count") and not fam(ran, "k_sort_scan")
    assert np.array_equal(pl.decode_table(got)[1][0], np.arange(n))


def test_two_values_alternating():
    n = 3 * SORT_TILE + 1
    got, _ = _exact(np.arange(n) % 2 * 1000 - 500)   # -500, 500: they differ in several bytes
    assert np.array_equal(pl.decode_table(got)[1][0], np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)]))
    _exact(np.arange(n) % 2, flags=DESC, n_scatter=1)


def test_sorted_and_reverse_sorted_input():
    n = 2 * SORT_TILE + 300
    _exact(np.arange(n) - 1000)
    _exact(np.arange(n)[::-1] - 1000)
    _exact(np.arange(n) // 3, flags=DESC)           # ties, already in order: DESC must not reverse them


def test_keys_that_differ_in_one_byte_cost_one_pass():
    n = 2 * SORT_TILE + 9
    rng = rng_for("bytes")
    _exact(((rng.integers(0, 256, n) << 24) - 2**31), n_scatter=1)       # the top byte only (the sign among it)
    _exact(rng.integers(0, 256, n) + 0x1200, n_scatter=1)                # the bottom byte only
    _exact(rng.integers(0, 256, n) << 8, n_scatter=1)
    _exact(rng.integers(0, 200, n), dt=I64, n_scatter=1)                 # INT64 in [0, 200): one pass of eight
    _exact(rng.integers(-2**62, 2**62, n), dt=I64, n_scatter=8)
    _exact(rng.integers(-2**31, 2**31, n), n_scatter=4)


def test_many_copies_of_few_keys_keep_their_input_order():
    key = rng_for("copies").permutation(np.repeat(np.arange(40) * 1_000_003 % 65_521 - 30_000, 300))
    got, _ = _exact(key)                             # payload = position: any instability shows
    pay = pl.decode_table(got)[1][0].reshape(40, 300)
    assert (np.diff(pay, axis=1) > 0).all()


# ------------------------------------------------------------------ types and flags
def edge_table(dt, rng, reps=3):
    """the edge list of tests/test_sort_plan.py as data, every value `reps` times, shuffled; + position"""
    bits = [b for _, b in sp.EDGES[dt]] * reps
    null = [v is None for v, _ in sp.EDGES[dt]] * reps
    at = rng.permutation(len(bits))
    raw = np.array(bits, dtype=np.uint64)[at]
    vals = raw.astype(np.uint32).view(np.int32) if dt == I32 else raw.view(km.NP_OF[dt])
    return [(dt, vals, ~np.array(null)[at]), (I32, np.arange(len(bits), dtype=np.int32))]


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_edge_values_of_every_type_under_every_flag(dt, flags):
    cols = edge_table(dt, rng_for("edges", dt, flags))
    got, ran = check(sort_plan(cols, [(0, flags)]), what=(dt, flags))
    assert fam(ran, "k_sort_scatter").get("k_sort_scatter<2>") == 1     # the NULL flag's pass
    rows = ordered_rows(got)
    nulls = [r[0] is None for r in rows]
    assert nulls == sorted(nulls, reverse=bool(flags & NF)) and any(nulls)
    if dt == F64:   # what is output keeps its own bits: every NaN payload and both zeros come back
        assert {r[0][1] & (2**64 - 1) for r in rows if r[0]} == {b for v, b in sp.EDGES[F64] if v is not None}


def test_nullable_column_without_a_null_costs_no_flag_pass():
    rng = rng_for("noflag")
    n = SORT_TILE + 100
    cols = [(I32, rng.integers(0, 500, n).astype(np.int32), rng.random(n) >= 0.3), (I32, np.arange(n, dtype=np.int32))]
    p = pl.Plan()
    sc = p.new_scan_node(0, [(0, I32), (1, I32)])
    keep = p.new_select_node(sc, [("IS_NOT_NULL", 0)], [(0, I32), (1, I32)])  # dense values + validity bytes, all set
    p.root = p.new_sort_node(keep, [(0, NF)], [(0, I32), (1, I32)])
    p.new_input(pl.make_table(cols))
    got, ran = check(p)
    assert 0 < got.num_rows < n and scatters(ran) == 2
    assert "k_sort_scatter<2>" not in ran and "k_sort_count<2>" not in ran
    _, ran = check(sort_plan(cols, [(0, NF)]))      # ... with them: one more pass
    assert ran.get("k_sort_scatter<2>") == 1 and ran.get("k_sort_count<2>") == 1
    assert scatters(ran) == 4 == expected_passes(*cols[0], NF)          # (a NULL's key is 0: the sign byte now differs too)


# ------------------------------------------------------------------ keys
def test_two_and_three_keys_of_mixed_types_and_directions():
    cols = sp.key_table(rng_for("keys"), 6_000, sp.TYPES, domain=3)      # heavy ties on every key
    for keys in ([(0, DESC), (2, NF)], [(3, 0), (1, DESC | NF), (4, DESC)], [(2, DESC | NF), (0, 0), (1, 0)]):
        check(sort_plan(cols, keys), what=keys)


def test_the_same_column_twice_and_a_key_that_is_not_output():
    cols = sp.key_table(rng_for("twice"), 5_000, sp.TYPES, domain=4)
    a, ran = check(sort_plan(cols, [(1, 0), (1, DESC), (2, 0)], outs=[0, 4]))
    assert sum(fam(ran, "k_sort_encode").values()) == 2                  # the second (1, ...) orders nothing
    b, _ = run(sort_plan(cols, [(1, 0), (2, 0)], outs=[0, 4]))
    assert ordered_rows(a) == ordered_rows(b)
    check(sort_plan(cols, [(1, DESC), (1, 0)], outs=[1, 1, 3]))


def test_eight_keys():
    rng = rng_for("eight")
    n = 4_000
    types = [I32, I64, F64, I32, I64, F64, I32, I64]
    cols = [(dt, rng.integers(0, 2, n).astype(km.NP_OF[dt]), rng.random(n) >= 0.1) for dt in types] + [(I32, np.arange(n, dtype=np.int32))]
    keys = [(c, int(rng.integers(0, 4))) for c in rng.permutation(8)]
    got, ran = check(sort_plan(cols, keys, outs=[8, 0, 7]))
    assert sum(fam(ran, "k_sort_encode").values()) == 8


def _pb(rng, n=6_000, kt=I32):
    k = km.key_values(kt, rng.integers(0, 900, n))
    p = [(kt, k, rng.random(n) >= 0.05), km.payload(rng, I64, n, True)]
    b = [(kt, km.key_values(kt, rng.integers(400, 1_400, n // 2)), rng.random(n // 2) >= 0.05),
         (I32, rng.integers(-50, 50, n // 2).astype(np.int32))]
    return p, b


def _two_scans(pcols, bcols):
    p = pl.Plan()
    sa = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(pcols)])
    sb = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(bcols)])
    p.new_input(pl.make_table(pcols))
    p.new_input(pl.make_table(bcols))
    return p, sa, sb


ALL4 = [(0, I32), (1, I64), (2, I32), (3, I32)]


def _binary(p, kind, build_left, l, r, outs):
    mk = {"join": p.new_join_node, "semi": p.new_semi_join_node, "anti": p.new_anti_join_node,
          "outer": p.new_outer_join_node, "full": p.new_full_outer_join_node}[kind]
    return mk(build_left, l, r, 0, 0, outs)


def test_dense_keys_of_a_join_and_paged_keys_of_a_scan():
    rng = rng_for("dense")
    pcols, bcols = _pb(rng)
    p, sa, sb = _two_scans(pcols, bcols)
    j = p.new_join_node(False, sa, sb, 0, 0, ALL4)
    p.root = p.new_sort_node(j, [(3, DESC), (0, 0)], ALL4)               # dense columns, ties on both
    got, ran = check(p)
    assert got.num_rows > 0 and scatters(ran) > 0
    cols = [(I32, rng.integers(0, 50, 5_000).astype(np.int32)), (I64, rng.integers(-9, 9, 5_000))]  # regular pages, read in place
    check(sort_plan(cols, [(1, 0), (0, DESC)]))


def _five(rng, n=3_000):
    return [km.payload(rng, I32, n, True), km.payload(rng, I64, n, False), km.payload(rng, F64, n, True),
            km.payload(rng, VC, n, False), (I32, rng.integers(0, 100, n).astype(np.int32))]


@pytest.mark.parametrize("enc,env", [("host", None), ("device", VDEV)])
def test_varchar_and_nullable_payloads_come_out_in_order_at_the_root(enc, env):
    cols = _five(rng_for("vc", enc))
    for kw in ({}, {"limit": 700, "offset": 33}):
        got, ran = check(sort_plan(cols, [(4, DESC), (0, NF)], outs=[3, 0, 2, 3], **kw), env, what=(enc, kw))
        assert got.num_rows > 0 and bool(fam(ran, "k_vc_encode")) == (env is not None)
    check(sort_plan(cols, [], outs=[3, 2], limit=500, offset=100), env)   # no key: the slice is a run of positions


# ------------------------------------------------------------------ slices
def test_limits_and_offsets():
    n = 1_000
    rng = rng_for("slices")
    cols = [(I32, rng.permutation(n).astype(np.int32)), (I64, rng.integers(-99, 99, n), rng.random(n) >= 0.2)]
    for limit in (0, 1, n - 1, n, n + 1, None):
        for offset in (0, 1, n - 1, n, n + 1):
            got, ran = check(sort_plan(cols, [(0, DESC)], limit=limit, offset=offset), what=(limit, offset))
            if got.num_rows == 0:
                assert all(c.pages.shape[0] == 0 for c in got.columns) and not sort_launches(ran)
    # offset + limit beyond 2^64
    for limit, offset, rows in ((2**64 - 2, 5, n - 5), (2**64 - 1, 2**64 - 1, 0), (7, 2**64 - 1, 0), (2**64 - 2, 2, n - 2)):
        got, _ = check(sort_plan(cols, [(0, 0)], limit=limit, offset=offset), what=(limit, offset))
        assert got.num_rows == rows


def test_boundary_inside_a_tie_group():
    rng = rng_for("ties")
    n = 3_000
    cols = [(I32, rng.integers(0, 12, n).astype(np.int32)), (I32, np.arange(n, dtype=np.int32))]
    inside = int((cols[0][1] < 5).sum()) + 7
    check(sort_plan(cols, [(0, 0)], limit=inside - 100, offset=100))     # a scan: stable, so still exact
    pcols, bcols = _pb(rng)
    p, sa, sb = _two_scans(pcols, bcols)
    j = p.new_join_node(False, sa, sb, 0, 0, ALL4)
    n_join, jcols = _sortref.evaluate(p, j)
    top = np.sort(jcols[3][1])[n_join // 2]
    cut = int((jcols[3][1] < top).sum()) + 1                             # one row into the group of `top`
    assert cut < int((jcols[3][1] <= top).sum())
    p.root = p.new_sort_node(j, [(3, 0)], ALL4, limit=cut - 10, offset=10)
    check(p, exact=False)


@pytest.mark.parametrize("count", [ROWS32 - 1, ROWS32, ROWS32 + 1, ROWS64 - 1, ROWS64, ROWS64 + 1])
def test_slices_around_one_result_pages_capacity(count):
    n = 3 * ROWS32 + 5
    rng = rng_for("pages", count)
    cols = [(I32, rng.permutation(n).astype(np.int32)), (I64, rng.integers(-2**62, 2**62, n)),
            (I64, rng.integers(0, 9, n), rng.random(n) >= 0.2)]
    got, ran = check(sort_plan(cols, [(0, 0)], limit=count, offset=17), what=count)
    assert got.columns[0].pages.shape[0] == -(-count // ROWS32) and got.columns[1].pages.shape[0] == -(-count // ROWS64)
    assert fam(ran, "k_encode_nullable") and fam(ran, "k_finish_pages")


def test_limit_and_offset_without_keys_over_a_scan():
    cols = _five(rng_for("nokeys"), 2_500)
    for limit, offset in ((10, 0), (None, 2_490), (100, 1_000), (None, 0), (0, 0), (5, 2_500)):
        got, ran = check(sort_plan(cols, [], outs=[1, 0, 4], limit=limit, offset=offset), what=(limit, offset))
        assert not fam(ran, "k_sort_encode") and not scatters(ran)
        assert bool(fam(ran, "k_sort_iota")) == (0 < got.num_rows < 2_500)


# ------------------------------------------------------------------ composition
def _under(kind, rng):
    """-> (plan, node, its output_attrs) for a child of every other kind"""
    pcols, bcols = _pb(rng)
    p, sa, sb = _two_scans(pcols, bcols)
    if kind == "agg":
        return p, p.new_agg_node(sa, 0, [(KEY, 0, I32), (STAR, 0, I64), (SUM, 1, I64)]), [(0, I32), (1, I64), (2, I64)]
    if kind == "select":
        return p, p.new_select_node(sa, [("LT", 1, 0), ("IS_NULL", 1), ("OR",)], [(0, I32), (1, I64)]), ALL4[:2]
    if kind == "sort":
        return p, p.new_sort_node(sa, [(1, DESC)], [(0, I32), (1, I64)], limit=4_000), ALL4[:2]
    outs = ALL4[:2] if kind in ("semi", "anti") else ALL4
    return p, _binary(p, kind, False, sa, sb, outs), outs


KINDS = ["join", "semi", "anti", "outer", "full", "agg", "select", "sort"]


@pytest.mark.parametrize("kind", KINDS)
def test_sort_as_the_root_over_every_other_kind(kind):
    p, node, outs = _under(kind, rng_for("over", kind))
    keys = [(len(outs) - 1, NF | DESC), (0, 0)]
    for kw in ({}, {"limit": 500, "offset": 250}):
        p.root = p.new_sort_node(node, keys, list(reversed(outs)), **kw)
        got, ran = check(p, exact=False, what=(kind, kw))
        assert got.num_rows > 0 and fam(ran, "k_sort_encode")


@pytest.mark.parametrize("build_left", [True, False], ids=["built", "probed"])
@pytest.mark.parametrize("kind", KINDS[:7])
def test_every_other_kind_over_a_sort_with_a_limit_at_a_key_boundary(kind, build_left):
    """the slice ends where a key value ends, so it is a determined multiset and the references apply"""
    pcols, bcols = _pb(rng_for("under", kind, build_left))
    p, sa, sb = _two_scans(pcols, bcols)
    k, valid = pcols[0][1], pcols[0][2]
    cut = np.sort(k[valid])[2 * valid.sum() // 3]
    limit = int((valid & (k >= cut)).sum())                              # NULLs last: the largest keys, whole groups
    s = p.new_sort_node(sa, [(0, DESC)], [(0, I32), (1, I64)], limit=limit)
    if kind == "agg":
        p.root = p.new_agg_node(s, 0, [(KEY, 0, I32), (STAR, 0, I64), (SUM, 1, I64)])
    elif kind == "select":
        p.root = p.new_select_node(s, [("LT", 1, 0), ("IS_NULL", 1), ("OR",)], [(1, I64), (0, I32)])
    else:
        outs = ALL4
        if kind in ("semi", "anti"):
            outs = [(2, I32), (3, I32)] if build_left else ALL4[:2]
        p.root = _binary(p, kind, build_left, s, sb, outs)
    got, ran = run(p)
    same_multiset(got, _sortref.execute(p), (kind, build_left))
    assert got.num_rows > 0 and scatters(ran) > 0


def test_a_non_root_sort_without_a_slice_launches_no_sort_kernel():
    pcols, bcols = _pb(rng_for("passthrough"))
    p, sa, sb = _two_scans(pcols, bcols)
    s = p.new_sort_node(sa, [(1, DESC), (0, 0)], [(1, I64), (0, I32)])
    p.root = p.new_join_node(False, s, sb, 1, 0, [(0, I64), (1, I32), (3, I32)])
    got, ran = run(p)
    same_multiset(got, _sortref.execute(p))
    assert got.num_rows > 0 and not sort_launches(ran), ran
    # ... but is validated all the same
    s2 = p.new_sort_node(sa, [(5, 0)], [(1, I64), (0, I32)])
    p.root = p.new_join_node(False, s2, sb, 1, 0, [(0, I64), (1, I32), (3, I32)])
    assert _error(p)[0] == ARG


def test_same_plan_twice_on_one_context():
    cols = sp.key_table(rng_for("twice"), 10_000, sp.TYPES, domain=5)
    p = sort_plan(cols, [(2, DESC), (0, NF)], limit=6_000, offset=5)
    a, _ = run(p)
    b, _ = run(p)
    assert a.num_rows == b.num_rows == 6_000 and ordered_rows(a) == ordered_rows(b)


# ------------------------------------------------------------------ fuzz
def fuzz_case(seed):
    rng = rng_for("fuzz", seed)
    n = int(rng.integers(1, 3_000))
    types = [[I32, I64, F64][int(rng.integers(0, 3))] for _ in range(4)]
    cols = sp.key_table(rng, n, types, null_p=[0.0, 0.05, 0.5][int(rng.integers(0, 3))], domain=int(rng.integers(1, 40)))
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, dt) for i, dt in enumerate(types)])
    p.new_input(pl.make_table(cols))
    child, kind = sc, ["scan", "select", "join", "agg"][int(rng.integers(0, 4))]
    if kind == "select":
        child = p.new_select_node(sc, [("IS_NOT_NULL", 0), ("IS_NULL", 1), ("OR",)], [(i, dt) for i, dt in enumerate(types)])
    elif kind == "join" and types[0] != F64:
        other = p.new_scan_node(0, [(0, types[0])])
        child = p.new_semi_join_node(False, sc, other, 0, 0, [(i, dt) for i, dt in enumerate(types)])
    elif kind == "agg" and types[0] != F64:
        child = p.new_agg_node(sc, 0, [(KEY, 0, types[0]), (STAR, 0, I64)])
        types = [types[0], I64]
    nk = int(rng.integers(0, 4))
    keys = [(int(rng.integers(0, len(types))), int(rng.integers(0, 4))) for _ in range(nk)]
    m = _sortref.evaluate(p, child)[0]
    limit = None if rng.random() < 0.3 else int(rng.integers(0, m + 3))
    offset = 0 if rng.random() < 0.4 else int(rng.integers(0, m + 2))
    p.root = p.new_sort_node(child, keys, [(i, dt) for i, dt in enumerate(types)], limit, offset)
    return p


@pytest.mark.parametrize("block", range(15))
def test_fuzz(block):
    """150 seeded cases, ten per block: type, flags, key count, NULL rate, limit, offset, child kind"""
    rows = 0
    for seed in range(10 * block, 10 * block + 10):
        got, _ = check(fuzz_case(seed), what=seed)
        rows += got.num_rows
    assert rows > 0


# ------------------------------------------------------------------ dirty memory
@pytest.mark.parametrize("env", POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env):
    for n in (SORT_TILE - 1, SORT_TILE + 1):
        for form in ("paged", "nulls"):
            grid_case(n, form, env)
    cols = sp.key_table(rng_for("poison"), 6_000, sp.TYPES, domain=3)
    check(sort_plan(cols, [(3, 0), (1, DESC | NF), (4, DESC)], limit=4_000, offset=9), env)
    s = context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


# ------------------------------------------------------------------ the error contract
def _error(p, ctx=None):
    with pytest.raises(capi.RjError) as e:
        capi.execute(p, ctx or context())
    return e.value.code, str(e.value)


ARG, UNSUPPORTED = 1, 5


@pytest.mark.parametrize("rows", [300, 0], ids=["rows", "empty-child"])
def test_error_contract(rows):
    """every refusal, also over an empty child: the node is checked before its child's rows are looked at"""
    cols = _five(rng_for("err"), rows)  # I32, I64, F64, VARCHAR, I32
    if not rows:
        cols = [(I32, np.zeros(0, np.int32)), (I64, np.zeros(0, np.int64)), (F64, np.zeros(0)), (VC, []), (I32, np.zeros(0, np.int32))]
    bad = lambda keys, **kw: _error(sort_plan(cols, keys, **kw))
    for keys, text in (([(5, 0)], "key column out of range"), ([(-1, 0)], "key column out of range"), ([(0, 0), (99, DESC)], "out of range"),
                       ([(0, 4)], "flags"), ([(0, -1)], "flags"), ([(1, 1 | 2 | 8)], "flags")):
        code, msg = bad(keys)
        assert code == ARG and text in msg, (keys, msg)
    code, msg = bad([(3, 0)])
    assert code == UNSUPPORTED and "VARCHAR" in msg
    code, msg = bad([(0, 0), (3, DESC)])
    assert code == UNSUPPORTED and "VARCHAR" in msg
    code, msg = bad([(k % 3, 0) for k in range(9)])
    assert code == UNSUPPORTED and "8" in msg
    check(sort_plan(cols, [(k % 3, k % 4) for k in range(8)], outs=[0, 1, 2]))   # (eight are fine)
    p = sort_plan(cols, [(0, 0)])
    p.nodes[p.root].output_attrs[1] = (1, I32)  # the child column is INT64
    code, msg = _error(p)
    assert code == ARG and "declared type" in msg
    p = sort_plan(cols, [(0, 0)])
    p.nodes[p.root].output_attrs[0] = (7, I32)
    code, msg = _error(p)
    assert code == ARG and "output attr out of range" in msg
    # keys announced, none given
    p = sort_plan(cols, [(0, 0)])
    cplan, keep = pl.plan_to_c(p)
    cplan.nodes[p.root].right_attr = 0
    c = context()
    out = C.c_void_p()
    rc = c.L.rj_execute(c.h, C.byref(cplan), C.byref(out))
    assert rc == ARG and b"NULL key pointer" in c.L.rj_last_error(c.h)
    del keep


def test_empty_child_and_empty_slice_give_typed_columns_without_pages():
    none = [(I32, np.zeros(0, np.int32)), (I64, np.zeros(0, np.int64)), (VC, [])]
    some = [(I32, np.arange(500, dtype=np.int32)), (I64, np.arange(500)), km.payload(rng_for("e"), VC, 500, False)]
    for cols, kw in ((none, {}), (none, {"limit": 5}), (some, {"limit": 0}), (some, {"offset": 500}), (some, {"offset": 2**63})):
        got, ran = check(sort_plan(cols, [(0, DESC)], outs=[1, 2, 0], **kw), what=kw)
        assert got.num_rows == 0 and [c.type for c in got.columns] == [I64, VC, I32]
        assert all(c.pages.shape[0] == 0 for c in got.columns) and not sort_launches(ran)


def test_execute_sharded_refuses_and_a_two_device_context_runs_on_one():
    cols = grid_table(5_000, "nulls", rng_for("two"))
    p = sort_plan(cols, [(0, DESC | NF)], limit=2_000)
    got, _ = check(p, devices=[0, 0])
    assert got.num_rows == 2_000
    ctx = context(devices=[0, 0])
    tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
    try:
        with pytest.raises(capi.RjError) as e:
            ctx.execute_sharded(p, tables)
        assert e.value.code == UNSUPPORTED and "RJ_NODE_SORT" in str(e.value)
    finally:
        for row in tables:
            for t in row:
                t.release()


def test_resident_tables_and_results_kept_on_the_device():
    cols = grid_table(50_000, "nulls", rng_for("resident"))
    p = sort_plan(cols, [(0, 0)], limit=20_000, offset=100)
    want = _sortref.rel_rows(_sortref.evaluate(p)[1], 20_000)
    ctx = context()
    t = ctx.upload(p.inputs[0])
    try:
        for keep in (True, False):
            r = ctx.execute_resident(p, [t], keep_on_device=keep)
            try:
                if keep:
                    assert all(r.device_pages(c) for c in range(r.num_cols))
                assert ordered_rows(r.to_table()) == want, keep
            finally:
                r.free()
    finally:
        t.release()


# ------------------------------------------------------------------ every compiled instantiation
def test_every_sort_instantiation_is_driven():
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.startswith("k_sort_")}
    assert compiled == {"k_sort_encode<4>", "k_sort_encode<8>", "k_sort_count<0>", "k_sort_count<1>", "k_sort_count<2>", "k_sort_scan",
                        "k_sort_scatter<0>", "k_sort_scatter<1>", "k_sort_scatter<2>", "k_sort_iota"}, sorted(compiled)
    cols = sp.key_table(rng_for("matrix"), SORT_TILE + 1, [I32, I64, F64])
    reached = set()
    for p in (sort_plan(cols, [(0, 0), (1, DESC), (2, NF)]), sort_plan(cols, [], limit=5, offset=5)):
        reached |= set(sort_launches(check(p)[1]))
    assert reached == compiled, (sorted(reached), sorted(compiled))
