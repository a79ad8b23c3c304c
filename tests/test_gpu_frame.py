"""ROWS frames, LAG / LEAD / FIRST_VALUE / LAST_VALUE and NTILE of window nodes on the device, through
the C-ABI, against the numpy reference tests/_frameref.py (tests/test_frame_plan.py ties it to a
row-at-a-time walk on the CPU).  Every result column is read by the strict page reader
tests/_pagecheck.py first.  Everything is exact: integers, and FP64 by bit pattern; every row is compared.

Every function here can depend on the order among peers, so a root window node over a SCAN child (ties
stable with respect to the scan's order) is compared row by row IN ORDER, and anything else as a multiset
with order keys that are unique within a partition.

Device path: the order, the head masks and the scans of the window node; a k_win_ranks launch with Q := P
gives every position its partition; k_frame_pick / k_frame_ntile / k_frame_sum have one thread per
position; k_frame_leaves / k_frame_levels build a range-extreme tree of fan-out FRAME_FANOUT (two levels
per launch, 256 positions per workgroup) and k_frame_extreme walks it.  The sizes below sit on and next
to the item (64), quarter (1024) and tile (4096) borders of the window kernels and on fan-out, fan-out^2
and fan-out^3 of the tree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _frameref
import _pagecheck as pc
import test_frame_plan as fp
import test_gpu_kernel_matrix as km
import test_gpu_window as gw
import test_sort_plan as sp
import test_window_plan as wp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
COL, ROWNO, RANK, DENSE, STAR, COUNT, SUM, MIN, MAX = wp.COL, wp.ROWNO, wp.RANK, wp.DENSE, wp.STAR, wp.COUNT, wp.SUM, wp.MIN, wp.MAX
LAG, LEAD, FIRST, LAST, NTILE, RSTAR, RCOUNT, RSUM, RMIN, RMAX = fp.LAG, fp.LEAD, fp.FIRST, fp.LAST, fp.NTILE, fp.RSTAR, fp.RCOUNT, fp.RSUM, fp.RMIN, fp.RMAX
UNB_P, UNB_F, FRAMES = fp.UNB_P, fp.UNB_F, fp.FRAMES
TILE = gw.TILE
F = int(re.search(r"constexpr int FRAME_FANOUT\s*=\s*(\d+);", gw._HPP).group(1))
assert F in (16, 64)
rng_for, window_plan, fam, launches = sp.rng_for, wp.window_plan, gw.fam, gw.launches
ARG, UNSUPPORTED = 1, 5
OFFSETS = [0, 1, 2, 63, 64, 65, 1024, 4096]
UNKNOWN = "unknown function code"


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in gw._contexts.values():
        c.destroy()
    gw._contexts.clear()


def check(p, env=None, what="", **kw):
    """Run plan p against the reference: a root window node over a scan row by row in order, anything
    else as a multiset."""
    got, ran = gw.run(p, env, **kw)
    n, cols = _frameref.evaluate(p)
    d = p.nodes[p.root].data
    assert got.num_rows == n, (what, got.num_rows, n)
    assert [c.type for c in got.columns] == [c[0] for c in cols], what
    rows, want = gw.ordered_rows(got), _frameref.rel_rows(cols, n)
    if isinstance(d, pl.WindowNode) and isinstance(p.nodes[d.child].data, pl.ScanNode):
        bad = [i for i, (a, b) in enumerate(zip(rows, want)) if a != b]
        assert not bad, (what, len(bad), bad[0], rows[bad[0]], want[bad[0]], _frameref.outputs_of(p.nodes[p.root]))
    else:
        assert gw._any_order(rows) == gw._any_order(want), what
    return got, ran


def table(part_sizes, rng, nulls=True, shuffle=True):
    """gw.laid_out_table with every order key distinct: an INT32 partition key (0), a unique INT32 order key
    (1), an INT64 value (2), a paged INT32 value (3) and an FP64 value (4); 2 and 4 nullable if `nulls`"""
    n = int(np.sum(part_sizes))
    cols = gw.laid_out_table(part_sizes, [1] * n, rng, shuffle)
    if not nulls:
        cols = [c[:2] for c in cols]
    return cols


def every_function(frames, offsets=(1,), buckets=(3,), cols=(2, 3, 4), types=(I64, I32, F64)):
    outs = [(NTILE, 0, I64, b, 0) for b in buckets] + [(RSTAR, 0, I64, lo, hi) for lo, hi in frames]
    for c, dt in zip(cols, types):
        outs += [(f, c, dt, k, 0) for f in (LAG, LEAD) for k in offsets]
        for lo, hi in frames:
            outs += [(FIRST, c, dt, lo, hi), (LAST, c, dt, lo, hi), (RCOUNT, c, I64, lo, hi), (RMIN, c, dt, lo, hi), (RMAX, c, dt, lo, hi)]
            outs += [(RSUM, c, I64, lo, hi)] if dt != F64 else []
    return outs


# ------------------------------------------------------------------ row counts and partitions
SIZES = sorted({1, 2, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 1, F - 1, F + 1, F * F - 1, F * F + 1,
                min(F**3 + 1, 300_000)})
PARTS = gw.PARTS
GRID_FRAMES = [(-6, 0), (-1, 1), (-65, 0), (UNB_P, -1), (-1024, 1024)]


def grid_case(n, part, nulls, env=None, frames=GRID_FRAMES):
    rng = rng_for("frame-grid", n, part, nulls)
    ps, _ = gw.form_sizes(n, part, "distinct", rng)
    cols = table(ps, rng, nulls)
    outs = [(COL, 1, I32), (ROWNO, 0, I64), (SUM, 2, I64)] + every_function(frames)
    return check(window_plan(cols, [(0, 0)], [(1, 0)], outs), env, what=(n, part, nulls))


@pytest.mark.parametrize("n", SIZES)
def test_size_grid(n):
    for part in PARTS:
        for nulls in (True, False):
            got, ran = grid_case(n, part, nulls)
            assert got.num_rows == n and sum(fam(ran, "k_frame_leaves").values()) == 6 and sum(fam(ran, "k_win_ranks").values()) == 2


@pytest.mark.parametrize("frame", FRAMES, ids=[f"{lo}..{hi}" for lo, hi in FRAMES])
def test_every_function_under_every_frame(frame):
    """frames wider than the partition, wider than the table, empty at one or both partition ends"""
    for n, part in ((3 * TILE + 1, "runs700"), (3 * TILE + 1, "one"), (1025, "runs3"), (F * F + 1, "each")):
        grid_case(n, part, True, frames=[frame])


def test_lag_and_lead_offsets():
    n = 3 * TILE + 1
    for part in ("one", "runs700", "runs3"):
        rng = rng_for("offsets", part)
        cols = table(gw.form_sizes(n, part, "distinct", rng)[0], rng)
        outs = [(f, c, dt, k, 0) for f in (LAG, LEAD) for k in OFFSETS + [n - 1, n, 2**63 - 1] for c, dt in ((2, I64), (3, I32), (4, F64))]
        got, _ = check(window_plan(cols, [(0, 0)], [(1, 0)], outs), what=part)
        if part == "one":
            rows = gw.ordered_rows(got)
            at = {o: i for i, o in enumerate(outs)}
            for f in (LAG, LEAD):
                assert all(r[at[(f, 3, I32, k, 0)]] is None for r in rows for k in (n, 2**63 - 1))    # no such row
                assert sum(r[at[(f, 3, I32, n - 1, 0)]] is not None for r in rows) == 1                # k = n - 1: one row has one
                assert [r[at[(f, 3, I32, 0, 0)]] for r in rows] == cols[3][1][np.argsort(cols[1][1], kind="stable")].tolist()


def around(border, total):
    sizes = [border, border - 1, border + 2]
    return sizes + ([total - sum(sizes)] if total > sum(sizes) else [])


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
@pytest.mark.parametrize("border", [F, 64, F * F, 1024, TILE])
def test_partition_ends_on_and_next_to_every_border(border, shuffle):
    ps = around(border, 3 * TILE + 1)
    cols = table(ps, rng_for("borders", border), True, shuffle)
    outs = [(ROWNO, 0, I64)] + every_function([(-1, -1), (1, 1), (-border, 0), (0, border), (-border - 1, border - 1)], offsets=(1, border - 1, border),
                                              buckets=(2, border), cols=(2, 4), types=(I64, F64))
    got, _ = check(window_plan(cols, [(0, 0)], [(1, 0)], outs), what=border)
    assert [i for i, r in enumerate(gw.ordered_rows(got)) if r[0] == 1] == np.r_[0, np.cumsum(ps)[:-1]].tolist()


def test_ntile_bucket_counts():
    for N in (1, 2, 65, 1000, 3 * TILE + 1):
        rng = rng_for("ntile", N)
        cols = table([N], rng)
        outs = [(NTILE, 0, I64, b, 0) for b in sorted({1, 2, 3, 64, max(N - 1, 1), N, N + 1, 2**40, 2**63 - 1})] + [(COL, 1, I32)]
        got, _ = check(window_plan(cols, [], [(1, 0)], outs), what=N)
        rows = gw.ordered_rows(got)
        assert [r[0] for r in rows] == [1] * N and [r[-2] for r in rows] == list(range(1, N + 1))     # one bucket; more buckets than rows
    rng = rng_for("ntile-parts")
    cols = table(gw.runs(3 * TILE + 1, 700, rng), rng)
    check(window_plan(cols, [(0, DESC)], [(1, 0)], [(NTILE, 0, I64, b, 0) for b in (1, 2, 3, 64, 699, 700, 701, 2**40)]))


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_edge_values_of_every_type_under_every_function(dt):
    """the edge list of tests/test_sort_plan.py (NULL, both zeros, NaNs of either sign and several payloads, the
    infinities, the extremes), every value three times, as partition key and as value"""
    rng = rng_for("frame-edges", dt)
    a, b = gw.edge_column(dt, rng), gw.edge_column(dt, rng)
    n = a[1].shape[0]
    cols = [a, b, (I32, np.arange(n, dtype=np.int32))]
    frames = [(-1, -1), (0, 0), (-2, 0), (0, 3), (UNB_P, UNB_F), (1, UNB_F)]
    outs = [(COL, 0, dt), (COL, 1, dt)] + every_function(frames, offsets=(0, 1, 2), buckets=(2,), cols=(1,), types=(dt,))
    got, _ = check(window_plan(cols, [], [(2, 0)], outs), what=(dt, "order only"))
    rows = gw.ordered_rows(got)
    if dt == F64:
        # LAG 0 / FIRST_VALUE (0, 0) keep -0.0 and every NaN payload; MIN / MAX over the one row canonicalise them
        own = [r[1] for r in rows]
        at = {o: i for i, o in enumerate(outs)}
        assert [r[at[(LAG, 1, dt, 0, 0)]] for r in rows] == own and [r[at[(FIRST, 1, dt, 0, 0)]] for r in rows] == own
        seen = {c[1] & (2**64 - 1) for c in own if c is not None}
        assert {sp.SNAN, sp.NEG_NAN, sp.PAYLOAD_NAN, 1 << 63} <= seen
        for f in (RMIN, RMAX):
            canon = {r[at[(f, 1, dt, 0, 0)]][1] & (2**64 - 1) for r in rows if r[at[(f, 1, dt, 0, 0)]] is not None}
            assert not canon & {sp.SNAN, sp.NEG_NAN, sp.PAYLOAD_NAN, 1 << 63} and wp.CANON_NAN in canon and 0 in canon
    for flags in sp.ALL_FLAGS:
        check(window_plan(cols, [(0, flags)], [(2, flags & DESC)], outs), what=(dt, flags, "partitioned"))


def test_extremes_equal_to_the_identities_wrapping_sums_and_all_null_frames():
    n = 2 * TILE + 11
    rng = rng_for("frame-extremes")
    k = np.sort(rng.integers(0, 5, n)).astype(np.int32)
    i64 = rng.choice(np.array([2**63 - 1, -2**63, 2**62, -1, 0], dtype=np.int64), n)
    i32 = rng.choice(np.array([2**31 - 1, -2**31, 0, -1], dtype=np.int32), n)
    i64[k == 0], i32[k == 0] = 2**63 - 1, 2**31 - 1          # only the maximum: MIN is the maximum, the identity of MIN
    i64[k == 1], i32[k == 1] = -2**63, -2**31                # only the minimum: MAX is the minimum, the identity of MAX
    valid = rng.random(n) >= 0.4
    valid[k == 4] = False                                    # a partition without any value
    valid[(np.arange(n) % 97) < 40] = False                  # runs of 40 NULLs: whole frames without a value
    cols = [(I32, k), (I64, i64, valid), (I32, i32, valid), (I32, np.arange(n, dtype=np.int32))]
    frames = [(-6, 0), (-1, 1), (-70, -1), (UNB_P, 0), (UNB_P, UNB_F), (0, 0)]
    outs = [(COL, 0, I32), (COL, 1, I64)] + every_function(frames, cols=(1, 2), types=(I64, I32))
    got, _ = check(window_plan(cols, [(0, 0)], [(3, 0)], outs))
    rows = gw.ordered_rows(got)
    at = {o[:5]: i + 2 for i, o in enumerate(outs[2:])}
    mn, mx, cnt, sm = at[(RMIN, 1, I64, -6, 0)], at[(RMAX, 1, I64, -6, 0)], at[(RCOUNT, 1, I64, -6, 0)], at[(RSUM, 1, I64, -6, 0)]
    hit = 0
    for r in rows:
        if r[cnt] == 0:
            assert r[mn] is None and r[mx] is None and r[sm] is None
        elif r[0] == 0:
            assert r[mn] == r[mx] == 2**63 - 1
            hit += 1
        elif r[0] == 1:
            assert r[mn] == r[mx] == -2**63
            hit += 1
        assert (r[0] != 4) or r[at[(RMAX, 1, I64, UNB_P, UNB_F)]] is None
    assert hit > 100 and any(r[cnt] == 0 for r in rows if r[0] < 4)
    # seven maxima do not fit: the sum wrapped
    assert any(r[0] == 0 and r[cnt] >= 3 and r[sm] == (r[cnt] * (2**63 - 1) + 2**63) % 2**64 - 2**63 for r in rows)
    check(window_plan(cols, [], [], outs))


# ------------------------------------------------------------------ several frames, key shapes, the launch log
def test_several_frames_of_one_column_share_the_sort_the_scan_and_the_tree():
    n = 2 * TILE + 5
    rng = rng_for("frame-log")
    cols = table(gw.runs(n, 700, rng), rng)
    one = [(RMIN, 2, I64, -6, 0)]
    many = [(RMIN, 2, I64, lo, hi) for lo, hi in FRAMES] + [(RSUM, 2, I64, -6, 0), (RSUM, 2, I64, -29, 0), (RSUM, 2, I64, -6, 0), (RCOUNT, 2, I64, 0, 6),
                                                          (RMAX, 2, I64, -6, 0), (RMAX, 2, I64, -29, 0), (SUM, 2, I64), (MIN, 2, I64)]
    _, ran1 = check(window_plan(cols, [(0, 0)], [(1, 0)], one))
    got, ran = check(window_plan(cols, [(0, 0)], [(1, 0)], many))
    assert launches(ran, "k_sort_") == launches(ran1, "k_sort_") and fam(ran, "k_group_heads") == fam(ran1, "k_group_heads")
    assert ran.get("k_win_scan<8>") == 1 and ran.get("k_win_tails<8>") == 1 and ran.get("k_win_ranks") == 2 and ran1.get("k_win_ranks") == 2
    assert ran.get("k_frame_leaves<8>") == 2 and ran1.get("k_frame_leaves<8>") == 1          # one tree for MIN, one for MAX
    levels = ran.get("k_frame_levels", 0)
    assert levels == 2 * ran1.get("k_frame_levels", 0) and levels == (2 if F == 16 else 0)
    assert ran.get("k_frame_extreme") == len(FRAMES) + 2 and ran.get("k_frame_sum") == 3    # the same (function, column, frame) is one column
    rows = gw.ordered_rows(got)
    assert all(r[len(FRAMES)] == r[len(FRAMES) + 2] for r in rows)


def test_no_keys_partition_keys_only_and_order_keys_only():
    n = TILE + 300
    rng = rng_for("frame-shapes")
    cols = table(gw.runs(n, 50, rng), rng, shuffle=False)
    outs = [(COL, 1, I32), (DENSE, 0, I64)] + every_function([(-6, 0), (1, 3), (UNB_P, UNB_F)])
    got, ran = check(window_plan(cols, [], [], outs), what="no key")
    assert not launches(ran, "k_sort_") and ran.get("k_win_one_head") == 1 and ran.get("k_win_ranks") == 1      # Q is P: one launch serves
    rows = gw.ordered_rows(got)
    assert np.array_equal(np.array([r[0] for r in rows]), cols[1][1])                       # the child's order
    _, ran = check(window_plan(cols, [(0, 0)], [], outs), what="partition only")
    assert ran.get("k_win_ranks") == 1 and not ran.get("k_win_one_head")
    _, ran = check(window_plan(cols, [], [(1, DESC)], outs), what="order only")
    assert ran.get("k_win_ranks") == 2 and ran.get("k_win_one_head") == 1
    # peers: the order among them is the scan's
    tied = [cols[0], (I32, (cols[1][1] // 7).astype(np.int32))] + cols[2:]
    check(window_plan(tied, [(0, 0)], [(1, 0)], outs + [(RANK, 0, I64), (COUNT, 2, I64)]), what="peers")


def test_every_frame_instantiation_is_driven():
    import _elfsyms
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.startswith("k_frame_")}
    cols = sp.key_table(rng_for("frame-matrix"), F**3 + 1 if F == 16 else 2 * TILE + 1, [I32, I64, F64])
    reached = set()
    for p in (window_plan(cols, [(0, 0)], [(1, DESC)], [(LAG, 0, I32, 1, 0), (RMIN, 0, I32, -6, 0), (RMAX, 2, F64, -6, 0), (RSUM, 1, I64, -6, 0)]),
              window_plan(cols, [], [(2, NF)], [(NTILE, 0, I64, 4, 0), (LEAD, 1, I64, 1, 0)])):
        reached |= set(launches(check(p)[1], "k_frame_"))
    assert reached == compiled, sorted(compiled ^ reached)


def test_a_plan_without_the_new_functions_launches_what_it_did():
    n = 2 * TILE + 5
    rng = rng_for("log")                                     # the plan of gw.test_launch_log_one_scan_set_per_distinct_value_column
    cols = gw.laid_out_table(*gw.form_sizes(n, "runs700", "random", rng), rng)
    outs = [(SUM, 2, I64), (MIN, 2, I64), (MAX, 2, I64), (COUNT, 2, I64), (MAX, 3, I32), (MIN, 3, I32), (COUNT, 4, I64), (STAR, 0, I64)]
    p = window_plan(cols, [(0, 0)], [(1, 0)], outs)
    assert pl.plan_to_c(p)[0].nodes[p.root].base_table_id == 0
    _, ran = check(p)
    assert not launches(ran, "k_frame_")
    assert launches(ran, "k_win_") == {"k_win_marks": 1, "k_win_carry": 1, "k_win_ranks": 1, "k_win_tails<8>": 2, "k_win_tails<4>": 1,
                                       "k_win_tail_carry": 3, "k_win_scan<8>": 2, "k_win_scan<4>": 1, "k_win_column": 7}
    # a garbage argument pointer is never read without a function that takes one
    cp, keep = pl.plan_to_c(p)
    cp.nodes[p.root].base_table_id = 0xDEAD0000
    c = gw.context()
    out = C.c_void_p()
    assert c.L.rj_execute(c.h, C.byref(cp), C.byref(out)) == 0
    c.L.rj_result_free(out)
    del keep


# ------------------------------------------------------------------ composition
def _parts_and_unique(rng, n=6_000):
    p = [(I32, rng.integers(0, 40, n).astype(np.int32), rng.random(n) >= 0.05), (I64, rng.permutation(n).astype(np.int64) - n // 2),
         km.payload(rng, I64, n, True)]
    b = [(I32, np.arange(10, 50, dtype=np.int32)), (I32, rng.integers(-50, 50, 40).astype(np.int32))]
    return p, b


COMP = [(LAG, 1, I64, 1, 0), (LEAD, 2, I64, 2, 0), (FIRST, 2, I64, -3, -1), (LAST, 1, I64, 0, UNB_F), (NTILE, 0, I64, 3, 0), (RSTAR, 0, I64, -2, 2),
        (RCOUNT, 2, I64, -6, 0), (RSUM, 2, I64, -6, 0), (RMIN, 2, I64, -6, 0), (RMAX, 1, I64, UNB_P, -1), (COL, 0, I32), (COL, 1, I64), (ROWNO, 0, I64)]


@pytest.mark.parametrize("kind", ["scan", "join", "outer", "select", "sort", "group", "window", "map"])
def test_frames_as_the_root_over_every_kind(kind):
    """column 1 is unique in every child: the order is determined"""
    p, sa, sb = gw._two_scans(*_parts_and_unique(rng_for("frame-over", kind)))
    three = [(0, I32), (1, I64), (2, I64)]
    outs = COMP
    if kind == "scan":
        child = sa
    elif kind == "join":        # the build side's keys are unique: no probe row is doubled
        child = p.new_join_node(False, sa, sb, 0, 0, three)
    elif kind == "outer":
        child = p.new_outer_join_node(False, sa, sb, 0, 0, three)
    elif kind == "select":
        child = p.new_select_node(sa, [("LT", 1, 0), ("IS_NULL", 2), ("OR",)], three)
    elif kind == "sort":
        child = p.new_sort_node(sa, [(1, DESC)], three, limit=4_000)
    elif kind == "group":       # (key, unique, payload) groups are the rows
        child = p.new_group_node(sa, [(1, 0)], [(pl.AGG_MIN, 0, I32), (pl.AGG_KEY, 1, I64), (pl.AGG_MAX, 2, I64)])
    elif kind == "window":
        child = p.new_window_node(sa, [(0, 0)], [(1, 0)], [(COL, 0, I32), (COL, 1, I64), (LAG, 2, I64, 1, 0)])
    else:
        child = p.new_map_node(sa, [("COL", 2), ("COL", 1), ("ADD",), ("OUT",)], [("COL", 0, I32), ("COL", 1, I64), ("EXPR", 0, I64)])
    p.root = p.new_window_node(child, [(0, NF)], [(1, DESC)], outs)
    got, ran = check(p, what=kind)
    assert got.num_rows > 1 and fam(ran, "k_frame_pick") and fam(ran, "k_frame_extreme")


@pytest.mark.parametrize("kind", ["join", "select", "sort", "group", "window", "map", "setop", "select-lead-is-null"])
def test_every_kind_over_frames(kind):
    rng = rng_for("frame-under", kind)
    pcols, _ = _parts_and_unique(rng)
    bcols = [(I64, np.arange(1, 40, dtype=np.int64)), (I32, rng.integers(-50, 50, 39).astype(np.int32))]
    p, sa, sb = gw._two_scans(pcols, bcols)
    w = p.new_window_node(sa, [(0, NF)], [(1, DESC)], [(COL, 0, I32), (COL, 1, I64), (LAG, 1, I64, 1, 0), (NTILE, 0, I64, 5, 0), (RSUM, 2, I64, -6, 0),
                                                       (RMIN, 2, I64, -3, 3), (LEAD, 2, I64, 1, 0)])
    if kind == "join":        # on the bucket number the window produced
        p.root = p.new_join_node(False, w, sb, 3, 0, [(0, I32), (1, I64), (2, I64), (4, I64), (8, I32)])
    elif kind == "select":
        p.root = p.new_select_node(w, [("LEQ", 3, 2)], [(0, I32), (1, I64), (3, I64), (5, I64)])
    elif kind == "select-lead-is-null":
        p.root = p.new_select_node(w, [("IS_NULL", 6)], [(0, I32), (1, I64), (6, I64)])
    elif kind == "sort":
        p.root = p.new_sort_node(w, [(4, DESC), (1, 0)], [(0, I32), (2, I64), (4, I64)], limit=500)
    elif kind == "group":
        p.root = p.new_group_node(w, [(3, 0)], [(pl.AGG_KEY, 3, I64), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_MIN, 2, I64), (pl.AGG_MAX, 5, I64)])
    elif kind == "window":
        p.root = p.new_window_node(w, [(3, 0)], [(1, 0)], [(COL, 3, I64), (COL, 1, I64), (RMAX, 4, I64, -2, 0), (LAG, 2, I64, 2, 0)])
    elif kind == "map":       # x - LAG(x)
        p.root = p.new_map_node(w, [("COL", 1), ("COL", 2), ("SUB",), ("OUT",)], [("COL", 0, I32), ("COL", 1, I64), ("EXPR", 0, I64)])
    else:
        p.root = p.new_setop_node(pl.SET_UNION, w, w, [(0, 0, I32), (2, 2, I64), (3, 3, I64)])
    got, ran = check(p, what=kind)
    assert got.num_rows > 1 and fam(ran, "k_frame_pick")
    if kind == "map":
        assert all(r[2] is None or r[2] < 0 for r in gw.ordered_rows(got))      # descending: every difference is negative
    if kind == "select-lead-is-null":
        assert got.num_rows >= 41


# ------------------------------------------------------------------ fuzz
def fuzz_case(seed):
    rng = rng_for("frame-fuzz", seed)
    n = int(rng.integers(1, 3_000)) if rng.random() < 0.8 else int(rng.integers(3_000, 3 * TILE + 2))
    types = [[I32, I64, F64][int(rng.integers(0, 3))] for _ in range(4)]
    null_p = [0.0, 0.05, 0.5][int(rng.integers(0, 3))]
    card = int(rng.integers(1, n + 1)) if rng.random() < 0.5 else int(rng.integers(1, 40))
    cols = []
    for dt in types:
        v = rng.integers(-(card // 2), card - card // 2, n)
        cols.append((dt, (v * 0.5).astype(np.float64) if dt == F64 else v.astype(km.NP_OF[dt]), rng.random(n) >= null_p))
    edge = sp.key_table(rng, min(n, 16), types, null_p=null_p)
    cols = [(dt, np.concatenate([e[1], v[e[1].shape[0]:]]), np.concatenate([e[2], m[e[2].shape[0]:]])) for (dt, v, m), e in zip(cols, edge)]
    cols.append((I32, rng.permutation(n).astype(np.int32)))                      # column 4: unique
    types = types + [I32]
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, dt) for i, dt in enumerate(types)])
    p.new_input(pl.make_table(cols))
    every = [(i, dt) for i, dt in enumerate(types)]
    child, kind = sc, ["scan", "scan", "scan", "select", "join"][int(rng.integers(0, 5))]
    if kind == "select":
        child = p.new_select_node(sc, [("IS_NOT_NULL", 0), ("IS_NULL", 1), ("OR",)], every)
    elif kind == "join" and types[0] != F64:
        other = p.new_scan_node(0, [(0, types[0])])
        child = p.new_semi_join_node(False, sc, other, 0, 0, every)
    nk = int(rng.integers(0, 5))
    keys = [(int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(nk)]
    n_part = int(rng.integers(0, nk + 1))
    part, order = keys[:n_part], keys[n_part:]
    if child != sc:
        order = order + [(4, int(rng.integers(0, 2)))]                            # not a scan: the order must be determined by the keys
    frames = FRAMES + [tuple(sorted(int(x) for x in rng.integers(-80, 80, 2))) for _ in range(4)]
    outs = fp.frame_outputs(types, frames, rng, offsets=(0, 1, 2, 63, 64, 65, int(rng.integers(0, n + 2)), 2**63 - 1),
                            buckets=(1, 2, 3, 64, int(rng.integers(1, n + 2)), 2**40))
    old = [o for o in wp.all_outputs(types, rng) if o[0] != ROWNO or child == sc][:6]
    outs = [outs[i] if i < len(outs) else old[i - len(outs)] for i in rng.permutation(len(outs) + len(old))]
    p.root = p.new_window_node(child, part, order, outs)
    return p


@pytest.mark.parametrize("block", range(15))
def test_fuzz(block):
    """150 seeded cases, ten per block: schema, key split, flags, functions and frames, NULL rate, run lengths, child kind"""
    rows = 0
    for seed in range(10 * block, 10 * block + 10):
        got, _ = check(fuzz_case(seed), what=seed)
        rows += got.num_rows
    assert rows > 0


# ------------------------------------------------------------------ dirty memory
@pytest.mark.parametrize("part", ["grid", "frames", "values", "fuzz"])
@pytest.mark.parametrize("env", gw.POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env, part):
    """nothing may rely on what the memory held: the block cache hands out filled blocks"""
    if part == "grid":
        for n in (1, F + 1, F * F + 1, 1025, TILE, TILE + 1, 3 * TILE + 1):
            for form in PARTS:
                grid_case(n, form, True, env)
    elif part == "frames":
        for frame in FRAMES:
            grid_case(2 * TILE + 1, "runs700", True, env, frames=[frame])
        rng = rng_for("frame-poison")
        cols = table([TILE + 5], rng)
        check(window_plan(cols, [], [], every_function(GRID_FRAMES, offsets=OFFSETS, buckets=(1, 3, 2**40))), env)
    elif part == "values":
        rng = rng_for("frame-poison-values")
        for dt in (F64, I64, I32):
            a, b = gw.edge_column(dt, rng), gw.edge_column(dt, rng)
            cols = [a, b, (I32, np.arange(a[1].shape[0], dtype=np.int32))]
            check(window_plan(cols, [(0, 0)], [(2, 0)], every_function([(-2, 0), (UNB_P, UNB_F), (1, 2)], cols=(0, 1), types=(dt, dt))), env, what=dt)
    else:
        for seed in range(2_000, 2_020):
            check(fuzz_case(seed), env, what=seed)
    s = gw.context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


# ------------------------------------------------------------------ the error contract
@pytest.mark.parametrize("rows", [5, 0], ids=["rows", "empty-child"])
def test_error_contract(rows):
    """every refusal, also over an empty child: the node is checked before its child's rows are looked at"""
    rng = rng_for("frame-err")
    types = [I32, I64, F64, VC, I32]
    if rows:
        cols = [km.payload(rng, I32, rows, True), km.payload(rng, I64, rows, False), km.payload(rng, F64, rows, True),
                km.payload(rng, VC, rows, False), (I32, rng.integers(0, 10, rows).astype(np.int32))]
    else:
        cols = gw._typed_empty(types)
    bad = lambda outs: gw._error(window_plan(cols, [(0, 0)], [(1, 0)], outs))
    # RJ_ERR_ARG
    for outs, text in (([(9, 1, I64, 0, 0)], UNKNOWN), ([(15, 0, I64, 0, 0)], UNKNOWN), ([(26, 0, I64, 0, 0)], UNKNOWN), ([(200, 0, I64, 0, 0)], UNKNOWN),
                       ([(RSUM, 1, I64, 1, 0)], "bad frame"), ([(RMIN, 1, I64, UNB_F, UNB_F)], "bad frame"), ([(RSTAR, 0, I64, UNB_P, UNB_P)], "bad frame"),
                       ([(FIRST, 1, I64, 0, -1)], "bad frame"), ([(LAST, 0, I32, 5, 4)], "bad frame"), ([(RCOUNT, 2, I64, UNB_F, UNB_P)], "bad frame"),
                       ([(LAG, 1, I64, -1, 0)], "LAG / LEAD"), ([(LEAD, 1, I64, 1, 1)], "LAG / LEAD"), ([(LAG, 1, I64, UNB_P, 0)], "LAG / LEAD"),
                       ([(NTILE, 0, I64, 0, 0)], "NTILE"), ([(NTILE, 0, I64, -4, 0)], "NTILE"), ([(NTILE, 0, I64, 2, 2)], "NTILE"),
                       ([(NTILE, 1, I64, 2, 0)], "NTILE takes no column"), ([(RSTAR, 2, I64, -1, 0)], "COUNT(*) takes no column"),
                       ([(LAG, 5, I64, 1, 0)], "output attr out of range"), ([(RMAX, 99, I64, -1, 0)], "output attr out of range"),
                       ([(LAG, 1, I32, 1, 0)], "declared type"), ([(LEAD, 2, I64, 1, 0)], "declared type"), ([(FIRST, 0, I64, -1, 0)], "declared type"),
                       ([(LAST, 2, I32, -1, 0)], "declared type"), ([(NTILE, 0, I32, 2, 0)], "declared type"), ([(RSTAR, 0, I32, -1, 0)], "declared type"),
                       ([(RCOUNT, 2, F64, -1, 0)], "declared type"), ([(RSUM, 0, I32, -1, 0)], "declared type"), ([(RMIN, 0, I64, -1, 0)], "declared type"),
                       ([(RMAX, 2, I64, -1, 0)], "declared type")):
        code, msg = bad(outs)
        assert code == ARG and text in msg, (outs, msg)
    # a function that takes an argument, and none given
    p = window_plan(cols, [(0, 0)], [(1, 0)], [(COL, 0, I32), (LAG, 1, I64, 1, 0)])
    cp, keep = pl.plan_to_c(p)
    cp.nodes[p.root].base_table_id = 0
    c = gw.context()
    out = C.c_void_p()
    assert c.L.rj_execute(c.h, C.byref(cp), C.byref(out)) == ARG and b"RJ_WINDOW_ARGS is NULL" in c.L.rj_last_error(c.h)
    del keep
    # RJ_ERR_UNSUPPORTED
    for func in (LAG, LEAD, FIRST, LAST, RCOUNT, RSUM, RMIN, RMAX):
        code, msg = bad([(func, 3, I64 if func in (RCOUNT, RSUM) else VC, 0, 0)])
        assert code == UNSUPPORTED and "VARCHAR" in msg, (func, msg)
    code, msg = bad([(RSUM, 2, I64, -6, 0)])
    assert code == UNSUPPORTED and "FP64" in msg and "SUM" in msg
    # the extremes of every argument are fine, and a VARCHAR column passes through next to them
    got, _ = check(window_plan(cols, [(0, 0)], [(4, 0), (1, 0)], [(COL, 3, VC), (LAG, 1, I64, 2**63 - 1, 0), (LEAD, 2, F64, 0, 0), (NTILE, 0, I64, 2**63 - 1, 0),
                                                                    (RSTAR, 0, I64, UNB_P, UNB_F), (RMIN, 2, F64, UNB_P, UNB_P + 1),
                                                                    (RMAX, 0, I32, UNB_F - 1, UNB_F), (FIRST, 0, I32, -2**63 + 1, 2**63 - 2)]))
    assert got.num_rows == rows


def test_empty_child_gives_typed_columns_without_pages():
    outs = [(LAG, 2, F64, 1, 0), (NTILE, 0, I64, 3, 0), (RMIN, 1, I64, -6, 0), (COL, 3, VC), (RSTAR, 0, I64, -1, 1), (RSUM, 0, I64, 0, 0), (LAST, 0, I32, 0, 5)]
    got, ran = check(window_plan(gw._typed_empty([I32, I64, F64, VC]), [(0, 0)], [(2, DESC)], outs))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [F64, I64, I64, VC, I64, I64, I32]
    assert all(c.pages.shape[0] == 0 for c in got.columns) and not launches(ran, "k_frame_") and not launches(ran, "k_win_")
