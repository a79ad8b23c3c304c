"""Window nodes (RJ_NODE_WINDOW) on the device, through the C-ABI, against the numpy reference
tests/_windowref.py (tests/test_window_plan.py ties it to a row-at-a-time walk on the CPU).  Every
result column is read by the strict page reader tests/_pagecheck.py first.  Everything is exact:
integers, and FP64 by bit pattern.

With a SCAN child the whole result is determined (ties are stable with respect to the scan's order), so
it is compared row by row IN ORDER.  Over any other child, and under any other node, the result is
compared as a multiset, and ROW_NUMBER is only asked for where the order keys are unique within a
partition: which peer gets which row number is unspecified there.

Device path: the sort's kernels order the rows by (partition keys, order keys), k_group_heads marks the
partition heads (P) and the peer-group heads (Q), and the k_win_* kernels work quarter by quarter (a
quarter = the 1024 positions of one wave of a 4096-position tile, 64 per item): the sizes and layouts
below put partition ends and peer-group ends on and next to every one of these borders.
RJ_TUNE_WIN_GRID caps the quarter entries the carry kernels' one workgroup takes per step, so that a
small input takes several steps.  The one limit no quick test can reach is the row limit (2^32 - 16 child rows)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _pagecheck as pc
import _windowref
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
import test_sort_plan as sp
import test_window_plan as wp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
COL, ROWNO, RANK, DENSE, STAR, COUNT, SUM, MIN, MAX = wp.COL, wp.ROWNO, wp.RANK, wp.DENSE, wp.STAR, wp.COUNT, wp.SUM, wp.MIN, wp.MAX
_HPP = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
TILE = int(re.search(r"constexpr int GROUP_TILE\s*=\s*(\d+);", _HPP).group(1))
assert TILE == 4096 and "constexpr int WIN_QUARTER = GROUP_TILE / GROUP_WAVES;" in _HPP
ROWS32, ROWS64 = (int(re.search(rf"constexpr uint32_t {n}\s*=\s*(\d+);", _HPP).group(1)) for n in ("ROWS32", "ROWS64"))
POISON = [{"RJ_DEBUG_POISON": str(m)} for m in (0x15A, 0x1FF)]
rng_for, window_plan, ALL_FLAGS = sp.rng_for, wp.window_plan, sp.ALL_FLAGS
fam = lambda ran, family: {n: c for n, c in ran.items() if n.split("<")[0] == family}
launches = lambda ran, prefix: {n: c for n, c in ran.items() if n.startswith(prefix)}
SCAN_SET = ("k_win_tails", "k_win_tail_carry", "k_win_scan")
ARG, UNSUPPORTED = 1, 5

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
    return _windowref.decoded_rows([c.type for c in got.columns], dec, got.num_rows)


def _any_order(rows):
    cell = lambda v: (1, 0) if v is None else (0, v[1] if isinstance(v, tuple) else v)
    return sorted(rows, key=lambda r: tuple(cell(v) for v in r))


def check(p, env=None, what="", **kw):
    """Run plan p against the reference: a root window node over a scan row by row in order, anything
    else as a multiset."""
    got, ran = run(p, env, **kw)
    n, cols = _windowref.evaluate(p)
    d = p.nodes[p.root].data
    assert got.num_rows == n, (what, got.num_rows, n)
    assert [c.type for c in got.columns] == [c[0] for c in cols], what
    rows, want = ordered_rows(got), _windowref.rel_rows(cols, n)
    if isinstance(d, pl.WindowNode) and isinstance(p.nodes[d.child].data, pl.ScanNode):
        assert rows == want, what
    else:
        assert _any_order(rows) == _any_order(want), what
    return got, ran


# ------------------------------------------------------------------ row counts, partitions, peers
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 1, ROWS64 - 1, ROWS64 + 1, ROWS32 - 1,
         ROWS32 + 1]
PARTS = ["one", "each", "runs3", "runs700"]
PEERS = ["distinct", "tied", "random"]
# all eight functions and two passed-through columns: a nullable INT64 (2), a paged INT32 (3), a nullable FP64 (4)
OUTS = [(COL, 0, I32), (ROWNO, 0, I64), (RANK, 0, I64), (DENSE, 0, I64), (STAR, 0, I64), (COUNT, 2, I64), (SUM, 2, I64), (MIN, 2, I64),
        (MAX, 3, I32), (MIN, 4, F64), (COL, 2, I64)]


def runs(n, mean, rng):
    sizes, total = [], 0
    while total < n:
        sizes.append(min(int(rng.integers(1, 2 * mean)), n - total))
        total += sizes[-1]
    return sizes


def laid_out_table(part_sizes, peer_sizes, rng, shuffle=True):
    """an INT32 partition key whose partitions have part_sizes in the order of the key, an INT32 order key
    whose runs over the sorted order have peer_sizes (a partition end ends a peer group anyway), a
    nullable INT64 value, a paged INT32 value and a nullable FP64 value"""
    part_sizes, peer_sizes = np.asarray(part_sizes, dtype=np.int64), np.asarray(peer_sizes, dtype=np.int64)
    n = int(part_sizes.sum())
    assert int(peer_sizes.sum()) == n
    at = rng.permutation(n) if shuffle else np.arange(n)
    pk = np.repeat(np.arange(part_sizes.shape[0]) * 3 - 7, part_sizes).astype(np.int32)[at]
    ok = np.repeat(np.arange(peer_sizes.shape[0]) * 5 - 11, peer_sizes).astype(np.int32)[at]
    return [(I32, pk), (I32, ok), (I64, rng.integers(-2**40, 2**40, n), rng.random(n) >= 0.3), (I32, rng.integers(-2**31, 2**31, n).astype(np.int32)),
            (F64, rng.integers(-50, 50, n) * 0.25, rng.random(n) >= 0.2)]


def form_sizes(n, part, peers, rng):
    ps = {"one": [n], "each": [1] * n, "runs3": runs(n, 3, rng), "runs700": runs(n, 700, rng)}[part]
    qs = {"distinct": [1] * n, "tied": [n], "random": runs(n, 4, rng)}[peers]
    return ps, qs


def grid_case(n, part, peers, env=None):
    rng = rng_for("grid", n, part, peers)
    cols = laid_out_table(*form_sizes(n, part, peers, rng), rng)
    return check(window_plan(cols, [(0, 0)], [(1, 0)], OUTS), env, what=(n, part, peers))


@pytest.mark.parametrize("n", SIZES)
def test_size_grid(n):
    for part in PARTS:
        for peers in PEERS:
            got, ran = grid_case(n, part, peers)
            assert got.num_rows == n and fam(ran, "k_win_ranks") and sum(fam(ran, "k_win_scan").values()) == 3


def around(border, total):
    """run lengths whose ends fall exactly on a multiple of `border`, one before the next one and one after the one after"""
    sizes = [border, border - 1, border + 2]                 # ends: border, 2 border - 1, 3 border + 1
    return sizes + [total - sum(sizes)]


def whole(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


LAYOUTS = {}
for _b in (64, 1024, TILE):
    _n = 4 * TILE + 500
    LAYOUTS[f"partition-ends-around-{_b}"] = (around(_b, _n), whole(_n, 3))
    LAYOUTS[f"peer-groups-end-around-{_b}"] = ([_n], around(_b, _n))
LAYOUTS["one-partition-over-three-tiles-peers-straddle"] = ([3 * TILE + 100], whole(3 * TILE + 100, 1000))
LAYOUTS["a-tile-without-a-partition-head"] = ([100, 2 * TILE + 3000, 50], whole(2 * TILE + 3150, 7))
LAYOUTS["a-tile-without-any-head"] = ([100, 2 * TILE + 3000, 50], [100, 2 * TILE + 3000, 50])
LAYOUTS["a-quarter-each"] = ([1024] * 9 + [3], [512] * 18 + [3])
LAYOUTS["single-rows-around-a-long-run"] = ([1] * 70 + [2 * TILE] + [1] * 70, [1] * 70 + [TILE, TILE] + [1] * 70)


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_partition_and_peer_group_ends_on_item_quarter_and_tile_borders(layout, shuffle):
    ps, qs = LAYOUTS[layout]
    assert all(s > 0 for s in ps) and all(s > 0 for s in qs)
    cols = laid_out_table(ps, qs, rng_for("layout", layout), shuffle)
    got, _ = check(window_plan(cols, [(0, 0)], [(1, 0)], OUTS), what=layout)
    rows = ordered_rows(got)
    # ROW_NUMBER restarts exactly where the partitions were laid out to begin
    assert [i for i, r in enumerate(rows) if r[1] == 1] == np.r_[0, np.cumsum(ps)[:-1]].tolist()


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_the_carry_kernels_take_several_steps(grid):
    """n = 5 tiles + 1 rows = 21 quarters, 1, 2 or 3 of them per step of the carry kernels: the scan inside a
    step and the total carried from step to step both take part"""
    env = {"RJ_TUNE_WIN_GRID": str(grid)}
    n = 5 * TILE + 1
    for part in PARTS:
        for peers in PEERS:
            grid_case(n, part, peers, env)
    for layout in ("one-partition-over-three-tiles-peers-straddle", "a-tile-without-any-head", "a-tile-without-a-partition-head"):
        ps, qs = LAYOUTS[layout]
        extra = n - sum(ps)
        cols = laid_out_table(list(ps) + [extra], list(qs) + [extra], rng_for("walk", layout, grid))
        check(window_plan(cols, [(0, DESC)], [(1, DESC)], OUTS), env, what=(layout, grid))


@pytest.mark.parametrize("env", [None, {"RJ_TUNE_WIN_GRID": "100"}], ids=["one-step", "three-steps-of-two-waves"])
def test_three_hundred_thousand_rows(env):
    """293 quarters: one step of the carry kernels over five waves, or three steps of 100 entries"""
    n = 300_000
    rng = rng_for("large")
    cols = laid_out_table(*form_sizes(n, "runs700", "random", rng), rng)
    got, _ = check(window_plan(cols, [(0, NF)], [(1, DESC)], OUTS), env)
    assert got.num_rows == n


# ------------------------------------------------------------------ values
def edge_column(dt, rng, times=3):
    bits = [b for _, b in sp.EDGES[dt]] * times
    null = [v is None for v, _ in sp.EDGES[dt]] * times
    at = rng.permutation(len(bits))
    raw = np.array(bits, dtype=np.uint64)[at]
    vals = raw.astype(np.uint32).view(np.int32) if dt == I32 else raw.view(km.NP_OF[dt])
    return (dt, vals, ~np.array(null)[at])


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_edge_values_of_every_key_type_under_every_flag(dt, flags):
    """the edge list of tests/test_sort_plan.py (NULL, both zeros, NaNs of either sign and several payloads,
    the infinities, the extremes), every value three times, as partition key, as order key and as value"""
    rng = rng_for("edges", dt, flags)
    a, b = edge_column(dt, rng), edge_column(dt, rng)
    cols = [a, b, (I32, np.arange(a[1].shape[0], dtype=np.int32))]
    outs = [(COL, 0, dt), (COL, 1, dt), (ROWNO, 0, I64), (RANK, 0, I64), (DENSE, 0, I64), (STAR, 0, I64), (COUNT, 1, I64), (MIN, 1, dt), (MAX, 1, dt),
            (MIN, 2, I32)]
    got, _ = check(window_plan(cols, [(0, flags)], [(1, flags)], outs), what=(dt, flags, "both"))
    rows = ordered_rows(got)
    distinct = len(sp.EDGES[dt]) - (4 if dt == F64 else 0)      # -0.0 = +0.0, four NaNs are one: ONE partition each
    assert sum(1 for r in rows if r[2] == 1) == distinct
    got, _ = check(window_plan(cols, [], [(0, flags)], outs), what=(dt, flags, "order only"))
    assert max(r[4] for r in ordered_rows(got)) == distinct     # ... and one peer group each
    check(window_plan(cols, [(1, flags)], [], outs), what=(dt, flags, "partition only"))


def test_every_null_pattern_over_two_nullable_partition_keys():
    rng = rng_for("nullpat")
    n = 3_000
    cols = [(I32, rng.integers(0, 3, n).astype(np.int32), rng.random(n) >= 0.4), (I64, rng.integers(0, 3, n), rng.random(n) >= 0.4),
            (I64, rng.integers(-99, 99, n), rng.random(n) >= 0.5)]
    for f0 in ALL_FLAGS:
        for f1 in (0, DESC | NF):
            got, _ = check(window_plan(cols, [(0, f0), (1, f1)], [(2, 0)], [(COL, 1, I64), (COL, 0, I32), (ROWNO, 0, I64), (SUM, 2, I64), (COL, 2, I64)]),
                           what=(f0, f1))
            assert sum(1 for r in ordered_rows(got) if r[2] == 1) == 16      # (NULL, x), (x, NULL) and (NULL, NULL) are partitions of their own


def test_zeros_and_nans_are_peers_and_one_partition():
    nan = lambda b: np.array([b], dtype=np.uint64).view(np.float64)[0]
    v = np.array([0.0, -0.0, nan(sp.QNAN), nan(sp.SNAN), nan(sp.NEG_NAN), nan(sp.PAYLOAD_NAN), 1.0, -0.0, 0.0, np.inf] * 30)
    n = v.shape[0]
    cols = [(F64, v), (I32, np.arange(n, dtype=np.int32)), (I32, np.zeros(n, dtype=np.int32))]
    outs = [(COL, 0, F64), (COL, 1, I32), (ROWNO, 0, I64), (RANK, 0, I64), (DENSE, 0, I64), (STAR, 0, I64), (MAX, 0, F64), (MIN, 0, F64)]
    got, _ = check(window_plan(cols, [(2, 0)], [(0, 0)], outs))             # as peers
    rows = ordered_rows(got)
    assert [r[5] for r in rows[:120]] == [120] * 120 and rows[0][7] == ("f64", 0) and rows[-1][6] == ("f64", wp.CANON_NAN)
    assert {r[0] for r in rows[:120]} == {("f64", 0), ("f64", -2**63)}     # passed through with their own bits
    assert [r[4] for r in rows[-120:]] == [4] * 120 and [r[3] for r in rows[-120:]] == [181] * 120
    got, _ = check(window_plan(cols, [(0, DESC)], [(1, DESC)], outs))       # as one partition
    rows = ordered_rows(got)
    assert [r[2] for r in rows[:120]] == list(range(1, 121)) and [r[1] for r in rows[:120]] == sorted([r[1] for r in rows[:120]], reverse=True)


def test_sums_wrap_and_extremes_are_not_sentinels():
    n = 2 * TILE + 11
    rng = rng_for("extremes")
    k = rng.integers(0, 5, n).astype(np.int32)
    i64 = rng.choice(np.array([2**63 - 1, -2**63, 2**62, -1, 0], dtype=np.int64), n)
    i32 = rng.choice(np.array([2**31 - 1, -2**31, 0, -1], dtype=np.int32), n)
    i64[k == 0], i32[k == 0] = 2**63 - 1, 2**31 - 1          # a partition of only the maximum: MIN is the maximum
    i64[k == 1], i32[k == 1] = -2**63, -2**31                # ... of only the minimum: MAX is the minimum
    cols = [(I32, k), (I64, i64, rng.random(n) >= 0.1), (I32, i32, rng.random(n) >= 0.1), (I32, rng.permutation(n).astype(np.int32))]
    outs = [(COL, 0, I32), (SUM, 1, I64), (MIN, 1, I64), (MAX, 1, I64), (SUM, 2, I64), (MIN, 2, I32), (MAX, 2, I32), (COUNT, 1, I64)]
    got, _ = check(window_plan(cols, [(0, 0)], [(3, 0)], outs))
    rows = ordered_rows(got)
    for r in rows:
        if r[0] == 0 and r[7]:
            assert r[2] == r[3] == 2**63 - 1
        if r[0] == 1 and r[7]:
            assert r[2] == r[3] == -2**63
    assert abs(int(i64[(k == 0) & cols[1][2]].astype(object).sum())) > 2**63     # the true sum does not fit: it wrapped
    check(window_plan(cols, [(0, 0)], [], outs))
    check(window_plan(cols, [], [], outs))


def test_running_value_goes_from_null_to_a_value_and_partitions_without_any_value():
    rng = rng_for("nulls")
    n = 3 * TILE + 77
    k = rng.integers(0, 9, n).astype(np.int32)
    o = rng.permutation(n).astype(np.int32)
    valid = rng.random(n) >= 0.3
    valid[k == 4] = False                                    # all-NULL in this partition only
    first = np.zeros(n, bool)
    for x in range(9):                                       # every partition begins with NULLs: its 40 lowest order keys
        at = np.flatnonzero(k == x)
        first[at[np.argsort(o[at])[:40]]] = True
    valid &= ~first
    cols = [(I32, k), (I32, o), (I64, rng.integers(-2**40, 2**40, n), valid), (F64, rng.integers(-9, 9, n) * 0.5, valid)]
    outs = [(COL, 0, I32), (ROWNO, 0, I64), (COUNT, 2, I64), (SUM, 2, I64), (MIN, 2, I64), (MAX, 3, F64), (MIN, 3, F64)]
    got, _ = check(window_plan(cols, [(0, 0)], [(1, 0)], outs))
    rows = ordered_rows(got)
    assert all(r[3] is None and r[4] is None and r[5] is None and r[2] == 0 for r in rows if r[1] <= 40 or r[0] == 4)
    assert all(r[3] is not None for r in rows if r[0] != 4 and r[2] > 0) and any(r[2] > 0 for r in rows)
    got, _ = check(window_plan(cols, [(0, 0)], [], outs[:1] + outs[2:]))
    assert {r[0] for r in ordered_rows(got) if r[2] is None} == {4}


# ------------------------------------------------------------------ key shapes
def test_no_key_at_all_launches_no_sort_kernel():
    rng = rng_for("nokey")
    n = 2 * TILE + 9
    cols = laid_out_table([n], [n], rng)
    got, ran = check(window_plan(cols, [], [], OUTS))
    rows = ordered_rows(got)
    assert not launches(ran, "k_sort_") and not fam(ran, "k_group_heads") and ran.get("k_win_one_head") == 1
    assert [r[1] for r in rows] == list(range(1, n + 1)) and {r[4] for r in rows} == {n} and {r[2] for r in rows} == {1}
    assert np.array_equal(np.array([r[0] for r in rows]), cols[0][1])       # the child's order


def test_partition_keys_only_order_keys_only_and_three_plus_five_keys():
    rng = rng_for("shapes")
    n = 5_000
    types = [I32, I64, F64, I32, I64, F64, I32, I64]
    cols = [(dt, rng.integers(0, 2, n).astype(km.NP_OF[dt]), rng.random(n) >= 0.1) for dt in types] + [(I64, rng.integers(-2**62, 2**62, n))]
    outs = [(COL, c, types[c]) for c in range(8)] + [(ROWNO, 0, I64), (RANK, 0, I64), (DENSE, 0, I64), (STAR, 0, I64), (SUM, 8, I64), (MAX, 8, I64)]
    keys = [(int(c), int(rng.integers(0, 4))) for c in rng.permutation(8)]
    _, ran = check(window_plan(cols, keys[:3], keys[3:], outs), what="3 + 5")
    assert sum(fam(ran, "k_sort_encode").values()) == 8 and sum(fam(ran, "k_group_heads").values()) == 8
    _, ran = check(window_plan(cols, keys[:2], [], outs), what="partition only")
    assert sum(fam(ran, "k_group_heads").values()) == 2 and not ran.get("k_win_one_head")
    _, ran = check(window_plan(cols, [], keys[:2], outs), what="order only")
    assert sum(fam(ran, "k_group_heads").values()) == 2 and ran.get("k_win_one_head") == 1


def test_a_column_in_both_lists_a_repeated_key_and_a_constant_key():
    cols = sp.key_table(rng_for("twice"), 5_000, sp.TYPES, domain=4) + [(I64, np.full(5_000, 77))]
    types = sp.TYPES + [I64]
    outs = wp.all_outputs(types)
    a, ran = check(window_plan(cols, [(1, 0), (2, 0)], [(1, DESC), (3, 0), (3, DESC)], outs))
    assert sum(fam(ran, "k_sort_encode").values()) == 3 and sum(fam(ran, "k_group_heads").values()) == 3
    b, _ = run(window_plan(cols, [(1, 0), (2, 0)], [(3, 0)], outs))
    assert ordered_rows(a) == ordered_rows(b)
    # a key column whose values are all equal: every pass is skipped, the child's order stays
    got, ran = check(window_plan(cols, [(5, DESC)], [(5, 0)], outs))
    assert fam(ran, "k_sort_encode") and not fam(ran, "k_sort_scatter") and not fam(ran, "k_sort_count")
    assert [r[0] for r in ordered_rows(got)] == list(range(1, 5_001))


# ------------------------------------------------------------------ outputs
def test_functions_only_pass_through_only_and_a_column_repeated():
    rng = rng_for("outs")
    n = TILE + 300
    cols = laid_out_table(*form_sizes(n, "runs3", "random", rng), rng)
    _, ran = check(window_plan(cols, [(0, 0)], [(1, 0)], [(DENSE, 0, I64), (MAX, 2, I64)]))
    assert sum(fam(ran, "k_win_scan").values()) == 1
    got, ran = check(window_plan(cols, [(0, 0)], [(1, 0)], [(COL, 3, I32), (COL, 2, I64), (COL, 4, F64)]))
    assert not launches(ran, "k_win_") and not fam(ran, "k_group_heads") and fam(ran, "k_sort_scatter")      # a sort and nothing else
    got, ran = check(window_plan(cols, [(0, 0)], [(1, 0)], [(COL, 2, I64), (SUM, 2, I64), (COL, 2, I64), (SUM, 2, I64), (RANK, 0, I64), (RANK, 0, I64)]))
    rows = ordered_rows(got)
    assert all(r[0] == r[2] and r[1] == r[3] and r[4] == r[5] for r in rows) and ran.get("k_win_column") == 1


@pytest.mark.parametrize("env", [{}, {"RJ_TUNE_VARCHAR_DEV": "1"}], ids=["host-encoder", "device-encoder"])
def test_varchar_and_nullable_columns_pass_through(env):
    rng = rng_for("varchar")
    n = 3_000
    strings = [None if i % 11 == 0 else b"s%d" % (i % 301) * (1 + i % 4) for i in range(n)]
    cols = [(I32, rng.integers(0, 40, n).astype(np.int32), rng.random(n) >= 0.1), (VC, strings), km.payload(rng, F64, n, True),
            (I32, rng.permutation(n).astype(np.int32))]
    outs = [(COL, 1, VC), (ROWNO, 0, I64), (COL, 2, F64), (COL, 0, I32), (COUNT, 2, I64), (COL, 1, VC)]
    got, _ = check(window_plan(cols, [(0, NF)], [(3, DESC)], outs), env or None)
    assert got.num_rows == n
    check(window_plan(cols, [], [], outs), env or None)


def test_launch_log_one_scan_set_per_distinct_value_column():
    n = 2 * TILE + 5
    rng = rng_for("log")
    cols = laid_out_table(*form_sizes(n, "runs700", "random", rng), rng)
    outs = [(SUM, 2, I64), (MIN, 2, I64), (MAX, 2, I64), (COUNT, 2, I64), (MAX, 3, I32), (MIN, 3, I32), (COUNT, 4, I64), (STAR, 0, I64)]
    _, ran = check(window_plan(cols, [(0, 0)], [(1, 0)], outs))
    assert ran.get("k_win_tails<8>") == 2 and ran.get("k_win_tails<4>") == 1 and ran.get("k_win_scan<8>") == 2 and ran.get("k_win_scan<4>") == 1
    assert ran.get("k_win_tail_carry") == 3 and ran.get("k_win_column") == 7
    assert ran.get("k_win_marks") == 1 and ran.get("k_win_carry") == 1 and ran.get("k_win_ranks") == 1
    # a ranking-only node, and COUNT(*): no column is read
    _, ran = check(window_plan(cols, [(0, 0)], [(1, 0)], [(ROWNO, 0, I64), (RANK, 0, I64), (DENSE, 0, I64), (STAR, 0, I64)]))
    assert not any(fam(ran, f) for f in SCAN_SET) and not fam(ran, "k_win_column")
    assert ran.get("k_win_ranks") == 1


# ------------------------------------------------------------------ composition
def _pb(rng, n=6_000):
    p = [(I32, rng.integers(0, 900, n).astype(np.int32), rng.random(n) >= 0.05), km.payload(rng, I64, n, True)]
    b = [(I32, rng.integers(400, 1_400, n // 2).astype(np.int32), rng.random(n // 2) >= 0.05), (I32, rng.integers(-50, 50, n // 2).astype(np.int32))]
    return p, b


def _two_scans(pcols, bcols):
    p = pl.Plan()
    sa = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(pcols)])
    sb = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(bcols)])
    p.new_input(pl.make_table(pcols))
    p.new_input(pl.make_table(bcols))
    return p, sa, sb


ALL4 = [(0, I32), (1, I64), (2, I32), (3, I32)]
AGG3 = [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_SUM, 1, I64)]


@pytest.mark.parametrize("kind", ["scan", "join", "outer", "select", "sort", "agg", "group"])
def test_window_as_the_root_over_every_kind(kind):
    """paged and nullable columns of a scan read in place, dense columns of a join, ...; no ROW_NUMBER: the
    order keys tie"""
    p, sa, sb = _two_scans(*_pb(rng_for("over", kind)))
    if kind == "scan":
        child, types = sa, [I32, I64]
    elif kind == "join":
        child, types = p.new_join_node(False, sa, sb, 0, 0, ALL4), [I32, I64, I32, I32]
    elif kind == "outer":
        child, types = p.new_outer_join_node(True, sa, sb, 0, 0, ALL4), [I32, I64, I32, I32]
    elif kind == "select":
        child, types = p.new_select_node(sa, [("LT", 1, 0), ("IS_NULL", 1), ("OR",)], ALL4[:2]), [I32, I64]
    elif kind == "sort":
        child, types = p.new_sort_node(sa, [(1, DESC)], ALL4[:2], limit=4_000), [I32, I64]
    elif kind == "agg":
        child, types = p.new_agg_node(sa, 0, AGG3), [I32, I64, I64]
    else:
        child, types = p.new_group_node(sa, [(0, DESC)], [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_MAX, 1, I64)]), [I32, I64, I64]
    last = len(types) - 1
    part, order = ([(1, 0)], [(last, NF | DESC)]) if kind in ("agg", "group") else ([(0, 0)], [(last, NF | DESC)])
    outs = [o for o in wp.all_outputs(types) if o[0] != ROWNO or kind == "scan"]
    p.root = p.new_window_node(child, part, order, outs)
    got, ran = check(p, what=kind)
    assert got.num_rows > 1 and fam(ran, "k_win_ranks") and fam(ran, "k_win_scan")


@pytest.mark.parametrize("kind", ["join", "select", "sort", "group", "window"])
def test_every_kind_over_a_window(kind):
    rng = rng_for("under", kind)
    n = 6_000
    pcols = [(I32, rng.integers(0, 300, n).astype(np.int32), rng.random(n) >= 0.05), (I64, rng.permutation(n).astype(np.int64) - 3_000)]
    bcols = [(I64, np.arange(1, 40, dtype=np.int64)), (I32, rng.integers(-50, 50, 39).astype(np.int32))]
    p, sa, sb = _two_scans(pcols, bcols)
    # the order key is unique: ROW_NUMBER is determined
    w = p.new_window_node(sa, [(0, NF)], [(1, DESC)], [(COL, 0, I32), (COL, 1, I64), (ROWNO, 0, I64), (DENSE, 0, I64), (SUM, 1, I64)])
    if kind == "join":        # on the rank column the window produced
        p.root = p.new_join_node(False, w, sb, 2, 0, [(0, I32), (1, I64), (2, I64), (4, I64), (6, I32)])
    elif kind == "select":    # top-3 per partition
        p.root = p.new_select_node(w, [("LEQ", 2, 3)], [(0, I32), (1, I64), (2, I64)])
    elif kind == "sort":
        p.root = p.new_sort_node(w, [(4, DESC), (2, 0), (0, 0)], [(0, I32), (2, I64), (4, I64)], limit=500)
    elif kind == "group":     # by DENSE_RANK
        p.root = p.new_group_node(w, [(3, 0)], [(pl.AGG_KEY, 3, I64), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_MIN, 1, I64), (pl.AGG_MAX, 4, I64)])
    else:                     # a second window over the first one's rank
        p.root = p.new_window_node(w, [(2, 0)], [(1, 0)], [(COL, 2, I64), (COL, 0, I32), (ROWNO, 0, I64), (MAX, 4, I64), (STAR, 0, I64)])
    got, ran = check(p, what=kind)
    assert got.num_rows > 1 and fam(ran, "k_win_ranks")
    if kind == "select":
        k, v = pcols[0][1], pcols[0][2]
        assert got.num_rows == sum(min(3, int(((k == x) & v).sum())) for x in np.unique(k[v])) + min(3, int((~v).sum()))


def test_same_plan_twice_on_one_context_and_on_two_devices():
    cols = sp.key_table(rng_for("twice"), 10_000, sp.TYPES, domain=5)
    p = window_plan(cols, [(2, DESC), (0, NF)], [(1, 0)], wp.all_outputs(sp.TYPES))
    a, _ = run(p)
    b, _ = run(p)
    assert a.num_rows == b.num_rows == 10_000 and ordered_rows(a) == ordered_rows(b)
    got, _ = check(p, devices=[0, 0])                       # a multi-device context runs the plan on its first device
    ctx = context(devices=[0, 0])
    tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
    try:
        with pytest.raises(capi.RjError) as e:
            ctx.execute_sharded(p, tables)
        assert e.value.code == UNSUPPORTED and "RJ_NODE_WINDOW" in str(e.value)
    finally:
        for row in tables:
            for t in row:
                t.release()


# ------------------------------------------------------------------ fuzz
def fuzz_case(seed):
    rng = rng_for("fuzz", seed)
    n = int(rng.integers(1, 3_000)) if rng.random() < 0.75 else int(rng.integers(3_000, 20_001))
    types = [[I32, I64, F64][int(rng.integers(0, 3))] for _ in range(4)]
    null_p = [0.0, 0.05, 0.5][int(rng.integers(0, 3))]
    card = int(rng.integers(1, n + 1)) if rng.random() < 0.5 else int(rng.integers(1, 40))   # run lengths: n / card
    cols = []
    for dt in types:
        v = rng.integers(-(card // 2), card - card // 2, n)
        cols.append((dt, (v * 0.5).astype(np.float64) if dt == F64 else v.astype(km.NP_OF[dt]), rng.random(n) >= null_p))
    edge = sp.key_table(rng, min(n, 16), types, null_p=null_p)                    # ... and the edge values of every type
    cols = [(dt, np.concatenate([e[1], v[e[1].shape[0]:]]), np.concatenate([e[2], m[e[2].shape[0]:]])) for (dt, v, m), e in zip(cols, edge)]
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, dt) for i, dt in enumerate(types)])
    p.new_input(pl.make_table(cols))
    every = [(i, dt) for i, dt in enumerate(types)]
    child, kind = sc, ["scan", "scan", "select", "join", "group"][int(rng.integers(0, 5))]
    if kind == "select":
        child = p.new_select_node(sc, [("IS_NOT_NULL", 0), ("IS_NULL", 1), ("OR",)], every)
    elif kind == "join" and types[0] != F64:
        other = p.new_scan_node(0, [(0, types[0])])
        child = p.new_semi_join_node(False, sc, other, 0, 0, every)
    elif kind == "group":
        child = p.new_group_node(sc, [(0, 0), (1, 0)], [(pl.AGG_KEY, 0, types[0]), (pl.AGG_KEY, 1, types[1]), (pl.AGG_COUNT_STAR, 0, I64),
                                                         (pl.AGG_MAX, 2, types[2])])
        types = [types[0], types[1], I64, types[2]]
    nk = int(rng.integers(0, 5))
    keys = [(int(rng.integers(0, len(types))), int(rng.integers(0, 4))) for _ in range(nk)]
    n_part = int(rng.integers(0, nk + 1))
    outs = wp.all_outputs(types, rng)
    if child != sc:
        outs = [o for o in outs if o[0] != ROWNO]
    p.root = p.new_window_node(child, keys[:n_part], keys[n_part:], outs)
    return p


@pytest.mark.parametrize("block", range(15))
def test_fuzz(block):
    """150 seeded cases, ten per block: schema, key split, flags, functions, NULL rate, run lengths, child kind"""
    rows = 0
    for seed in range(10 * block, 10 * block + 10):
        got, _ = check(fuzz_case(seed), what=seed)
        rows += got.num_rows
    assert rows > 0


# ------------------------------------------------------------------ dirty memory
@pytest.mark.parametrize("part", ["grid", "fuzz-a", "fuzz-b", "fuzz-c"])
@pytest.mark.parametrize("env", POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env, part):
    """nothing may rely on what the memory held: the block cache hands out filled blocks.  The tile-boundary
    sizes of the grid and 30 fuzz cases per fill pattern."""
    if part == "grid":
        for n in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 1):
            for form in PARTS:
                grid_case(n, form, "random", env)
        cols = laid_out_table([TILE + 5], [TILE + 5], rng_for("poison"))
        check(window_plan(cols, [], [], OUTS), env)
    else:
        first = 1_000 + 10 * "abc".index(part[-1])
        for seed in range(first, first + 10):
            check(fuzz_case(seed), env, what=seed)
    s = context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


# ------------------------------------------------------------------ the error contract
def _typed_empty(types):
    return [(dt, np.zeros(0, km.NP_OF[dt])) if dt != VC else (VC, []) for dt in types]


def _error(p, ctx=None):
    with pytest.raises(capi.RjError) as e:
        capi.execute(p, ctx or context())
    return e.value.code, str(e.value)


@pytest.mark.parametrize("rows", [5, 0], ids=["rows", "empty-child"])
def test_error_contract(rows):
    """every refusal, also over an empty child: the node is checked before its child's rows are looked at"""
    rng = rng_for("err")
    types = [I32, I64, F64, VC, I32]
    if rows:
        cols = [km.payload(rng, I32, rows, True), km.payload(rng, I64, rows, False), km.payload(rng, F64, rows, True),
                km.payload(rng, VC, rows, False), (I32, rng.integers(0, 10, rows).astype(np.int32))]
    else:
        cols = _typed_empty(types)
    ok = [(COL, 0, I32), (STAR, 0, I64)]
    bad = lambda part, order, outs=ok: _error(window_plan(cols, part, order, outs))
    # RJ_ERR_ARG
    for part, order, text in (([(5, 0)], [], "key column out of range"), ([], [(-1, 0)], "key column out of range"),
                              ([(0, 0)], [(99, DESC)], "out of range"), ([(0, 4)], [], "flags"), ([], [(0, -1)], "flags"), ([(1, 1 | 2 | 8)], [], "flags")):
        code, msg = bad(part, order, [(STAR, 0, I64)])
        assert code == ARG and text in msg, (part, order, msg)
    for outs, text in (([(SUM, 5, I64)], "output attr out of range"), ([(COL, 7, I32)], "output attr out of range"),
                       ([(9, 1, I64)], "unknown function code"), ([(200, 0, I64)], "unknown function code"),
                       ([(STAR, 1, I64)], "COUNT(*) takes no column"), ([(ROWNO, 1, I64)], "ranking function takes no column"),
                       ([(RANK, 2, I64)], "takes no column"), ([(DENSE, 4, I64)], "takes no column"),
                       ([(COL, 0, I64)], "declared type"), ([(COL, 3, I32)], "declared type"), ([(STAR, 0, I32)], "declared type"),
                       ([(ROWNO, 0, I32)], "declared type"), ([(COUNT, 1, I32)], "declared type"), ([(SUM, 4, I32)], "declared type"),
                       ([(MIN, 1, I32)], "declared type"), ([(MAX, 2, I64)], "declared type"), ([(MIN, 4, I64)], "declared type")):
        code, msg = bad([(0, 0)], [(1, 0)], outs)
        assert code == ARG and text in msg, (outs, msg)
    c = context()
    out = C.c_void_p()
    # n_part > n_keys
    p = window_plan(cols, [(0, 0)], [(1, 0)], ok)
    cplan, keep = pl.plan_to_c(p)
    cplan.nodes[p.root].left_attr = 3
    assert c.L.rj_execute(c.h, C.byref(cplan), C.byref(out)) == ARG and b"partition keys out of" in c.L.rj_last_error(c.h)
    # keys announced, none given
    cplan.nodes[p.root].left_attr = 1
    cplan.nodes[p.root].right_attr = 0
    assert c.L.rj_execute(c.h, C.byref(cplan), C.byref(out)) == ARG and b"NULL key pointer" in c.L.rj_last_error(c.h)
    del keep
    # RJ_ERR_UNSUPPORTED
    for part, order in (([(3, 0)], []), ([(0, 0)], [(3, DESC)])):
        code, msg = bad(part, order, [(STAR, 0, I64)])
        assert code == UNSUPPORTED and "VARCHAR key" in msg, msg
    for func in (COUNT, MIN, MAX, SUM):
        code, msg = bad([(0, 0)], [], [(func, 3, I64 if func in (COUNT, SUM) else VC)])
        assert code == UNSUPPORTED and "VARCHAR" in msg, msg
    code, msg = bad([(0, 0)], [], [(SUM, 2, I64)])
    assert code == UNSUPPORTED and "FP64" in msg and "SUM" in msg
    code, msg = bad([(k % 3, 0) for k in range(4)], [(k % 3, 0) for k in range(5)], [(STAR, 0, I64)])
    assert code == UNSUPPORTED and "8" in msg
    # eight keys are fine, and a VARCHAR column passes through
    got, _ = check(window_plan(cols, [(k % 3, k % 4) for k in range(3)], [(k % 3, k % 4) for k in range(3, 8)],
                               [(COL, 3, VC), (COL, 2, F64), (STAR, 0, I64), (COUNT, 2, I64), (MAX, 2, F64), (DENSE, 0, I64)]))
    assert got.num_rows == rows


def test_empty_child_gives_typed_columns_without_pages():
    got, ran = check(window_plan(_typed_empty([I32, I64, F64, VC]), [(0, 0)], [(2, DESC)],
                                 [(COL, 2, F64), (STAR, 0, I64), (MIN, 1, I64), (COL, 3, VC), (ROWNO, 0, I64), (COL, 0, I32)]))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [F64, I64, I64, VC, I64, I32]
    assert all(c.pages.shape[0] == 0 for c in got.columns) and not launches(ran, "k_win_") and not launches(ran, "k_sort_")


# ------------------------------------------------------------------ every compiled instantiation
def test_every_window_instantiation_is_driven():
    import _elfsyms
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.startswith("k_win_")}
    cols = sp.key_table(rng_for("matrix"), TILE + 1, [I32, I64, F64])
    reached = set()
    for p in (window_plan(cols, [(0, 0)], [(1, DESC)], [(MIN, 0, I32), (MAX, 2, F64), (RANK, 0, I64)]), window_plan(cols, [], [(2, NF)], [(STAR, 0, I64)])):
        reached |= set(launches(check(p)[1], "k_win_"))
    assert reached == compiled, sorted(compiled - reached)
