"""Set operations (RJ_NODE_SETOP) on the device, through the C-ABI, against the numpy reference
tests/_setopref.py (tests/test_setop_plan.py ties it to a row-at-a-time Counter on the CPU).  Every result
column is read by the strict page reader tests/_pagecheck.py first.

Comparison rule: a root sorting operation (every operation but UNION ALL) promises the order of its output
columns and canonical values, so it is compared position by position, doubles by their bits; UNION ALL at
the root over two SCAN children promises left rows then right rows in table order and is compared position
by position too; everything else is compared as a multiset.

Device path: k_setop_concat puts both children's columns one behind the other; the sort's kernels order the
rows, k_group_heads / k_group_scan find and number the runs, k_setop_left / k_setop_scan / k_setop_runs
count every run's rows and left rows, k_setop_mult / k_setop_scan / k_setop_offsets scan the
multiplicities, k_setop_emit lists the run of every output row, k_group_keys and the gather produce the
columns.  The geometry is the grouping's: a tile of GROUP_TILE = 4096 positions (read from
csrc/rj_device.hpp below), a quarter per wave, 64 positions per item; runs are walked in tiles of 4096 and
output rows in tiles of 1024.  RJ_TUNE_SETOP_GRID caps the workgroups, so that one workgroup walks several
tiles.  The one limit no quick test can reach is the row limit (2^32 - 16 rows in both children)."""
import os
import re

import numpy as np
import pytest

import _layouts as lay
import _pagecheck as pc
import _setopref
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
import test_group_plan as gp
import test_setop_plan as tp
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
UNION_ALL, UNION, INTERSECT, INTERSECT_ALL, EXCEPT, EXCEPT_ALL = OPS = tp.OPS
SORTING, OP_NAMES = tp.SORTING, tp.OP_NAMES
_HPP = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
GROUP_TILE = int(re.search(r"constexpr int GROUP_TILE\s*=\s*(\d+);", _HPP).group(1))
assert GROUP_TILE == 4096
ROWS32, ROWS64 = (int(re.search(rf"constexpr uint32_t {n}\s*=\s*(\d+);", _HPP).group(1)) for n in ("ROWS32", "ROWS64"))
T = GROUP_TILE
POISON = [{"RJ_DEBUG_POISON": str(m)} for m in (0x15A, 0x1FF)]
rng_for, setop_plan = sp.rng_for, tp.setop_plan
fam = lambda ran, family: {n: c for n, c in ran.items() if n.split("<")[0] == family}
launches = lambda ran, prefix: {n: c for n, c in ran.items() if n.startswith(prefix)}
ARG, UNSUPPORTED = 1, 5
COUNT_KERNELS = ("k_setop_left", "k_setop_runs", "k_setop_mult", "k_setop_offsets", "k_setop_emit")

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
    return _setopref.decoded_rows([c.type for c in got.columns], dec, got.num_rows)


def _any_order(rows):
    cell = lambda v: (2, 0) if v is None else ((1, v) if isinstance(v, bytes) else (0, v[1] if isinstance(v, tuple) else v))
    return sorted(rows, key=lambda r: tuple(cell(v) for v in r))


def promises_order(p):
    d = p.nodes[p.root].data
    if not isinstance(d, pl.SetOpNode):
        return False
    return d.op != UNION_ALL or all(isinstance(p.nodes[k].data, pl.ScanNode) for k in (d.left, d.right))


def check(p, env=None, what="", exact=None, **kw):
    """Run plan p against the reference under the comparison rule of the module's docstring (exact: overrides it)."""
    got, ran = run(p, env, **kw)
    n, cols = _setopref.evaluate(p)
    assert got.num_rows == n, (what, got.num_rows, n)
    assert [c.type for c in got.columns] == [c[0] for c in cols], what
    rows, want = ordered_rows(got), _setopref.rel_rows(cols, n)
    if promises_order(p) if exact is None else exact:
        assert rows == want, what
    else:
        assert _any_order(rows) == _any_order(want), what
    if n == 0:
        assert all(c.pages.shape[0] == 0 for c in got.columns), what
    return got, ran


# ------------------------------------------------------------------ sizes and run layouts
SIZE_PAIRS = [(0, 0), (0, 1), (1, 0), (0, 65), (65, 0), (1, 1), (1, 62), (63, 1), (32, 33), (64, 64), (T - 2, 1), (T - 1, 1), (1, T), (T, T),
              (T - 1, T + 1), (63, T + 1), (0, 3 * T + 1), (3 * T + 1, 0), (3 * T + 1, 1), (T, 2 * T + 1), (3 * T + 1, 3 * T + 1)]
FORMS = ["each", "one", "random"]
PAIRS2 = [(0, 0, I32), (1, 1, F64)]


def rows_of(keys):
    """the two columns of the grids: an INT32 key and an FP64 column that is a function of it (rows are equal exactly when the keys are)"""
    keys = np.asarray(keys, dtype=np.int64)
    return [(I32, (keys * 3 - 7).astype(np.int32)), (F64, keys.astype(np.float64) * 0.5 - 1.0)]


def form_keys(l, r, form, rng):
    """-> (left keys, right keys): the l + r rows all distinct, all equal, or in runs of random lengths whose copies
    are dealt to the two sides at random (left and right copies interleave inside a run)"""
    n = l + r
    if form == "each":
        keys = np.arange(n)
    elif form == "one":
        keys = np.zeros(n, dtype=np.int64)
    else:
        sizes = []
        while sum(sizes) < n:
            sizes.append(min(int(rng.integers(1, 201)), n - sum(sizes)))
        keys = np.repeat(np.arange(len(sizes)), sizes)
    keys = keys[rng.permutation(n)]
    return keys[:l], keys[l:]


def grid_case(l, r, env=None):
    for form in FORMS:
        rng = rng_for("grid", l, r, form)
        lk, rk = form_keys(l, r, form, rng)
        for op in OPS:
            got, ran = check(setop_plan(op, rows_of(lk), rows_of(rk), PAIRS2), env, what=(l, r, form, OP_NAMES[op]))
            if form == "one" and l + r:
                assert not fam(ran, "k_sort_scatter")          # every digit is constant: no pass, no permutation
                assert got.num_rows == tp.copies(op, l, r)
            if form == "each":
                assert got.num_rows == {UNION_ALL: l + r, UNION: l + r, INTERSECT: 0, INTERSECT_ALL: 0, EXCEPT: l, EXCEPT_ALL: l}[op]


@pytest.mark.parametrize("l,r", SIZE_PAIRS)
def test_size_grid(l, r):
    grid_case(l, r)


@pytest.mark.parametrize("l,r", SIZE_PAIRS)
@pytest.mark.parametrize("grid", [1, 3])
def test_size_grid_with_one_workgroup_walking_several_tiles(grid, l, r):
    grid_case(l, r, {"RJ_TUNE_SETOP_GRID": str(grid)})


LAYOUTS = {
    "ends-at-64-1024-tile": [64, 960, T - 1024, 1, 63, 64 + 1024, 5],
    "ends-one-before-and-after": [63, 2, 959, 1, T - 1025, 2, 100],
    "three-whole-tiles": [T - 3, 3 * T + 10, 7],
    "three-whole-tiles-aligned": [T, 3 * T, T, 1],
    "a-wave-quarter-each": [1024] * 9 + [3],
    "single-rows-around-a-long-run": [1] * 70 + [2 * T] + [1] * 70,
}


def dealt(sizes, rng, shuffle):
    """runs of these sizes in key order, every run's copies dealt to the sides: all left, all right, or a random mix"""
    keys = np.repeat(np.arange(len(sizes)), sizes)
    side = np.concatenate([[np.ones(s, bool), np.zeros(s, bool), rng.random(s) < 0.5, rng.random(s) < 0.9][(i + int(rng.integers(0, 2))) % 4]
                           for i, s in enumerate(sizes)])
    lk, rk = keys[side], keys[~side]
    if shuffle:
        lk, rk = lk[rng.permutation(lk.shape[0])], rk[rng.permutation(rk.shape[0])]
    return lk, rk


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_runs_that_end_on_item_wave_and_tile_borders(layout, shuffle):
    lk, rk = dealt(LAYOUTS[layout], rng_for("layout", layout), shuffle)
    for op in OPS:
        got, ran = check(setop_plan(op, rows_of(lk), rows_of(rk), PAIRS2), what=(layout, OP_NAMES[op]))
        if op == UNION:
            assert got.num_rows == len(LAYOUTS[layout])
        if op not in (UNION_ALL, UNION):
            assert all(fam(ran, k) for k in COUNT_KERNELS[:-1]) and bool(fam(ran, "k_setop_emit")) == (got.num_rows > 0), ran


def test_the_boundary_of_the_concatenation_falls_inside_a_run():
    """both children in key order: the left child's last run goes on as the right child's first"""
    for cut in (1, 63, 64, 65, T - 1, T, T + 1):
        lk = np.r_[np.arange(50), np.full(cut, 50)]
        rk = np.r_[np.full(2 * T - cut, 50), np.arange(51, 90)]
        for op in OPS:
            check(setop_plan(op, rows_of(lk), rows_of(rk), PAIRS2), what=(cut, OP_NAMES[op]))


# ------------------------------------------------------------------ expansion
@pytest.mark.parametrize("op", [INTERSECT_ALL, EXCEPT_ALL], ids=["intersect_all", "except_all"])
def test_one_run_expands_to_three_tiles_and_one_row(op):
    m, rng = 3 * T + 1, rng_for("expand", op)
    if op == INTERSECT_ALL:
        lk, rk = np.r_[np.full(m, 40), np.arange(80)], np.r_[np.full(m + 5, 40), np.arange(0, 80, 2)]
    else:
        lk, rk = np.r_[np.full(m + 7, 40), np.arange(80)], np.r_[np.full(7, 40), np.arange(0, 80, 2)]
    lk, rk = lk[rng.permutation(lk.shape[0])], rk[rng.permutation(rk.shape[0])]
    for env in (None, {"RJ_TUNE_SETOP_GRID": "1"}, {"RJ_TUNE_SETOP_GRID": "3"}):
        got, _ = check(setop_plan(op, rows_of(lk), rows_of(rk), PAIRS2), env)
        assert got.num_rows == m + 40
    # G = 1
    got, _ = check(setop_plan(op, rows_of(np.zeros(2 * m)), rows_of(np.zeros(m - 1 if op == EXCEPT_ALL else m)), PAIRS2))
    assert got.num_rows == (m + 1 if op == EXCEPT_ALL else m)


@pytest.mark.parametrize("env", [None, {"RJ_TUNE_SETOP_GRID": "3"}], ids=["grid", "three-workgroups"])
def test_long_stretches_of_runs_without_copies_between_emitting_runs(env):
    n = 3 * T + 50
    emitting = np.array([0, 1, 700, 701, T - 1, T, T + 1, 2 * T + 300, n - 1])
    allk = np.arange(n)
    rest = np.setdiff1d(allk, emitting)
    rng = rng_for("stretches")
    # EXCEPT [ALL]: the right side cancels everything but the emitting runs (which have 1 or 3 copies on the left)
    lk = np.r_[allk, np.repeat(emitting[::2], 2)][rng.permutation(n + 2 * 5)]
    got, _ = check(setop_plan(EXCEPT, rows_of(lk), rows_of(rest), PAIRS2), env)
    assert got.num_rows == 9
    got, _ = check(setop_plan(EXCEPT_ALL, rows_of(lk), rows_of(rest), PAIRS2), env)
    assert got.num_rows == 9 + 10
    # INTERSECT [ALL]: the right side holds only the emitting runs, some several times
    rk = np.repeat(emitting, [1, 2, 1, 5, 1, 1, 3, 1, 2])
    got, _ = check(setop_plan(INTERSECT, rows_of(lk), rows_of(rk), PAIRS2), env)
    assert got.num_rows == 9
    got, _ = check(setop_plan(INTERSECT_ALL, rows_of(lk), rows_of(rk), PAIRS2), env)
    assert got.num_rows == sum(min(a, b) for a, b in zip([3, 1, 3, 1, 3, 1, 3, 1, 3], [1, 2, 1, 5, 1, 1, 3, 1, 2]))


def test_no_copies_anywhere_gives_no_rows_and_no_pages():
    rng = rng_for("nothing")
    a = rng.integers(0, 500, 2 * T + 3)
    for op, lk, rk in ((EXCEPT, a, a[::-1]), (EXCEPT_ALL, a, np.r_[a, a]), (INTERSECT, a, a + 1000), (INTERSECT_ALL, a, a + 1000)):
        got, ran = check(setop_plan(op, rows_of(lk), rows_of(rk), PAIRS2), what=OP_NAMES[op])
        assert got.num_rows == 0 and [c.type for c in got.columns] == [I32, F64] and all(c.pages.shape[0] == 0 for c in got.columns)
        assert fam(ran, "k_setop_offsets") and not fam(ran, "k_setop_emit") and not fam(ran, "k_group_keys")


@pytest.mark.parametrize("nulls", [False, True], ids=["no-nulls", "nulls"])
@pytest.mark.parametrize("count", [ROWS32 - 1, ROWS32, ROWS32 + 1, ROWS64 - 1, ROWS64, ROWS64 + 1, 3 * ROWS32 + 5])
def test_result_row_counts_around_one_result_pages_capacity(count, nulls):
    rng = rng_for("pages", count, nulls)
    keys = rng.permutation(count + 300)
    mk = lambda k: [(I32, k.astype(np.int32), (k % 7 != 3) if nulls else np.ones(k.shape[0], bool)), (I64, k.astype(np.int64) * 2**33 - 5)]
    outs = [(0, 0, I32), (1, 1, I64)]
    for op, lk, rk in ((EXCEPT, keys, keys[count:]), (EXCEPT_ALL, np.r_[keys, keys[:20]], np.r_[keys[count:], keys[:20]]),
                       (INTERSECT, keys, keys[:count]), (INTERSECT_ALL, keys, np.r_[keys[:count], keys[:9]]), (UNION, keys[:count // 2], keys[count // 3:count]),
                       (UNION_ALL, keys[:count // 2], keys[count // 2:count])):
        got, ran = check(setop_plan(op, mk(lk), mk(rk), outs), what=(count, OP_NAMES[op]))
        assert got.num_rows == count
        assert got.columns[0].pages.shape[0] == -(-count // ROWS32) and got.columns[1].pages.shape[0] == -(-count // ROWS64)
        assert bool(fam(ran, "k_encode_nullable")) == nulls, (OP_NAMES[op], ran)


# ------------------------------------------------------------------ values
def edge_column(dt, times, rng):
    bits = [b for _, b in sp.EDGES[dt]] * times
    null = np.array([v is None for v, _ in sp.EDGES[dt]] * times)
    at = rng.permutation(len(bits))
    raw = np.array(bits, dtype=np.uint64)[at]
    vals = raw.astype(np.uint32).view(np.int32) if dt == I32 else raw.view(km.NP_OF[dt])
    return (dt, vals, ~null[at])


@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_edge_values_of_every_type(dt):
    """the edge list of tests/test_sort_plan.py (NULL, both zeros, NaNs of either sign and several payloads, the
    infinities, the extremes): three copies on the left, one on the right"""
    rng = rng_for("edges", dt)
    lcols, rcols = [edge_column(dt, 3, rng)], [edge_column(dt, 1, rng)]
    distinct = len(sp.EDGES[dt]) - (4 if dt == F64 else 0)      # -0.0 = +0.0, four NaNs are one
    n = len(sp.EDGES[dt])
    for op in OPS:
        got, _ = check(setop_plan(op, lcols, rcols, [(0, 0, dt)]), what=(dt, OP_NAMES[op]))
        assert got.num_rows == {UNION_ALL: 4 * n, UNION: distinct, INTERSECT: distinct, INTERSECT_ALL: n, EXCEPT: 0, EXCEPT_ALL: 2 * n}[op]
        rows = ordered_rows(got)
        if op != UNION_ALL and rows:
            assert rows[-1] == (None,)                           # NULLs last
            if dt == F64:
                assert ("f64", gp.CANON_NAN) in [r[0] for r in rows] and not [r for r in rows if r[0] == ("f64", sp.bits_of(-0.0) - 2**64)]


def test_zeros_of_either_sign_and_nans_of_different_payloads_across_the_sides():
    f = lambda *bits: np.array(bits, dtype=np.uint64).view(np.float64)
    nz = sp.bits_of(-0.0)
    lcols = [(F64, f(nz, sp.SNAN, sp.NEG_NAN, sp.bits_of(1.5)), np.ones(4, bool))]
    rcols = [(F64, f(0, sp.PAYLOAD_NAN, sp.bits_of(2.5)), np.ones(3, bool))]
    rows = lambda op: ordered_rows(check(setop_plan(op, lcols, rcols, [(0, 0, F64)]))[0])
    Z, N = ("f64", 0), ("f64", gp.CANON_NAN)
    assert rows(INTERSECT) == [(Z,), (N,)] and rows(INTERSECT_ALL) == [(Z,), (N,)]
    assert rows(EXCEPT) == [(("f64", sp.bits_of(1.5)),)] and rows(EXCEPT_ALL) == [(("f64", sp.bits_of(1.5)),), (N,)]
    assert rows(UNION) == [(Z,), (("f64", sp.bits_of(1.5)),), (("f64", sp.bits_of(2.5)),), (N,)]
    signed = lambda b: ("f64", b - (2**64 if b >> 63 else 0))
    assert rows(UNION_ALL) == [(signed(b),) for b in (nz, sp.SNAN, sp.NEG_NAN, sp.bits_of(1.5), 0, sp.PAYLOAD_NAN, sp.bits_of(2.5))]


def test_every_null_pattern_over_two_columns_on_both_sides():
    rng = rng_for("nullpat")
    mk = lambda n: [(I32, rng.integers(0, 3, n).astype(np.int32), rng.random(n) >= 0.4), (I64, rng.integers(0, 3, n), rng.random(n) >= 0.4)]
    lcols, rcols = mk(3_000), mk(3_000)
    for op in OPS:
        got, _ = check(setop_plan(op, lcols, rcols, [(1, 1, I64), (0, 0, I32)]), what=OP_NAMES[op])
        if op in (UNION, INTERSECT):
            assert got.num_rows == 16            # (3 values + NULL) squared: (NULL, x), (x, NULL) and (NULL, NULL) are rows of their own
    only_left = [(I32, np.array([1, 1, 1], np.int32), np.array([0, 1, 0], bool)), (I64, np.array([1, 1, 1]), np.array([1, 0, 0], bool))]
    got, _ = check(setop_plan(EXCEPT, only_left, [(I32, np.array([1], np.int32), np.ones(1, bool)), (I64, np.array([1]), np.ones(1, bool))], [(0, 0, I32), (1, 1, I64)]))
    assert ordered_rows(got) == [(1, None), (None, 1), (None, None)]


@pytest.mark.parametrize("side", ["left", "right"])
def test_a_column_that_is_nullable_on_one_side_only(side):
    rng = rng_for("one-sided", side)
    n = T + 77
    nullable = [(I32, rng.integers(0, 50, n).astype(np.int32), rng.random(n) >= 0.2), (I64, rng.integers(0, 3, n), rng.random(n) >= 0.2)]
    plain = [(I32, rng.integers(0, 50, n).astype(np.int32)), (I64, rng.integers(0, 3, n))]          # regular pages, read in place
    lcols, rcols = (nullable, plain) if side == "left" else (plain, nullable)
    for op in OPS:
        got, ran = check(setop_plan(op, lcols, rcols, [(0, 0, I32), (1, 1, I64)]), what=(side, OP_NAMES[op]))
        assert fam(ran, "k_encode_nullable") or got.num_rows == 0  # nullable by declaration, whatever the rows hold


# ------------------------------------------------------------------ column counts and pairings
TYPES8 = [I32, I64, F64, I32, I64, F64, I32, I64]


def narrow_table(rng, n, types=TYPES8):
    return [(dt, rng.integers(0, 2, n).astype(km.NP_OF[dt]), rng.random(n) >= 0.1) for dt in types]


@pytest.mark.parametrize("n_cols", range(1, 9))
def test_one_to_eight_columns_of_mixed_types(n_cols):
    rng = rng_for("cols", n_cols)
    lcols, rcols = narrow_table(rng, 3_000), narrow_table(rng, 2_000)
    outs = [(int(c), int(c), TYPES8[c]) for c in rng.permutation(8)[:n_cols]]
    for op in OPS:
        got, ran = check(setop_plan(op, lcols, rcols, outs), what=(n_cols, OP_NAMES[op]))
        assert sum(fam(ran, "k_setop_concat").values()) == n_cols
        if op == UNION_ALL:
            assert not launches(ran, "k_sort_") and not launches(ran, "k_group_")
        else:
            assert sum(fam(ran, "k_sort_encode").values()) == n_cols and sum(fam(ran, "k_group_heads").values()) == n_cols


def test_nine_distinct_pairs_and_reordered_and_repeated_pairs():
    rng = rng_for("nine")
    types = TYPES8 + [I32]
    lcols, rcols = narrow_table(rng, 500, types), narrow_table(rng, 400, types)
    nine = [(c, c, types[c]) for c in range(9)]
    for op in SORTING:
        code, msg = _error(setop_plan(op, lcols, rcols, nine))
        assert code == UNSUPPORTED and "8" in msg and "distinct" in msg, msg
    got, _ = check(setop_plan(UNION_ALL, lcols, rcols, nine + [(0, 3, I32), (8, 8, I32)]))
    assert got.num_rows == 900 and len(got.columns) == 11
    # pairs across columns, in another order, and twelve outputs over four distinct pairs
    cross = [(3, 0, I32), (1, 4, I64), (5, 2, F64), (0, 6, I32)]
    for op in OPS:
        outs = [cross[i] for i in (2, 0, 3, 1, 2, 2, 0, 1, 3, 3, 0, 1)]
        got, ran = check(setop_plan(op, lcols, rcols, outs), what=OP_NAMES[op])
        assert len(got.columns) == 12 and sum(fam(ran, "k_setop_concat").values()) == 4
        if op != UNION_ALL:
            assert sum(fam(ran, "k_group_heads").values()) == 4
        a = ordered_rows(got)
        assert all(r[0] == r[4] == r[5] and r[1] == r[6] for r in a)


# ------------------------------------------------------------------ UNION ALL keeps the bits
@pytest.mark.parametrize("layout", ["canonical", "one_short_middle", "nullable"])
def test_union_all_keeps_every_values_bits(layout):
    rng = rng_for("bits", layout)
    n = 4 * 1007 + 137
    bits = np.array([b for v, b in sp.EDGES[F64] if v is not None], dtype=np.uint64)
    f64 = bits[rng.integers(0, bits.shape[0], n)].view(np.float64)
    i32 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    valid = rng.random(n) >= 0.3 if layout == "nullable" else None
    name = "canonical" if layout == "nullable" else layout
    cut, canon = lay.tables([lay.Col(F64, f64, valid, name), lay.Col(I32, i32, valid, name)])
    p = pl.Plan()
    a, b = lay.scan_all(p, 0, cut), lay.scan_all(p, 1, cut)
    p.root = p.new_setop_node(UNION_ALL, a, b, [(0, 0, F64), (1, 1, I32)])
    p.new_input(cut)
    p.new_input(cut)
    got, ran = check(p, what=layout)
    assert got.num_rows == 2 * n and not launches(ran, "k_sort_") and not launches(ran, "k_group_")
    v, m = pl.decode_table(got)[0]
    m = np.asarray(m, bool)
    want_m = np.ones(n, bool) if valid is None else valid
    assert np.array_equal(m, np.r_[want_m, want_m])
    assert np.array_equal(np.asarray(v, np.float64).view(np.uint64)[m], np.r_[f64, f64].view(np.uint64)[m])     # -0.0 and every NaN payload
    # canonical pages without NULLs are read in place and written straight into the result's pages; any other layout is
    # decoded into dense values with validity bytes first
    assert bool(fam(ran, "k_encode_nullable")) == (layout != "canonical") and bool(fam(ran, "k_finish_pages")) == (layout == "canonical")


# ------------------------------------------------------------------ VARCHAR
def _vc_table(rng, n):
    return [(I32, rng.integers(0, 100, n).astype(np.int32)), (VC, [b"s%d" % (i * 7 % 311) if i % 11 else None for i in range(n)]), (I64, np.arange(n))]


def test_union_all_of_two_selections_over_one_table_carries_a_varchar_column():
    rng = rng_for("vc")
    cols = _vc_table(rng, 3_000)
    every = [(0, I32), (1, VC), (2, I64)]
    p = pl.Plan()
    a, b = p.new_scan_node(0, every), p.new_scan_node(0, every)
    sa = p.new_select_node(a, [("LT", 0, 30)], every)
    sb = p.new_select_node(b, [("GEQ", 0, 80)], every)
    p.root = p.new_setop_node(UNION_ALL, sa, sb, [(1, 1, VC), (0, 0, I32), (2, 2, I64), (1, 1, VC)])
    p.new_input(pl.make_table(cols))
    got, ran = check(p)
    assert got.num_rows == int(((cols[0][1] < 30) | (cols[0][1] >= 80)).sum()) and fam(ran, "k_setop_concat")
    # ... straight from the scans (row ids that are positions), and with one side empty
    q = pl.Plan()
    a, b = q.new_scan_node(0, every), q.new_scan_node(0, every)
    q.root = q.new_setop_node(UNION_ALL, a, b, [(1, 1, VC), (0, 0, I32)])
    q.new_input(pl.make_table(cols))
    got, _ = check(q)
    assert got.num_rows == 6_000
    r = pl.Plan()
    a, b = r.new_scan_node(0, every), r.new_scan_node(0, every)
    sb = r.new_select_node(b, [("GEQ", 0, 1000)], every)
    r.root = r.new_setop_node(UNION_ALL, a, sb, [(1, 1, VC), (0, 0, I32)])
    r.new_input(pl.make_table(cols))
    got, ran = check(r, exact=True)
    assert got.num_rows == 3_000 and not launches(ran, "k_setop_")


@pytest.mark.parametrize("rows", [200, 0], ids=["rows", "empty-children"])
def test_varchar_pairs_that_are_refused(rows):
    rng = rng_for("vc-refused")
    cols = _vc_table(rng, rows) if rows else _typed_empty([I32, VC, I64])
    cols = cols + [cols[1]]                                        # a second VARCHAR column of the same table
    every = [(0, I32), (1, VC), (2, I64), (3, VC)]
    p = pl.Plan()
    a, b = p.new_scan_node(0, every), p.new_scan_node(1, every)
    p.new_input(pl.make_table(cols))
    p.new_input(pl.make_table(cols))
    for outs in ([(1, 1, VC)], [(0, 0, I32), (1, 1, VC)]):          # two tables
        p.root = p.new_setop_node(UNION_ALL, a, b, outs)
        code, msg = _error(p)
        assert code == UNSUPPORTED and "two base-table columns" in msg, msg
    c = p.new_scan_node(0, every)
    p.root = p.new_setop_node(UNION_ALL, a, c, [(1, 3, VC)])        # one table, two columns
    code, msg = _error(p)
    assert code == UNSUPPORTED and "two base-table columns" in msg, msg
    for op in SORTING:                                             # any VARCHAR pair under a sorting operation
        p.root = p.new_setop_node(op, a, c, [(0, 0, I32), (1, 1, VC)])
        code, msg = _error(p)
        assert code == UNSUPPORTED and "VARCHAR pair" in msg and "sorting" in msg, msg
    p.root = p.new_setop_node(UNION_ALL, a, c, [(3, 3, VC), (1, 1, VC)])
    got, _ = check(p)
    assert got.num_rows == 2 * rows


# ------------------------------------------------------------------ composition
def _pb(rng, n=5_000):
    a = [(I32, rng.integers(0, 600, n).astype(np.int32), rng.random(n) >= 0.05), (I64, rng.integers(-3, 3, n), rng.random(n) >= 0.1)]
    b = [(I32, rng.integers(300, 900, n // 2).astype(np.int32), rng.random(n // 2) >= 0.05), (I64, rng.integers(-3, 3, n // 2))]
    return a, b


def _two_scans(acols, bcols):
    p = pl.Plan()
    sa = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(acols)])
    sb = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(bcols)])
    p.new_input(pl.make_table(acols))
    p.new_input(pl.make_table(bcols))
    return p, sa, sb


BOTH = [(0, I32), (1, I64)]
KINDS_BELOW = ["scan", "join", "semi", "anti", "outer", "full", "agg", "select", "sort", "group", "window", "map", "setop"]


def _below(p, kind, sa, sb):
    """a node of `kind` over scan sa (and sb) that outputs (INT32, INT64)"""
    if kind == "scan":
        return sa
    if kind == "join":
        return p.new_join_node(True, sb, sa, 0, 0, [(2, I32), (1, I64)])
    if kind == "semi":
        return p.new_semi_join_node(True, sb, sa, 0, 0, [(2, I32), (3, I64)])
    if kind == "anti":
        return p.new_anti_join_node(True, sb, sa, 0, 0, [(2, I32), (3, I64)])
    if kind == "outer":
        return p.new_outer_join_node(True, sb, sa, 0, 0, [(0, I32), (3, I64)])
    if kind == "full":
        return p.new_full_outer_join_node(True, sb, sa, 0, 0, [(0, I32), (3, I64)])
    if kind == "agg":
        return p.new_agg_node(sa, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT, 1, I64)])
    if kind == "select":
        return p.new_select_node(sa, [("LT", 1, 1), ("IS_NULL", 0), ("OR",)], BOTH)
    if kind == "sort":
        return p.new_sort_node(sa, [(1, pl.SORT_DESC), (0, 0)], BOTH, limit=3_000)
    if kind == "group":
        return p.new_group_node(sa, [(0, pl.SORT_DESC)], [(pl.AGG_KEY, 0, I32), (pl.AGG_MIN, 1, I64)])
    if kind == "window":
        return p.new_window_node(sa, [(0, 0)], [(1, 0)], [(pl.WIN_COL, 0, I32), (pl.WIN_RANK, 0, I64)])
    if kind == "map":
        return p.new_map_node(sa, [("COL", 1), ("INT", 2), ("MUL",), ("OUT",)], [("COL", 0, I32), ("EXPR", 0, I64)])
    return p.new_setop_node(EXCEPT_ALL, sa, sb, [(0, 0, I32), (1, 1, I64)])


@pytest.mark.parametrize("kind", KINDS_BELOW)
def test_every_kind_below_each_child(kind):
    for op in (UNION_ALL, INTERSECT_ALL, EXCEPT):
        for left in (True, False):
            p, sa, sb = _two_scans(*_pb(rng_for("below", kind)))
            child = _below(p, kind, sa, sb)
            l, r = (child, sb) if left else (sb, child)
            p.root = p.new_setop_node(op, l, r, [(1, 1, I64), (0, 0, I32)])
            got, ran = check(p, what=(kind, OP_NAMES[op], left))
            assert (got.num_rows > 0 or op != UNION_ALL) and fam(ran, "k_setop_concat")


@pytest.mark.parametrize("kind", ["join-build", "join-probe", "semi", "outer", "agg", "select", "sort", "group", "window", "map", "setop"])
def test_every_kind_above_the_node(kind):
    for op in (UNION_ALL, UNION, EXCEPT_ALL):
        p, sa, sb = _two_scans(*_pb(rng_for("above", kind)))
        s = p.new_setop_node(op, sa, sb, [(0, 0, I32), (1, 1, I64)])
        exact = None
        if kind == "join-build":      # the set operation is the build side and its first column the key
            p.root = p.new_join_node(True, s, sb, 0, 0, [(0, I32), (1, I64), (3, I64)])
        elif kind == "join-probe":
            p.root = p.new_join_node(False, s, sb, 0, 0, [(0, I32), (1, I64), (3, I64)])
        elif kind == "semi":
            p.root = p.new_semi_join_node(False, s, sb, 0, 0, BOTH)
        elif kind == "outer":
            p.root = p.new_outer_join_node(False, s, sb, 0, 0, [(0, I32), (1, I64), (3, I64)])
        elif kind == "agg":
            p.root = p.new_agg_node(s, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_SUM, 1, I64)])
        elif kind == "select":
            p.root = p.new_select_node(s, [("GEQ", 0, 450), ("IS_NULL", 1), ("OR",)], BOTH)
        elif kind == "sort":          # every column is a key: the order is fully determined
            p.root = p.new_sort_node(s, [(1, pl.SORT_DESC | pl.SORT_NULLS_FIRST), (0, 0)], BOTH, limit=700, offset=3)
            exact = True
        elif kind == "group":
            p.root = p.new_group_node(s, [(1, 0)], [(pl.AGG_KEY, 1, I64), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_MAX, 0, I32)])
            exact = True
        elif kind == "window":
            p.root = p.new_window_node(s, [(1, 0)], [(0, 0)], [(pl.WIN_COL, 1, I64), (pl.WIN_COL, 0, I32), (pl.WIN_RANK, 0, I64), (pl.WIN_COUNT_STAR, 0, I64)])
        elif kind == "map":           # a MAP at the root keeps the node's order
            p.root = p.new_map_node(s, [("COL", 0), ("COL", 1), ("ADD",), ("OUT",)], [("EXPR", 0, I64), ("COL", 0, I32), ("COL", 1, I64)])
            exact = True
        else:                         # (A op B) EXCEPT C
            p.root = p.new_setop_node(EXCEPT, s, sa, [(0, 0, I32), (1, 1, I64)])
        got, ran = check(p, what=(kind, OP_NAMES[op]), exact=exact)
        assert fam(ran, "k_setop_concat")


def test_a_union_then_except():
    """(A UNION B) EXCEPT C and (A UNION ALL B) EXCEPT ALL C over three tables"""
    rng = rng_for("abc")
    mk = lambda n: [(I32, rng.integers(0, 40, n).astype(np.int32), rng.random(n) >= 0.1), (I64, rng.integers(0, 3, n))]
    for inner, outer in ((UNION, EXCEPT), (UNION_ALL, EXCEPT_ALL), (INTERSECT_ALL, UNION_ALL)):
        p = pl.Plan()
        a, b, c = (p.new_scan_node(i, BOTH) for i in range(3))
        u = p.new_setop_node(inner, a, b, [(0, 0, I32), (1, 1, I64)])
        p.root = p.new_setop_node(outer, u, c, [(1, 1, I64), (0, 0, I32)])
        for n in (T + 5, 900, 300):
            p.new_input(pl.make_table(mk(n)))
        check(p, what=(OP_NAMES[inner], OP_NAMES[outer]))


def test_same_plan_twice_on_one_context():
    lk, rk = form_keys(2 * T, T + 9, "random", rng_for("twice"))
    p = setop_plan(EXCEPT_ALL, rows_of(lk), rows_of(rk), PAIRS2)
    a, _ = run(p)
    b, _ = run(p)
    assert a.num_rows == b.num_rows > 1 and ordered_rows(a) == ordered_rows(b)


# ------------------------------------------------------------------ fuzz
def fuzz_case(seed):
    rng = rng_for("fuzz", seed)
    op = int(rng.integers(0, 6))
    size = lambda: int(rng.integers(0, 3_000)) if rng.random() < 0.75 else int(rng.integers(3_000, 3 * T + 100))
    ln, rn = size(), size()
    if rng.random() < 0.05:
        ln = 0
    types = [[I32, I64, F64][int(rng.integers(0, 3))] for _ in range(int(rng.integers(1, 5)))]
    null_p = [0.0, 0.05, 0.5][int(rng.integers(0, 3))]
    card = int(rng.integers(1, ln + rn + 2)) if rng.random() < 0.5 else int(rng.integers(1, 12))   # duplicate rate

    def table(n):
        if n == 0:
            return tp.empty_cols(types)
        cols = []
        for dt in types:
            v = rng.integers(-(card // 2), card - card // 2, n)
            cols.append((dt, (v * 0.5).astype(np.float64) if dt == F64 else v.astype(km.NP_OF[dt]), rng.random(n) >= null_p))
        edge = sp.key_table(rng, min(n, 16), types, null_p=null_p)                    # ... and the edge values of every type
        return [(dt, np.concatenate([e[1], v[e[1].shape[0]:]]), m) for (dt, v, m), e in zip(cols, edge)]

    outs = tp.random_pairs(rng, types, types, int(rng.integers(1, 5)))
    return setop_plan(op, table(ln), table(rn), outs)


@pytest.mark.parametrize("block", range(15))
def test_fuzz(block):
    """150 seeded cases, ten per block: operation, 1 to 4 columns, types, NULL rate, duplicate rate, sizes up to three tiles"""
    for seed in range(10 * block, 10 * block + 10):
        check(fuzz_case(seed), what=seed)


# ------------------------------------------------------------------ dirty memory
@pytest.mark.parametrize("part", ["sizes-a", "sizes-b", "expand", "fuzz-a", "fuzz-b"])
@pytest.mark.parametrize("env", POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env, part):
    """nothing may rely on zeroed memory: the block cache hands out filled blocks"""
    if part.startswith("sizes"):
        for l, r in SIZE_PAIRS[part == "sizes-b"::2]:
            grid_case(l, r, env)
    elif part == "expand":
        m = 3 * T + 1
        check(setop_plan(INTERSECT_ALL, rows_of(np.r_[np.full(m, 4), np.arange(9)]), rows_of(np.r_[np.arange(0, 9, 2), np.full(m, 4)]), PAIRS2), env)
        a = rng_for("poison").integers(0, 500, 2 * T + 3)
        check(setop_plan(EXCEPT, rows_of(a), rows_of(a), PAIRS2), env)
        lk, rk = dealt(LAYOUTS["single-rows-around-a-long-run"], rng_for("poison", 2), True)
        for op in OPS:
            check(setop_plan(op, rows_of(lk), rows_of(rk), PAIRS2), env)
    else:
        first = 1_000 + 10 * "ab".index(part[-1])
        for seed in range(first, first + 10):
            check(fuzz_case(seed), env, what=seed)
    s = context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


# ------------------------------------------------------------------ the launch log
def test_launch_log_shows_what_each_operation_launches():
    rng = rng_for("log")
    n = 2 * T + 5
    mk = lambda: [(I32, rng.integers(0, 50, n).astype(np.int32)), (I64, rng.integers(0, 9, n), rng.random(n) >= 0.5), (F64, rng.integers(0, 4, n) * 0.5)]
    lcols, rcols = mk(), mk()
    outs = [(0, 0, I32), (1, 1, I64), (2, 2, F64), (0, 0, I32)]
    _, ran = check(setop_plan(UNION_ALL, lcols, rcols, outs))
    assert not launches(ran, "k_sort_") and not launches(ran, "k_group_") and set(launches(ran, "k_setop_")) == {"k_setop_concat<4>", "k_setop_concat<8>"}
    assert ran["k_setop_concat<4>"] == 1 and ran["k_setop_concat<8>"] == 2
    for empty_left in (True, False):                               # one empty side: nothing at all below the root's page encoding
        e = tp.empty_cols([I32, I64, F64])
        _, ran = check(setop_plan(UNION_ALL, e if empty_left else lcols, rcols if empty_left else e, outs))
        assert not launches(ran, "k_setop_") and not launches(ran, "k_sort_") and not launches(ran, "k_group_")
    p = pl.Plan()                                                   # ... and below the root nothing whatsoever
    a, b = p.new_scan_node(0, [(0, I32), (1, I64), (2, F64)]), p.new_scan_node(1, [(0, I32), (1, I64), (2, F64)])
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(tp.empty_cols([I32, I64, F64])))
    u = p.new_setop_node(UNION_ALL, a, b, [(0, 0, I32)])
    p.root = p.new_select_node(u, [], [(0, I32)])
    _, ran = check(p)
    assert not launches(ran, "k_setop_")
    for op in SORTING:
        _, ran = check(setop_plan(op, lcols, rcols, outs), what=OP_NAMES[op])
        assert ran["k_setop_concat<4>"] == 1 and ran["k_setop_concat<8>"] == 2
        assert ran["k_group_heads<4>"] == 1 and ran["k_group_heads<8>"] == 2 and ran["k_group_scan"] == 1       # once per distinct pair
        assert ran["k_group_keys<4>"] == 1 and ran["k_group_keys<8>"] == 2 and not fam(ran, "k_group_reduce")
        assert sum(fam(ran, "k_sort_encode").values()) == 3
        if op == UNION:                                            # every run once: nothing to count
            assert set(launches(ran, "k_setop_")) == {"k_setop_concat<4>", "k_setop_concat<8>"}
        else:
            assert {k: ran.get(k) for k in COUNT_KERNELS} == dict.fromkeys(COUNT_KERNELS, 1) and ran["k_setop_scan"] == 2


def test_every_setop_instantiation_is_driven():
    import _elfsyms
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.startswith("k_setop_")}
    cols = sp.key_table(rng_for("matrix"), T + 1, [I32, I64])
    _, ran = check(setop_plan(INTERSECT_ALL, cols, cols, [(0, 0, I32), (1, 1, I64)]))
    assert set(launches(ran, "k_setop_")) == compiled, sorted(compiled - set(ran))


# ------------------------------------------------------------------ the error contract
def _error(p, ctx=None):
    with pytest.raises(capi.RjError) as e:
        capi.execute(p, ctx or context())
    return e.value.code, str(e.value)


def _typed_empty(types):
    return [(dt, np.zeros(0, km.NP_OF[dt])) if dt != VC else (VC, []) for dt in types]


@pytest.mark.parametrize("rows", [300, 0], ids=["rows", "empty-children"])
def test_error_contract(rows):
    """every refusal, also over empty children: the node is checked before its children's rows are looked at"""
    rng = rng_for("err")
    types = [I32, I64, F64, I32]
    cols = [km.payload(rng, dt, rows, k % 2 == 0) for k, dt in enumerate(types)] if rows else _typed_empty(types)
    ok = [(0, 0, I32), (1, 1, I64)]
    for op in OPS:
        bad = lambda outs, op=op: _error(setop_plan(op, cols, cols, outs))
        for outs, text in (([], "no output columns"), ([(4, 0, I32)], "left column 4 out of range"), ([(0, 4, I32)], "right column 4 out of range"),
                           (ok + [(0, 2**32 - 1, I32)], "out of range"), ([(0, 1, I32)], "differ in type"), ([(2, 1, F64)], "differ in type"),
                           ([(0, 3, I64)], "declared type"), ([(2, 2, I64)], "declared type"), (ok + [(1, 1, I32)], "declared type")):
            code, msg = bad(outs)
            assert code == ARG and text in msg, (OP_NAMES[op], outs, msg)
    for op in (6, 7, 255, 2**40):
        code, msg = _error(setop_plan(op, cols, cols, ok))
        assert code == ARG and "unknown operation code" in msg, msg
    # the same plans are fine without the mistake
    for op in OPS:
        got, _ = check(setop_plan(op, cols, cols, ok + [(0, 3, I32), (2, 2, F64)]), what=OP_NAMES[op])
        assert got.num_rows == (2 * rows if op == UNION_ALL else got.num_rows) and (rows or got.num_rows == 0)


def test_execute_sharded_refuses_and_a_two_device_context_runs_on_one():
    lk, rk = form_keys(3_000, 2_000, "random", rng_for("two"))
    p = setop_plan(INTERSECT_ALL, rows_of(lk), rows_of(rk), PAIRS2)
    got, _ = check(p, devices=[0, 0])
    assert got.num_rows > 1
    ctx = context(devices=[0, 0])
    tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
    try:
        with pytest.raises(capi.RjError) as e:
            ctx.execute_sharded(p, tables)
        assert e.value.code == UNSUPPORTED and "RJ_NODE_SETOP" in str(e.value)
    finally:
        for row in tables:
            for t in row:
                t.release()


def test_empty_children_give_typed_columns_without_pages():
    e = _typed_empty([I32, I64, F64, VC])
    for op in OPS:
        outs = [(2, 2, F64), (0, 0, I32), (1, 1, I64)] + ([(3, 3, VC)] if op == UNION_ALL else [])
        p = pl.Plan()
        a, b = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(e)]), p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(e)])
        p.root = p.new_setop_node(op, a, b, outs)
        p.new_input(pl.make_table(e))
        got, ran = check(p, what=OP_NAMES[op])
        assert got.num_rows == 0 and [c.type for c in got.columns] == [t for _, _, t in outs]
        assert all(c.pages.shape[0] == 0 for c in got.columns) and not launches(ran, "k_setop_") and not launches(ran, "k_sort_")
