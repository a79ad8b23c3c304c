"""RJ_AGG_FSUM, the exactly rounded FP64 sum of RJ_NODE_GROUP, on the device, through the C-ABI, against
the reference tests/_fsumref.py (integers in units of 2^-1074, rounded by Python; tests/test_fsum_plan.py
ties it to math.fsum and to the host twin of the kernels' arithmetic).  Every result column is read by
the strict page reader tests/_pagecheck.py first, and every sum is compared bit for bit.

Device path: what RJ_NODE_GROUP runs without FSUM (tests/test_gpu_group.py), and for every column under
FSUM k_fsum_slots / k_fsum_zero / k_fsum_reduce / k_fsum_finish (csrc/rj_fsum.hip).  The geometry is the
grouping's: a tile of 4096 positions, a quarter per wave, 64 positions per item; RJ_TUNE_GROUP_GRID caps
the workgroups, so that one workgroup walks several tiles and neighbours share groups in the arena."""
import math

import numpy as np
import pytest

import _fsumref
import _layouts as lay
import _pagecheck as pc
import test_fsum_plan as fp
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
import test_group_plan as gp
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
KEY, STAR, COUNT, SUM, MIN, MAX, FSUM = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX, pl.AGG_FSUM
GROUP_TILE = 4096
POISON = [{"RJ_DEBUG_POISON": str(m)} for m in (0x15A, 0x1FF)]
GRIDS = [None, {"RJ_TUNE_GROUP_GRID": "1"}, {"RJ_TUNE_GROUP_GRID": "3"}]
GRID_IDS = ["grid-default", "grid-1", "grid-3"]
rng_for, group_plan, bits_of = sp.rng_for, gp.group_plan, sp.bits_of
fam = lambda ran, family: {n: c for n, c in ran.items() if n.split("<")[0] == family}
launches = lambda ran, prefix: {n: c for n, c in ran.items() if n.startswith(prefix)}
ARG, UNSUPPORTED = 1, 5
O = ("OUT",)
f64 = lambda bits: np.asarray(bits, dtype=np.uint64).view(np.float64)
cell = lambda bits: None if bits is None else ("f64", bits - 2**64 if bits >> 63 else bits)     # a double in a result row (_sortref.rel_rows)

_contexts = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _contexts.values():
        c.destroy()
    _contexts.clear()


def context(env=None):
    key = tuple(sorted((env or {}).items()))
    if key not in _contexts:
        _contexts[key] = fm.tuned_context(env or {})
    return _contexts[key]


def run(p, env=None):
    c = context(env)
    c.launch_log(True)
    try:
        got = capi.execute(p, c)
        ran = km.launched(c)
    finally:
        c.launch_log(False)
    return got, ran


def ordered_rows(got):
    """the result's rows IN ORDER (doubles as ("f64", bits)), every column through the strict page reader first"""
    dec = pc.check_table(got)
    assert pc.same_as(dec, pl.decode_table(got))
    return _fsumref.decoded_rows([c.type for c in got.columns], dec, got.num_rows)


def _any_order(rows):
    cell = lambda v: (1, 0) if v is None else (0, v[1] if isinstance(v, tuple) else v)
    return sorted(rows, key=lambda r: tuple(cell(v) for v in r))


_reference = {}


def reference(p, tag=None):
    """(rows, columns) of the plan, computed once per tag and left unchanged"""
    if tag is None:
        return _fsumref.evaluate(p)
    if tag not in _reference:
        _reference[tag] = _fsumref.evaluate(p)
    return _reference[tag]


def check(p, env=None, what="", tag=None):
    """a root grouping position by position, doubles by their bits; any other root as a multiset"""
    got, ran = run(p, env)
    n, cols = reference(p, tag)
    assert got.num_rows == n, (what, got.num_rows, n)
    assert [c.type for c in got.columns] == [c[0] for c in cols], what
    rows, want = ordered_rows(got), _fsumref.rel_rows(cols, n)
    if isinstance(p.nodes[p.root].data, pl.GroupNode):
        assert rows == want, (what, [(i, a, b) for i, (a, b) in enumerate(zip(rows, want)) if a != b][:3])
    else:
        assert _any_order(rows) == _any_order(want), what
    return got, ran


# ------------------------------------------------------------------ row counts and run layouts
SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, GROUP_TILE - 1, GROUP_TILE, GROUP_TILE + 1, 3 * GROUP_TILE + 1]
FORMS = ["one", "each", "random"]
OUTS = [(KEY, 0, I32), (FSUM, 1, F64), (COUNT, 1, I64), (STAR, 0, I64)]


def values(rng, n, specials=True):
    """mixed magnitudes and signs, pairs that cancel, a few non-finite values"""
    v = fp.random_multiset(rng, n).view(np.float64).copy()
    if specials and n > 64:
        at = rng.integers(0, n, max(3, n // 500))
        v[at] = rng.choice(np.array([np.inf, -np.inf, np.nan, -0.0]), at.shape[0])
    return v


def sized_table(sizes, rng, nulls, shuffle=True, specials=True):
    """an INT32 key whose groups have these sizes in the order of the key, and an FP64 value"""
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    key = np.repeat(np.arange(sizes.shape[0]) * 3 - 7, sizes).astype(np.int32)
    if shuffle:
        key = key[rng.permutation(n)]
    v = values(rng, n, specials)
    return [(I32, key), (F64, v, rng.random(n) >= 0.3) if nulls else (F64, v)]


def form_sizes(n, form, rng):
    if form == "one":
        return [n]
    if form == "each":
        return np.ones(n, dtype=np.int64)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 201)), n - sum(sizes)))
    return sizes


def grid_case(n, form, nulls, env=None):
    rng = rng_for("fsum-grid", n, form, nulls)
    cols = sized_table(form_sizes(n, form, rng), rng, nulls)
    got, ran = check(group_plan(cols, [(0, 0)], OUTS), env, what=(n, form, nulls, env), tag=("grid", n, form, nulls))
    assert got.num_rows == {"one": 1, "each": n}.get(form, got.num_rows)
    assert ran.get("k_fsum_reduce<true>") == 1 and ran.get("k_fsum_finish") == 1 and len(fam(ran, "k_fsum_reduce")) == 1
    return got


@pytest.mark.parametrize("env", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("nulls", [False, True], ids=["no-nulls", "nulls"])
@pytest.mark.parametrize("form", FORMS)
def test_size_grid(form, nulls, env):
    for n in SIZES:
        grid_case(n, form, nulls, env)


LAYOUTS = {
    "ends-at-64-1024-tile": [64, 960, GROUP_TILE - 1024, 1, 63, 64 + 1024, 5],
    "ends-one-before-and-after": [63, 2, 959, 1, GROUP_TILE - 1025, 2, 100],
    "one-group-over-three-tiles": [GROUP_TILE - 3, 3 * GROUP_TILE + 10, 7],
    "three-whole-tiles-aligned": [GROUP_TILE, 3 * GROUP_TILE, GROUP_TILE, 1],
    "a-wave-quarter-each": [1024] * 9 + [3],
    "single-rows-around-a-long-run": [1] * 70 + [2 * GROUP_TILE] + [1] * 70,
    "every-item-border": [64] * 20 + [63, 65, 1, 127, 129],
}


@pytest.mark.parametrize("env", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_runs_that_end_on_item_wave_and_tile_borders(layout, env):
    for shuffle in (False, True):
        cols = sized_table(LAYOUTS[layout], rng_for("fsum-layout", layout, shuffle), True, shuffle)
        got, _ = check(group_plan(cols, [(0, 0)], OUTS), env, what=(layout, shuffle), tag=("layout", layout, shuffle))
        assert np.array_equal(pl.decode_table(got)[3][0], LAYOUTS[layout])          # COUNT(*): the run lengths, in key order


# ------------------------------------------------------------------ values
def edge_columns():
    """the CPU edge grid as one table: one group per entry, in the grid's (sorted) order"""
    key, bits, valid = [], [], []
    for g, name in enumerate(sorted(fp.EDGE)):
        b, ok = fp.EDGE[name]
        key += [g] * len(b)
        bits += b
        valid += [True] * len(b) if ok is None else ok
    return np.array(key, dtype=np.int32), np.array(bits, dtype=np.uint64), np.array(valid, dtype=bool)


@pytest.mark.parametrize("env", GRIDS + POISON[:1], ids=GRID_IDS + ["poison"])
def test_edge_grid_mixed_into_one_table(env):
    key, bits, valid = edge_columns()
    at = rng_for("fsum-edge-mixed").permutation(key.shape[0])
    cols = [(I32, key[at]), (F64, f64(bits[at]), valid[at])]
    got, _ = check(group_plan(cols, [(0, 0)], OUTS), env, tag="edge-mixed")
    rows = ordered_rows(got)
    names = [n for n in sorted(fp.EDGE) if fp.EDGE[n][0]]
    assert len(rows) == len(names)
    for name, r in zip(names, rows):            # ... and directly against the per-entry reference
        want = _fsumref.fsum_bits(*fp.EDGE[name])
        assert r[1] == cell(want), name


@pytest.mark.parametrize("name", sorted(n for n in fp.EDGE if fp.EDGE[n][0]))
def test_edge_grid_one_group_each(name):
    """every entry as a column of its own: as one keyed group and as the scalar aggregate"""
    b, ok = fp.EDGE[name]
    want = cell(_fsumref.fsum_bits(b, ok))
    col = (F64, f64(b)) if ok is None else (F64, f64(b), np.array(ok))
    got, _ = check(group_plan([(I32, np.zeros(len(b), np.int32)), col], [(0, 0)], [(FSUM, 1, F64)]), what=name)
    assert ordered_rows(got) == [(want,)]
    got, ran = check(group_plan([(I32, np.zeros(len(b), np.int32)), col], [], [(FSUM, 1, F64), (COUNT, 1, I64)]), what=name)
    assert ordered_rows(got)[0][0] == want and ran.get("k_fsum_reduce<false>") == 1


def test_infinities_and_nans_stay_in_their_group():
    rng = rng_for("fsum-neighbours")
    sizes = [100, 1, 2, 700, 64, 3000, 5, 1, 1, 2]
    cols = sized_table(sizes, rng, False, shuffle=False, specials=False)
    k, v = cols[0][1], cols[1][1]
    v[k == -7 + 3 * 3] = 1.0
    v[np.flatnonzero(k == -7 + 3 * 3)[[5, 300]]] = [np.inf, -np.inf]          # group 3: NaN
    v[np.flatnonzero(k == -7 + 3 * 5)[1500]] = -np.inf                        # group 5: -inf
    v[k == -7 + 3 * 4] = -0.0                                                 # group 4: -0.0 only -> +0.0
    v[np.flatnonzero(k == -7 + 3 * 7)] = np.nan                               # a group of one NaN
    at = rng.permutation(k.shape[0])
    got, _ = check(group_plan([(I32, k[at]), (F64, v[at])], [(0, 0)], OUTS))
    rows = ordered_rows(got)
    assert rows[3][1] == cell(fp.NAN) and rows[5][1] == cell(fp.NINF) and rows[4][1] == cell(0) and rows[7][1] == cell(fp.NAN)
    finite = [r[1][1] % 2**64 for i, r in enumerate(rows) if i not in (3, 5, 7)]
    assert all((b >> 52) & 0x7FF != 0x7FF for b in finite)


def test_a_column_of_negative_zeros_and_the_null_group_of_a_nullable_key():
    rng = rng_for("fsum-null-key")
    n = 3 * GROUP_TILE
    k = rng.integers(0, 6, n).astype(np.int32)
    kvalid = rng.random(n) >= 0.2
    v = values(rng, n)
    got, _ = check(group_plan([(I32, k, kvalid), (F64, v, rng.random(n) >= 0.1), (F64, np.full(n, -0.0))], [(0, NF)],
                              [(KEY, 0, I32), (FSUM, 1, F64), (FSUM, 2, F64), (STAR, 0, I64)]))
    rows = ordered_rows(got)
    assert rows[0][0] is None and len(rows) == 7 and all(r[2] == ("f64", 0) for r in rows)


def test_groups_without_a_value_are_null_whatever_their_neighbours_hold():
    rng = rng_for("fsum-null-groups")
    sizes = [1, 64, 1, 1024, 2, 4096 + 5, 1, 3]
    cols = sized_table(sizes, rng, True, shuffle=True)
    k, (_, v, ok) = cols[0][1], cols[1]
    for g in range(8):      # four groups without a value, and at least one value in every other group
        ok[k == -7 + 3 * g] &= g not in (0, 3, 5, 6)
        if g not in (0, 3, 5, 6):
            ok[np.flatnonzero(k == -7 + 3 * g)[0]] = True
    got, _ = check(group_plan(cols, [(0, DESC)], OUTS))
    rows = ordered_rows(got)[::-1]
    assert [r[1] is None for r in rows] == [g in (0, 3, 5, 6) for g in range(8)]


def test_a_group_that_spans_every_bit_of_the_accumulator():
    """values from 2^-1074 to the largest double in one group of more than a tile, next to short groups"""
    rng = rng_for("fsum-span")
    n = GROUP_TILE + 500
    e = rng.integers(0, 2047, n).astype(np.uint64)
    bits = (e << np.uint64(52)) | rng.integers(0, 2**52, n, dtype=np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))
    bits[:4] = [1, fp.DBL_MAX, 1 | fp.NEG, fp.DBL_MAX | fp.NEG]
    key = np.r_[np.full(n, 5), [1, 1, 9]].astype(np.int32)
    v = np.r_[f64(bits), [0.1, 0.2, -5e-324]]
    for env in GRIDS:
        check(group_plan([(I32, key), (F64, v)], [(0, 0)], OUTS), env, tag="span")
    # large cancellation, then a tiny rest: every huge value has its negative, 3 * 2^-1074 is left
    big = f64(bits[: n // 2 * 2 // 2])
    big = big[np.isfinite(big)]
    v = np.r_[big, -big, [5e-324] * 3]
    v = v[rng.permutation(v.shape[0])]
    got, _ = check(group_plan([(I32, np.zeros(v.shape[0], np.int32)), (F64, v)], [(0, 0)], [(FSUM, 1, F64)]))
    assert ordered_rows(got) == [(("f64", 3),)]


# ------------------------------------------------------------------ the scalar aggregate
def test_scalar_aggregate_over_no_rows_one_row_and_many_workgroups():
    outs = [(FSUM, 1, F64), (COUNT, 1, I64), (STAR, 0, I64), (FSUM, 2, F64)]
    empty = [(I32, np.zeros(0, np.int32)), (F64, np.zeros(0)), (F64, np.zeros(0))]
    for env in (None, POISON[0]):
        got, ran = check(group_plan(empty, [], outs), env)
        assert ordered_rows(got) == [(None, 0, 0, None)] and not fam(ran, "k_fsum_reduce")
    got, _ = check(group_plan([(I32, np.array([1], np.int32)), (F64, np.array([-0.0])), (F64, np.array([-2.5]))], [], outs))
    assert ordered_rows(got) == [(cell(0), 1, 1, cell(bits_of(-2.5)))]
    n = 300_000
    rng = rng_for("fsum-scalar")
    cols = [(I32, np.zeros(n, np.int32)), (F64, values(rng, n, specials=False), rng.random(n) >= 0.01), (F64, rng.random(n) * 1e-3 - 2e-4)]
    for env in GRIDS + POISON[1:]:
        got, ran = check(group_plan(cols, [], outs), env, tag="scalar-300k")
        assert got.num_rows == 1 and not launches(ran, "k_sort_") and not fam(ran, "k_group_heads")
        assert ran.get("k_fsum_reduce<false>") == 2 and len(fam(ran, "k_fsum_reduce")) == 1
    want = _fsumref.fsum_bits(cols[2][1].view(np.uint64))
    assert ordered_rows(got)[0][3] == cell(want) and want == bits_of(math.fsum(cols[2][1].tolist()))


# ------------------------------------------------------------------ order independence
def test_row_orders_paginations_and_grid_caps_give_identical_bits():
    rng = rng_for("fsum-orders")
    n = 2 * GROUP_TILE + 77
    key = rng.integers(0, 40, n).astype(np.int32)
    v, ok = values(rng, n), rng.random(n) >= 0.25
    outs = [(KEY, 0, I32), (FSUM, 1, F64), (COUNT, 1, I64)]
    want = None
    for o, at in enumerate((np.arange(n), np.arange(n)[::-1], rng.permutation(n))):
        for layout in ("canonical", "one_short_middle", "random_cuts"):
            cols = [lay.Col(I32, key[at], None, layout, seed=o), lay.Col(F64, v[at], ok[at], layout, seed=o + 1)]
            cut, canon = lay.tables(cols)
            p = group_plan([(I32, key[at]), (F64, v[at], ok[at])], [(0, 0)], outs)
            for env in GRIDS:
                got, _ = run(lay.with_inputs(p, [cut]), env)
                rows = ordered_rows(got)
                if want is None:
                    n_ref, ref = _fsumref.evaluate(p)
                    want = _fsumref.rel_rows(ref, n_ref)
                assert rows == want, (o, layout, env)


# ------------------------------------------------------------------ together with the rest
def _kcols(rng, n=6_000):
    price = np.round(rng.random(n) * 1000, 2)
    return [(I32, rng.integers(0, 50, n).astype(np.int32), rng.random(n) >= 0.05), (F64, price, rng.random(n) >= 0.1),
            (I64, rng.integers(1, 20, n)), (F64, values(rng, n))]


def _scan_plan(cols):
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    p.new_input(pl.make_table(cols))
    return p, sc


def test_next_to_every_other_function_and_two_fsum_columns():
    cols = _kcols(rng_for("fsum-mix"))
    outs = [(FSUM, 3, F64), (KEY, 0, I32), (MIN, 1, F64), (FSUM, 1, F64), (COUNT, 1, I64), (STAR, 0, I64), (MAX, 3, F64), (SUM, 2, I64),
            (FSUM, 1, F64), (COUNT, 3, I64), (MAX, 1, F64), (FSUM, 3, F64)]
    got, ran = check(group_plan(cols, [(0, DESC | NF)], outs))
    assert got.num_rows == 51 and ran.get("k_fsum_reduce<true>") == 2             # one launch per column under FSUM
    check(group_plan(cols, [(0, 0), (2, DESC)], outs))
    check(group_plan(cols, [(1, 0)], [(KEY, 1, F64), (FSUM, 1, F64), (FSUM, 3, F64)]))      # the summed column is the key
    check(group_plan(cols, [], outs[2:]))


def test_sum_of_price_times_qty_and_the_avg_recipe():
    """a MAP below computes price * qty in doubles, the grouping sums the products exactly, and a MAP above
    divides by the count: AVG is FSUM(x) / TO_F64(COUNT(x)), NULL where the group has no value"""
    cols = _kcols(rng_for("fsum-avg"))
    cols[1][2][cols[0][1] == 7] = False                                          # the group of key 7 has no price
    p, sc = _scan_plan(cols)
    m = p.new_map_node(sc, [("COL", 1), ("COL", 2), ("TO_F64",), ("MUL",), O], [("COL", 0, I32), ("EXPR", 0, F64), ("COL", 1, F64)])
    g = p.new_group_node(m, [(0, 0)], [(KEY, 0, I32), (FSUM, 1, F64), (COUNT, 1, I64), (FSUM, 2, F64), (COUNT, 2, I64)])
    p.root = g
    check(p)
    p.root = p.new_map_node(g, [("COL", 3), ("COL", 4), ("TO_F64",), ("DIV",), O], [("COL", 0, I32), ("COL", 1, F64), ("EXPR", 0, F64)])
    got, ran = check(p)
    rows = {r[0]: r for r in ordered_rows(got)}
    assert rows[7][1] is None and rows[7][2] is None and fam(ran, "k_fsum_reduce") and sum(fam(ran, "k_map").values()) == 2
    k, price, ok = cols[0][1], cols[1][1], cols[1][2] & cols[0][2]
    sel = ok & (k == 3)
    avg = np.float64(math.fsum(price[sel].tolist())) / np.float64(int(sel.sum()))
    assert rows[3][2] == cell(bits_of(float(avg)))


@pytest.mark.parametrize("kind", ["join", "select", "sort", "window", "setop"])
def test_fsum_over_every_kind(kind):
    rng = rng_for("fsum-over", kind)
    cols = _kcols(rng)
    p, sc = _scan_plan(cols)
    every = [(i, c[0]) for i, c in enumerate(cols)]
    if kind == "join":
        other = p.new_scan_node(1, [(0, I32)])
        p.new_input(pl.make_table([(I32, rng.integers(0, 60, 300).astype(np.int32))]))
        child = p.new_join_node(False, sc, other, 0, 0, every)
    elif kind == "select":
        child = p.new_select_node(sc, [("GEQ", 2, 5), ("IS_NULL", 0), ("OR",)], every)
    elif kind == "sort":
        child = p.new_sort_node(sc, [(2, DESC), (0, 0)], every, limit=4_500, offset=3)
    elif kind == "window":
        child = p.new_window_node(sc, [(0, 0)], [(2, 0)], [(pl.WIN_COL, 0, I32), (pl.WIN_COL, 1, F64), (pl.WIN_ROW_NUMBER, 0, I64), (pl.WIN_COL, 3, F64)])
    else:
        child = p.new_setop_node(pl.SET_UNION_ALL, sc, sc, [(i, i, c[0]) for i, c in enumerate(cols)])
    p.root = p.new_group_node(child, [(0, NF)], [(KEY, 0, I32), (FSUM, 1, F64), (FSUM, 3, F64), (STAR, 0, I64)])
    got, ran = check(p, what=kind)
    assert got.num_rows > 1 and ran.get("k_fsum_reduce<true>") == 2


@pytest.mark.parametrize("kind", ["join", "select", "sort", "window", "setop", "group"])
def test_every_kind_over_fsum(kind):
    rng = rng_for("fsum-under", kind)
    cols = _kcols(rng)
    p, sc = _scan_plan(cols)
    g = p.new_group_node(sc, [(0, 0)], [(KEY, 0, I32), (FSUM, 1, F64), (COUNT, 1, I64), (FSUM, 3, F64)])
    out3 = [(0, I32), (1, F64), (2, I64)]
    if kind == "join":
        other = p.new_scan_node(1, [(0, I32)])
        p.new_input(pl.make_table([(I32, rng.integers(0, 60, 300).astype(np.int32))]))
        p.root = p.new_join_node(True, g, other, 0, 0, out3)
    elif kind == "select":          # HAVING COUNT(price) >= 100
        p.root = p.new_select_node(g, [("GEQ", 2, 100)], out3)
    elif kind == "sort":            # ORDER BY the sum
        p.root = p.new_sort_node(g, [(1, DESC), (0, 0)], out3, limit=20)
    elif kind == "window":          # the rank of a group by its sum
        p.root = p.new_window_node(g, [], [(1, DESC)], [(pl.WIN_COL, 0, I32), (pl.WIN_COL, 1, F64), (pl.WIN_RANK, 0, I64)])
    elif kind == "setop":
        p.root = p.new_setop_node(pl.SET_UNION, g, g, [(0, 0, I32), (1, 1, F64), (3, 3, F64)])
    else:                           # the sums of the sums, by count parity ... by count
        p.root = p.new_group_node(g, [(2, 0)], [(KEY, 2, I64), (FSUM, 1, F64), (FSUM, 3, F64)])
    got, ran = check(p, what=kind)
    assert got.num_rows > 0 and fam(ran, "k_fsum_reduce")


def test_order_at_the_root_with_an_fsum_column():
    cols = _kcols(rng_for("fsum-root-order"))
    for flags in sp.ALL_FLAGS:
        got, _ = check(group_plan(cols, [(0, flags), (2, DESC)], [(FSUM, 1, F64), (KEY, 2, I64), (KEY, 0, I32)]), what=flags)
        keys = [(r[2], r[1]) for r in ordered_rows(got)]
        nulls = [k[0] is None for k in keys]
        assert nulls == sorted(nulls, reverse=bool(flags & NF)) and len(set(keys)) == len(keys)


# ------------------------------------------------------------------ fuzz
def fuzz_case(seed):
    rng = rng_for("fsum-fuzz", seed)
    n = int(rng.integers(1, 3_000)) if rng.random() < 0.75 else int(rng.integers(3_000, 40_001))
    types = [[I32, I64, F64][int(rng.integers(0, 3))] for _ in range(3)] + [F64, F64]
    null_p = [0.0, 0.05, 0.5][int(rng.integers(0, 3))]
    card = int(rng.integers(1, n + 1)) if rng.random() < 0.5 else int(rng.integers(1, 40))
    cols = []
    for dt in types[:3]:
        v = rng.integers(-(card // 2), card - card // 2, n)
        cols.append((dt, (v * 0.5).astype(np.float64) if dt == F64 else v.astype(km.NP_OF[dt]), rng.random(n) >= null_p))
    cols.append((F64, values(rng, n), rng.random(n) >= null_p))
    cols.append((F64, np.round(rng.standard_normal(n) * 100, 3), rng.random(n) >= null_p))
    p, sc = _scan_plan(cols)
    every = [(i, dt) for i, dt in enumerate(types)]
    child, kind = sc, ["scan", "select", "sort", "map"][int(rng.integers(0, 4))]
    if kind == "select":
        child = p.new_select_node(sc, [("IS_NOT_NULL", 0), ("IS_NULL", 1), ("OR",)], every)
    elif kind == "sort":
        child = p.new_sort_node(sc, [(1, DESC)], every)
    elif kind == "map":
        child = p.new_map_node(sc, [("COL", 3), ("COL", 4), ("MUL",), O], [("COL", i, dt) for i, dt in enumerate(types[:4])] + [("EXPR", 0, F64)])
    nk = int(rng.integers(0, 4))
    keys = [(int(rng.integers(0, len(types))), int(rng.integers(0, 4))) for _ in range(nk)]
    outs = gp.all_outputs(types, keys, rng) + [(FSUM, 3 + int(rng.integers(0, 2)), F64)]
    outs += [(FSUM, c, F64) for c in range(5) if types[c] == F64 and rng.random() < 0.4]
    outs = [outs[i] for i in rng.permutation(len(outs))]
    p.root = p.new_group_node(child, keys, outs)
    return p


@pytest.mark.parametrize("block", range(15))
def test_fuzz(block):
    """150 seeded grouping plans that hold FSUM, ten per block"""
    rows = 0
    for seed in range(10 * block, 10 * block + 10):
        got, ran = check(fuzz_case(seed), GRIDS[seed % 3], what=seed)
        assert fam(ran, "k_fsum_reduce") or got.num_rows == 0 or not fam(ran, "k_group_reduce")
        rows += got.num_rows
    assert rows > 0


# ------------------------------------------------------------------ dirty memory
@pytest.mark.parametrize("part", ["one", "each", "random", "layouts", "fuzz"])
@pytest.mark.parametrize("env", POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env, part):
    """nothing may rely on zeroed memory: the block cache hands out filled blocks"""
    if part in FORMS:
        for n in SIZES:
            grid_case(n, part, True, {**env, "RJ_TUNE_GROUP_GRID": "3"} if n > GROUP_TILE else env)
    elif part == "layouts":
        for layout in sorted(LAYOUTS):
            cols = sized_table(LAYOUTS[layout], rng_for("fsum-layout", layout, True), True, True)
            check(group_plan(cols, [(0, 0)], OUTS), {**env, "RJ_TUNE_GROUP_GRID": "3"}, what=layout, tag=("layout", layout, True))
    else:
        for seed in range(1_000, 1_015):
            check(fuzz_case(seed), env, what=seed)
    s = context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


# ------------------------------------------------------------------ the launch log
def test_fsum_launches_appear_exactly_when_an_output_names_fsum():
    n = 2 * GROUP_TILE + 5
    rng = rng_for("fsum-log")
    cols = [(I32, rng.integers(0, 50, n).astype(np.int32)), (F64, values(rng, n), rng.random(n) >= 0.5), (F64, rng.random(n))]
    without = [(KEY, 0, I32), (STAR, 0, I64), (COUNT, 1, I64), (MIN, 1, F64), (MAX, 2, F64)]
    _, ran0 = check(group_plan(cols, [(0, 0)], without))
    assert not launches(ran0, "k_fsum_")
    _, ran1 = check(group_plan(cols, [(0, 0)], without + [(FSUM, 1, F64)]))
    assert launches(ran1, "k_fsum_") == {"k_fsum_slots": 1, "k_fsum_zero": 1, "k_fsum_reduce<true>": 1, "k_fsum_finish": 1}
    rest = lambda ran: {k: v for k, v in ran.items() if not k.startswith("k_fsum_") and k.split("<")[0] not in ("k_group_column", "k_encode_nullable")}
    assert rest(ran1) == rest(ran0)                     # a column that is already reduced: only the FSUM kernels and its result column are new
    _, ran2 = check(group_plan(cols, [(0, 0)], [(FSUM, 2, F64), (FSUM, 2, F64)]))
    assert ran2.get("k_fsum_reduce<true>") == 1 and ran2.get("k_group_reduce<8,true>") == 1     # the count that decides NULL
    _, ran3 = check(group_plan(cols, [], [(FSUM, 1, F64)]))
    assert launches(ran3, "k_fsum_") == {"k_fsum_slots": 1, "k_fsum_zero": 1, "k_fsum_reduce<false>": 1, "k_fsum_finish": 1}
    import _elfsyms
    compiled = {x for x in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if x.startswith("k_fsum_")}
    assert compiled == set(launches(ran1, "k_fsum_")) | set(launches(ran3, "k_fsum_"))


# ------------------------------------------------------------------ the error contract
def _error(p):
    with pytest.raises(capi.RjError) as e:
        capi.execute(p, context())
    return e.value.code, str(e.value)


@pytest.mark.parametrize("rows", [300, 0], ids=["rows", "empty-child"])
def test_error_contract(rows):
    rng = rng_for("fsum-err")
    types = [I32, I64, F64, VC]
    if rows:
        cols = [km.payload(rng, I32, rows, True), km.payload(rng, I64, rows, False), km.payload(rng, F64, rows, True), km.payload(rng, VC, rows, False)]
    else:
        cols = [(dt, np.zeros(0, km.NP_OF[dt])) if dt != VC else (VC, []) for dt in types]
    bad = lambda keys, outs: _error(group_plan(cols, keys, outs))
    for keys in ([(0, 0)], []):
        for c in (0, 1):
            code, msg = bad(keys, [(FSUM, c, F64)])
            assert code == ARG and "FSUM takes an FP64 column" in msg and "RJ_AGG_SUM" in msg, msg
        code, msg = bad(keys, [(FSUM, 2, I64)])
        assert code == ARG and "declared type" in msg, msg
        code, msg = bad(keys, [(FSUM, 3, F64)])
        assert code == UNSUPPORTED and "VARCHAR" in msg, msg
        for func in (6, 7, 9, 200):
            code, msg = bad(keys, [(func, 2, F64)])
            assert code == ARG and "unknown function code" in msg, (func, msg)
        code, msg = bad(keys, [(SUM, 2, I64)])
        assert code == UNSUPPORTED and "FP64" in msg and "SUM" in msg, msg
        code, msg = bad(keys, [(FSUM, 4, F64)])
        assert code == ARG and "out of range" in msg, msg
    p, sc = _scan_plan(cols)
    p.root = p.new_agg_node(sc, 0, [(KEY, 0, I32), (FSUM, 2, F64)])
    code, msg = _error(p)
    assert code == ARG and "RJ_NODE_GROUP" in msg and "FSUM" in msg, msg
    got, _ = check(group_plan(cols, [(0, 0)], [(KEY, 0, I32), (FSUM, 2, F64), (COUNT, 2, I64)]))
    assert (got.num_rows == 0) == (rows == 0)
