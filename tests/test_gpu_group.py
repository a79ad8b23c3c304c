"""Grouping nodes (RJ_NODE_GROUP) on the device, through the C-ABI, against the numpy reference
tests/_groupref.py (tests/test_group_plan.py ties it to a row-at-a-time dictionary on the CPU).  Every
result column is read by the strict page reader tests/_pagecheck.py first.

A grouping's result is one deterministic multiset whatever order the child's rows have (keys and FP64
MIN / MAX come out canonical, no function depends on the row order), and at the root its rows are in
the order of the keys: a root grouping is compared position by position, doubles by their bits; below
another node the plan's result is compared as a multiset.

Device path: the sort's kernels order the rows by the keys, then k_group_heads / k_group_scan find and
number the runs, k_group_keys / k_group_init / k_group_reduce / k_group_column produce the columns.  The
geometry is a tile of GROUP_TILE = 4096 positions (read from csrc/rj_device.hpp below), a quarter per
wave, 64 positions per item: the sizes below put group boundaries on and next to every one of these
borders.  RJ_TUNE_GROUP_GRID caps the workgroups of k_group_reduce, so that one workgroup walks several
tiles.  The one limit no quick test can reach is the row limit (2^32 - 16 child rows)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _groupref
import _pagecheck as pc
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
import test_group_plan as gp
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
KEY, STAR, COUNT, SUM, MIN, MAX = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX
_HPP = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
GROUP_TILE = int(re.search(r"constexpr int GROUP_TILE\s*=\s*(\d+);", _HPP).group(1))
assert GROUP_TILE == 4096
ROWS32, ROWS64 = (int(re.search(rf"constexpr uint32_t {n}\s*=\s*(\d+);", _HPP).group(1)) for n in ("ROWS32", "ROWS64"))
POISON = [{"RJ_DEBUG_POISON": str(m)} for m in (0x15A, 0x1FF)]
rng_for, group_plan, ALL_FLAGS = sp.rng_for, gp.group_plan, sp.ALL_FLAGS
fam = lambda ran, family: {n: c for n, c in ran.items() if n.split("<")[0] == family}
launches = lambda ran, prefix: {n: c for n, c in ran.items() if n.startswith(prefix)}
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
    return _groupref.decoded_rows([c.type for c in got.columns], dec, got.num_rows)


def _any_order(rows):
    cell = lambda v: (1, 0) if v is None else (0, v[1] if isinstance(v, tuple) else v)
    return sorted(rows, key=lambda r: tuple(cell(v) for v in r))


def check(p, env=None, what="", **kw):
    """Run plan p against the reference: a root grouping position by position (the order of the keys is
    promised there), any other root as a multiset."""
    got, ran = run(p, env, **kw)
    n, cols = _groupref.evaluate(p)
    node = p.nodes[p.root]
    assert got.num_rows == n, (what, got.num_rows, n)
    assert [c.type for c in got.columns] == [c[0] for c in cols], what
    rows, want = ordered_rows(got), _groupref.rel_rows(cols, n)
    if isinstance(node.data, pl.GroupNode):
        assert rows == want, what
    else:
        assert _any_order(rows) == _any_order(want), what
    return got, ran


# ------------------------------------------------------------------ row counts and run layouts
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, GROUP_TILE - 1, GROUP_TILE, GROUP_TILE + 1, 3 * GROUP_TILE + 1]
FORMS = ["one", "each", "random"]
OUTS = [(KEY, 0, I32), (STAR, 0, I64), (COUNT, 1, I64), (SUM, 1, I64), (MIN, 1, I64), (MAX, 1, I64), (SUM, 2, I64), (MAX, 2, I32)]


def sized_table(sizes, rng, shuffle=True):
    """an INT32 key whose groups have these sizes in the order of the key, a nullable INT64 value and a
    paged INT32 value"""
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    key = np.repeat(np.arange(sizes.shape[0]) * 3 - 7, sizes).astype(np.int32)
    if shuffle:
        key = key[rng.permutation(n)]
    return [(I32, key), (I64, rng.integers(-2**40, 2**40, n), rng.random(n) >= 0.3), (I32, rng.integers(-2**31, 2**31, n).astype(np.int32))]


def form_sizes(n, form, rng):
    if form == "one":
        return [n]
    if form == "each":
        return np.ones(n, dtype=np.int64)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 201)), n - sum(sizes)))
    return sizes


def grid_case(n, form, env=None):
    rng = rng_for("grid", n, form)
    cols = sized_table(form_sizes(n, form, rng), rng)
    got, ran = check(group_plan(cols, [(0, 0)], OUTS), env, what=(n, form))
    if form == "one":   # every key digit is constant: no sort pass, no permutation
        assert not fam(ran, "k_sort_scatter") and got.num_rows == 1
    if form == "each":
        assert got.num_rows == n
    return got, ran


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_size_grid(n, form):
    grid_case(n, form)


LAYOUTS = {
    "ends-at-64-1024-tile": [64, 960, GROUP_TILE - 1024, 1, 63, 64 + 1024, 5],
    "ends-one-before-and-after": [63, 2, 959, 1, GROUP_TILE - 1025, 2, 100],
    "three-whole-tiles": [GROUP_TILE - 3, 3 * GROUP_TILE + 10, 7],
    "three-whole-tiles-aligned": [GROUP_TILE, 3 * GROUP_TILE, GROUP_TILE, 1],
    "a-wave-quarter-each": [1024] * 9 + [3],
    "single-rows-around-a-long-run": [1] * 70 + [2 * GROUP_TILE] + [1] * 70,
}


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffled"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_runs_that_end_on_item_wave_and_tile_borders(layout, shuffle):
    cols = sized_table(LAYOUTS[layout], rng_for("layout", layout), shuffle)
    got, ran = check(group_plan(cols, [(0, 0)], OUTS), what=layout)
    assert got.num_rows == len(LAYOUTS[layout])
    assert np.array_equal(pl.decode_table(got)[1][0], LAYOUTS[layout])          # COUNT(*): the run lengths, in key order
    assert fam(ran, "k_sort_scatter")


# ------------------------------------------------------------------ carry across tiles and workgroups
@pytest.mark.parametrize("grid", [1, 3])
def test_one_workgroup_walks_several_tiles(grid):
    """n = 5 tiles + 7 rows on 1 or 3 workgroups: groups across a tile boundary inside a workgroup's run
    and across the boundary of two runs"""
    env = {"RJ_TUNE_GROUP_GRID": str(grid)}
    n = 5 * GROUP_TILE + 7
    for form in FORMS:
        got, ran = grid_case(n, form, env)
        assert ran.get("k_group_reduce<8,true>") == 1 and ran.get("k_group_reduce<4,true>") == 1
    for layout, sizes in sorted(LAYOUTS.items()):
        sizes = list(sizes) + [n]
        cols = sized_table(sizes, rng_for("carry", layout, grid))
        got, _ = check(group_plan(cols, [(0, DESC)], OUTS), env, what=(layout, grid))
        assert np.array_equal(pl.decode_table(got)[1][0], sizes[::-1])
    # one group over everything, no key at all
    cols = sized_table([n], rng_for("carry-scalar", grid))
    _, ran = check(group_plan(cols, [], OUTS[1:]), env)
    assert ran.get("k_group_reduce<8,false>") == 1 and ran.get("k_group_reduce<4,false>") == 1     # the variant without heads


# ------------------------------------------------------------------ result pages
@pytest.mark.parametrize("nulls", [False, True], ids=["no-nulls", "nulls"])
@pytest.mark.parametrize("count", [ROWS32 - 1, ROWS32, ROWS32 + 1, ROWS64 - 1, ROWS64, ROWS64 + 1])
def test_group_counts_around_one_result_pages_capacity(count, nulls):
    rng = rng_for("pages", count, nulls)
    valid = rng.random(count) >= 0.3 if nulls else np.ones(count, bool)
    cols = [(I32, rng.permutation(count).astype(np.int32)), (I64, rng.integers(-2**62, 2**62, count)),
            (I32, rng.integers(-9, 9, count).astype(np.int32), valid)]
    # every row its own group: `count` rows of 4- and 8-byte columns, MIN / SUM NULL where the row's value is
    got, ran = check(group_plan(cols, [(1, 0), (0, 0)], [(KEY, 0, I32), (KEY, 1, I64), (MIN, 2, I32), (SUM, 2, I64), (STAR, 0, I64)]), what=(count, nulls))
    assert got.num_rows == count
    assert got.columns[0].pages.shape[0] == -(-count // ROWS32) and got.columns[1].pages.shape[0] == -(-count // ROWS64)
    assert got.columns[4].pages.shape[0] == -(-count // ROWS64) and bool(fam(ran, "k_encode_nullable")) == nulls


# ------------------------------------------------------------------ keys
@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_edge_values_of_every_key_type_under_every_flag(dt, flags):
    """the edge list of tests/test_sort_plan.py (NULL, both zeros, NaNs of either sign and several payloads,
    the infinities, the extremes), every value three times: the ROW ORDER and the canonical values"""
    bits = [b for _, b in sp.EDGES[dt]] * 3
    null = [v is None for v, _ in sp.EDGES[dt]] * 3
    at = rng_for("edges", dt, flags).permutation(len(bits))
    raw = np.array(bits, dtype=np.uint64)[at]
    vals = raw.astype(np.uint32).view(np.int32) if dt == I32 else raw.view(km.NP_OF[dt])
    cols = [(dt, vals, ~np.array(null)[at]), (I32, np.arange(len(bits), dtype=np.int32))]
    got, _ = check(group_plan(cols, [(0, flags)], [(KEY, 0, dt), (STAR, 0, I64), (MIN, 1, I32), (MIN, 0, dt), (MAX, 0, dt)]), what=(dt, flags))
    rows = ordered_rows(got)
    distinct = len(sp.EDGES[dt]) - (4 if dt == F64 else 0)      # -0.0 = +0.0, four NaNs are one
    assert len(rows) == distinct
    nulls = [r[0] is None for r in rows]
    assert nulls == sorted(nulls, reverse=bool(flags & NF)) and sum(nulls) == 1
    assert [r[1] for r in rows if r[0] is not None and r[0] != ("f64", gp.CANON_NAN) and r[0] != ("f64", 0)] == [3] * (distinct - (3 if dt == F64 else 1))
    if dt == F64:
        assert ("f64", gp.CANON_NAN) in [r[0] for r in rows] and ("f64", 0) in [r[0] for r in rows]
        assert {r[0]: r[1] for r in rows}[("f64", gp.CANON_NAN)] == 12 and {r[0]: r[1] for r in rows}[("f64", 0)] == 6


def test_every_null_pattern_over_two_nullable_keys():
    rng = rng_for("nullpat")
    n = 3_000
    cols = [(I32, rng.integers(0, 3, n).astype(np.int32), rng.random(n) >= 0.4), (I64, rng.integers(0, 3, n), rng.random(n) >= 0.4),
            (I64, rng.integers(-99, 99, n), rng.random(n) >= 0.5)]
    for f0 in ALL_FLAGS:
        for f1 in (0, DESC | NF):
            got, _ = check(group_plan(cols, [(0, f0), (1, f1)], [(KEY, 1, I64), (KEY, 0, I32), (STAR, 0, I64), (SUM, 2, I64)]), what=(f0, f1))
            assert got.num_rows == 16            # (3 values + NULL) squared: (NULL, x), (x, NULL) and (NULL, NULL) are groups of their own


@pytest.mark.parametrize("n_keys", range(1, 9))
def test_one_to_eight_keys_of_mixed_types(n_keys):
    rng = rng_for("keys", n_keys)
    n = 4_000
    types = [I32, I64, F64, I32, I64, F64, I32, I64]
    cols = [(dt, rng.integers(0, 2, n).astype(km.NP_OF[dt]), rng.random(n) >= 0.1) for dt in types] + [(I64, rng.integers(-2**62, 2**62, n))]
    keys = [(int(c), int(rng.integers(0, 4))) for c in rng.permutation(8)[:n_keys]]
    outs = [(KEY, c, types[c]) for c, _ in keys] + [(STAR, 0, I64), (SUM, 8, I64), (MAX, 8, I64)]
    got, ran = check(group_plan(cols, keys, outs), what=keys)
    assert got.num_rows == len(set(zip(*[np.where(cols[k][2], cols[k][1], -1).tolist() for k, _ in keys])))
    assert sum(fam(ran, "k_sort_encode").values()) == n_keys and sum(fam(ran, "k_group_heads").values()) == n_keys


def test_three_key_types_and_mixed_directions_with_heavy_ties():
    cols = sp.key_table(rng_for("mixed"), 6_000, sp.TYPES, domain=3)
    for keys in ([(0, DESC), (2, NF)], [(3, 0), (1, DESC | NF), (4, DESC)], [(2, DESC | NF), (0, 0), (1, 0)], [(4, 0)]):
        check(group_plan(cols, keys, gp.all_outputs(sp.TYPES, keys)), what=keys)


def test_a_key_column_that_repeats_and_a_key_that_is_not_output():
    cols = sp.key_table(rng_for("twice"), 5_000, sp.TYPES, domain=4)
    a, ran = check(group_plan(cols, [(1, 0), (1, DESC), (2, 0)], [(STAR, 0, I64), (KEY, 2, F64), (KEY, 2, F64)]))
    assert sum(fam(ran, "k_sort_encode").values()) == 2 and sum(fam(ran, "k_group_heads").values()) == 2
    b, _ = run(group_plan(cols, [(1, 0), (2, 0)], [(STAR, 0, I64), (KEY, 2, F64), (KEY, 2, F64)]))
    assert ordered_rows(a) == ordered_rows(b)
    check(group_plan(cols, [(1, DESC), (1, 0)], [(KEY, 1, I64), (MIN, 1, I64), (KEY, 1, I64)]))


# ------------------------------------------------------------------ aggregates
def test_every_function_on_every_legal_type_and_a_group_without_a_value():
    rng = rng_for("functions")
    n = 5_000
    types = [I32, I32, I64, F64]
    k = rng.integers(0, 40, n).astype(np.int32)
    cols = [(I32, k, rng.random(n) >= 0.05)]
    for dt in types[1:]:
        valid = (rng.random(n) >= 0.3) & (k != 7)        # the group of key 7 holds no value at all
        cols.append((dt, (rng.integers(-1000, 1000, n) * (0.25 if dt == F64 else 1)).astype(km.NP_OF[dt]), valid))
    got, _ = check(group_plan(cols, [(0, 0)], gp.all_outputs(types, [(0, 0)])))
    row7 = [r for r in ordered_rows(got) if r[0] == 7][0]
    outs = gp.all_outputs(types, [(0, 0)])
    for (func, c, _), v in zip(outs, row7):
        if c in (1, 2, 3) and func != STAR:
            assert v == (0 if func == COUNT else None), (func, c, v)


def test_sums_wrap_and_extremes_are_not_sentinels():
    n = 2 * GROUP_TILE + 11
    rng = rng_for("extremes")
    k = rng.integers(0, 5, n).astype(np.int32)
    i64 = rng.choice(np.array([2**63 - 1, -2**63, 2**62, -1, 0], dtype=np.int64), n)
    i32 = rng.choice(np.array([2**31 - 1, -2**31, 0, -1], dtype=np.int32), n)
    i64[k == 0], i32[k == 0] = 2**63 - 1, 2**31 - 1          # a group of only the maximum: MIN is the maximum
    i64[k == 1], i32[k == 1] = -2**63, -2**31                # ... of only the minimum: MAX is the minimum
    cols = [(I32, k), (I64, i64, rng.random(n) >= 0.1), (I32, i32, rng.random(n) >= 0.1)]
    outs = [(KEY, 0, I32), (SUM, 1, I64), (MIN, 1, I64), (MAX, 1, I64), (SUM, 2, I64), (MIN, 2, I32), (MAX, 2, I32), (COUNT, 1, I64)]
    got, _ = check(group_plan(cols, [(0, 0)], outs))
    rows = ordered_rows(got)
    assert rows[0][2] == rows[0][3] == 2**63 - 1 and rows[0][5] == rows[0][6] == 2**31 - 1
    assert rows[1][2] == rows[1][3] == -2**63 and rows[1][5] == rows[1][6] == -2**31
    assert abs(int(i64[(k == 0) & cols[1][2]].astype(object).sum())) > 2**63     # the true sum does not fit: it wrapped
    check(group_plan(cols, [], outs[1:]))


def test_fp64_min_max_over_nan_infinities_zeros_and_denormals():
    bits = np.array([b for v, b in sp.EDGES[F64] if v is not None], dtype=np.uint64)
    rng = rng_for("f64")
    n = 3_000
    k = rng.integers(0, 30, n).astype(np.int32)
    v = bits[rng.integers(0, bits.shape[0], n)].view(np.float64)
    v[k == 3] = np.array([sp.NEG_NAN], dtype=np.uint64).view(np.float64)[0]     # only NaNs: MIN is the canonical NaN
    v[k == 4] = -0.0                                                             # only -0.0: MIN = MAX = +0.0
    v[k == 5] = -np.inf
    cols = [(I32, k), (F64, v, rng.random(n) >= 0.2)]
    got, _ = check(group_plan(cols, [(0, 0)], [(KEY, 0, I32), (MIN, 1, F64), (MAX, 1, F64), (COUNT, 1, I64)]))
    rows = {r[0]: r for r in ordered_rows(got)}
    assert rows[3][1] == rows[3][2] == ("f64", gp.CANON_NAN) and rows[4][1] == rows[4][2] == ("f64", 0)
    assert rows[5][1] == rows[5][2] == ("f64", sp.bits_of(-np.inf) - 2**64)


def test_twelve_outputs_over_six_columns_behind_an_int64_key():
    """what RJ_NODE_AGG refuses (its carry limit), RJ_NODE_GROUP runs"""
    rng = rng_for("twelve")
    n = 6_000
    cols = [(I64, rng.integers(-50, 50, n) * 2**33, rng.random(n) >= 0.05)]
    cols += [(dt, rng.integers(-2**20, 2**20, n).astype(km.NP_OF[dt]), rng.random(n) >= 0.2) for dt in (I32, I64, I32, I64, I32, I64)]
    outs = [(KEY, 0, I64), (STAR, 0, I64), (SUM, 1, I64), (COUNT, 1, I64), (MIN, 2, I64), (COUNT, 2, I64), (MAX, 3, I32), (COUNT, 3, I64),
            (SUM, 4, I64), (COUNT, 4, I64), (MIN, 5, I32), (MAX, 6, I64)]
    assert len(outs) == 12 and len({c for f, c, _ in outs if f not in (KEY, STAR)}) == 6
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    p.root = p.new_agg_node(sc, 0, outs)
    p.new_input(pl.make_table(cols))
    code, msg = _error(p)
    assert code == UNSUPPORTED and "carry words" in msg
    check(group_plan(cols, [(0, 0)], outs))


# ------------------------------------------------------------------ the scalar aggregate, DISTINCT
def _typed_empty(types):
    return [(dt, np.zeros(0, km.NP_OF[dt])) if dt != VC else (VC, []) for dt in types]


def test_scalar_aggregate_over_no_rows_one_row_and_many_workgroups():
    outs = [(STAR, 0, I64), (COUNT, 1, I64), (SUM, 1, I64), (MIN, 1, I64), (MAX, 0, I32), (MIN, 2, F64)]
    got, ran = check(group_plan(_typed_empty([I32, I64, F64]), [], outs))
    assert ordered_rows(got) == [(0, 0, None, None, None, None)]
    assert not fam(ran, "k_group_reduce") and fam(ran, "k_group_init")           # the identities are the result
    got, _ = check(group_plan([(I32, np.array([-5], np.int32)), (I64, np.array([9])), (F64, np.array([-0.0]))], [], outs))
    assert ordered_rows(got) == [(1, 1, 9, 9, -5, ("f64", 0))]
    n = 300_000
    rng = rng_for("scalar")
    cols = [(I32, rng.integers(-2**31, 2**31, n).astype(np.int32)), (I64, rng.integers(-2**62, 2**62, n), rng.random(n) >= 0.01), (F64, rng.random(n))]
    got, ran = check(group_plan(cols, [], outs))
    assert got.num_rows == 1 and not launches(ran, "k_sort_") and not fam(ran, "k_group_heads") and not fam(ran, "k_group_scan")
    assert sum(fam(ran, "k_group_reduce").values()) == 3                          # one launch per distinct column; COUNT(*) rides along


def test_distinct_over_two_columns():
    rng = rng_for("distinct")
    n = 20_000
    cols = [(I32, rng.integers(0, 40, n).astype(np.int32), rng.random(n) >= 0.02), (F64, rng.integers(-3, 3, n) * 0.5, rng.random(n) >= 0.02),
            (I64, np.arange(n))]
    got, ran = check(group_plan(cols, [(0, 0), (1, DESC)], [(KEY, 0, I32), (KEY, 1, F64)]))
    pairs = got.num_rows
    assert 41 * 6 <= pairs <= 41 * 7 and not fam(ran, "k_group_reduce") and not fam(ran, "k_group_init")
    got, _ = check(group_plan(cols, [(0, 0), (1, DESC)], []))                     # no output at all: the group count
    assert got.num_rows == pairs and not got.columns


# ------------------------------------------------------------------ agreement with the hashed path
@pytest.mark.parametrize("seed", range(20))
def test_same_multiset_as_the_hashed_aggregation(seed):
    rng = rng_for("hashed", seed)
    n = int(rng.integers(1, 30_000))
    kt, vt = [I32, I64][seed % 2], [I32, I64][(seed // 2) % 2]
    card = int(rng.integers(1, n + 1))
    cols = [(kt, km.key_values(kt, rng.integers(0, card, n)), rng.random(n) >= [0.0, 0.1][seed % 3 == 0]),
            (vt, rng.integers(-2**31, 2**31, n).astype(km.NP_OF[vt]), rng.random(n) >= [0.0, 0.3][seed % 4 == 0])]
    outs = [(KEY, 0, kt), (STAR, 0, I64), (COUNT, 1, I64), (SUM, 1, I64), (MIN, 1, vt), (MAX, 1, vt)]
    a, _ = run(group_plan(cols, [(0, int(rng.integers(0, 4)))], outs))
    p = pl.Plan()
    sc = p.new_scan_node(0, [(0, kt), (1, vt)])
    p.root = p.new_agg_node(sc, 0, outs)
    p.new_input(pl.make_table(cols))
    b, ran = run(p)
    assert fam(ran, "k_agg_parts") and a.num_rows == b.num_rows
    assert _any_order(ordered_rows(a)) == _any_order(ordered_rows(b))


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


@pytest.mark.parametrize("kind", ["scan", "join", "outer", "select", "sort", "agg", "group"])
def test_grouping_as_the_root_over_every_kind(kind):
    """paged and nullable columns of a scan read in place, dense columns of a join, ..."""
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
        child, types = p.new_agg_node(sa, 0, [(KEY, 0, I32), (STAR, 0, I64), (SUM, 1, I64)]), [I32, I64, I64]
    else:
        child, types = p.new_group_node(sa, [(0, DESC)], [(KEY, 0, I32), (STAR, 0, I64), (MAX, 1, I64)]), [I32, I64, I64]
    last = len(types) - 1
    keys = [(last, NF | DESC)] if kind in ("agg", "group") else [(0, 0), (last, NF | DESC)][: 1 if kind in ("scan", "select", "sort") else 2]
    p.root = p.new_group_node(child, keys, gp.all_outputs(types, keys))
    got, ran = check(p, what=kind)
    assert got.num_rows > 1 and fam(ran, "k_group_heads") and fam(ran, "k_group_reduce")


@pytest.mark.parametrize("kind", ["join", "semi", "select", "sort", "group", "agg"])
def test_every_kind_over_a_grouping(kind):
    p, sa, sb = _two_scans(*_pb(rng_for("under", kind)))
    g = p.new_group_node(sa, [(0, NF)], [(KEY, 0, I32), (STAR, 0, I64), (MIN, 1, I64), (SUM, 1, I64)])
    if kind == "join":        # joins on the key column the grouping produced (the NULL group drops out)
        p.root = p.new_join_node(True, g, sb, 0, 0, [(0, I32), (1, I64), (2, I64), (5, I32)])
    elif kind == "semi":
        p.root = p.new_semi_join_node(False, g, sb, 0, 0, [(0, I32), (3, I64)])
    elif kind == "select":    # HAVING COUNT(*) >= 8 OR MIN(x) IS NULL
        p.root = p.new_select_node(g, [("GEQ", 1, 8), ("IS_NULL", 2), ("OR",)], [(0, I32), (1, I64), (2, I64)])
    elif kind == "sort":
        p.root = p.new_sort_node(g, [(1, DESC), (0, 0)], [(0, I32), (1, I64), (3, I64)], limit=50)
    elif kind == "group":     # how many keys have each count
        p.root = p.new_group_node(g, [(1, DESC)], [(KEY, 1, I64), (STAR, 0, I64), (MIN, 0, I32), (MAX, 3, I64)])
    else:
        p.root = p.new_agg_node(g, 1, [(KEY, 1, I64), (STAR, 0, I64), (MAX, 0, I32)])
    got, ran = check(p, what=kind)
    assert got.num_rows > 1 and fam(ran, "k_group_reduce")


def test_same_plan_twice_on_one_context():
    cols = sp.key_table(rng_for("twice"), 10_000, sp.TYPES, domain=5)
    p = group_plan(cols, [(2, DESC), (0, NF)], gp.all_outputs(sp.TYPES, [(2, 0), (0, 0)]))
    a, _ = run(p)
    b, _ = run(p)
    assert a.num_rows == b.num_rows > 1 and ordered_rows(a) == ordered_rows(b)


def test_resident_tables_and_results_kept_on_the_device():
    cols = sized_table(form_sizes(50_000, "random", rng_for("resident")), rng_for("resident", 2))
    p = group_plan(cols, [(0, DESC)], OUTS)
    n, ref = _groupref.evaluate(p)
    want = _groupref.rel_rows(ref, n)
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


# ------------------------------------------------------------------ fuzz
def fuzz_case(seed):
    rng = rng_for("fuzz", seed)
    n = int(rng.integers(1, 3_000)) if rng.random() < 0.75 else int(rng.integers(3_000, 70_001))
    types = [[I32, I64, F64][int(rng.integers(0, 3))] for _ in range(4)]
    null_p = [0.0, 0.05, 0.5][int(rng.integers(0, 3))]
    card = int(rng.integers(1, n + 1)) if rng.random() < 0.5 else int(rng.integers(1, 40))   # distinct values per column: 1 .. n
    cols = []
    for dt in types:
        v = rng.integers(-(card // 2), card - card // 2, n)
        cols.append((dt, (v * 0.5).astype(np.float64) if dt == F64 else v.astype(km.NP_OF[dt]), rng.random(n) >= null_p))
    edge = sp.key_table(rng, min(n, 16), types, null_p=null_p)                    # ... and the edge values of every type
    cols = [(dt, np.concatenate([e[1], v[e[1].shape[0]:]]), m) for (dt, v, m), e in zip(cols, edge)]
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, dt) for i, dt in enumerate(types)])
    p.new_input(pl.make_table(cols))
    every = [(i, dt) for i, dt in enumerate(types)]
    child, kind = sc, ["scan", "select", "join", "sort", "group"][int(rng.integers(0, 5))]
    if kind == "select":
        child = p.new_select_node(sc, [("IS_NOT_NULL", 0), ("IS_NULL", 1), ("OR",)], every)
    elif kind == "join" and types[0] != F64:
        other = p.new_scan_node(0, [(0, types[0])])
        child = p.new_semi_join_node(False, sc, other, 0, 0, every)
    elif kind == "sort":
        child = p.new_sort_node(sc, [(1, DESC)], every)
    elif kind == "group":
        child = p.new_group_node(sc, [(0, 0), (1, 0)], [(KEY, 0, types[0]), (KEY, 1, types[1]), (STAR, 0, I64), (MAX, 2, types[2])])
        types = [types[0], types[1], I64, types[2]]
    nk = int(rng.integers(0, 4))
    keys = [(int(rng.integers(0, len(types))), int(rng.integers(0, 4))) for _ in range(nk)]
    p.root = p.new_group_node(child, keys, gp.all_outputs(types, keys, rng))
    return p


@pytest.mark.parametrize("block", range(15))
def test_fuzz(block):
    """150 seeded cases, ten per block: key count (0 .. 3), types, NULL rate, cardinality, outputs, child kind"""
    rows = 0
    for seed in range(10 * block, 10 * block + 10):
        got, _ = check(fuzz_case(seed), what=seed)
        rows += got.num_rows
    assert rows > 0


# ------------------------------------------------------------------ dirty memory
@pytest.mark.parametrize("part", ["one", "each", "random", "fuzz-a", "fuzz-b", "fuzz-c"])
@pytest.mark.parametrize("env", POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env, part):
    """nothing may rely on zeroed memory: the block cache hands out filled blocks.  The row-count grid
    and 30 fuzz cases per fill pattern."""
    if part in FORMS:
        for n in SIZES:
            grid_case(n, part, env)
        check(group_plan(_typed_empty([I32, I64]), [], [(STAR, 0, I64), (SUM, 1, I64)]), env)
    else:
        first = 1_000 + 10 * "abc".index(part[-1])
        for seed in range(first, first + 10):
            check(fuzz_case(seed), env, what=seed)
    s = context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


# ------------------------------------------------------------------ the launch log
def test_launch_log_shows_the_group_kernels_and_the_skipped_sorts():
    n = 2 * GROUP_TILE + 5
    rng = rng_for("log")
    cols = [(I32, rng.integers(0, 50, n).astype(np.int32)), (I64, np.full(n, 77)), (I64, rng.integers(0, 9, n), rng.random(n) >= 0.5)]
    outs = [(KEY, 0, I32), (KEY, 1, I64), (STAR, 0, I64), (SUM, 2, I64), (MIN, 2, I64), (MAX, 0, I32)]
    _, ran = check(group_plan(cols, [(0, 0), (1, 0)], outs))
    for f in ("k_group_heads", "k_group_scan", "k_group_keys", "k_group_init", "k_group_reduce", "k_group_column"):
        assert fam(ran, f), (f, ran)
    assert ran["k_group_heads<4>"] == 1 and ran["k_group_heads<8>"] == 1 and ran["k_group_keys<4>"] == 1 and ran["k_group_keys<8>"] == 1
    assert ran["k_group_reduce<8,true>"] == 1 and ran["k_group_reduce<4,true>"] == 1 and len(fam(ran, "k_group_reduce")) == 2   # several functions: one launch
    assert sum(fam(ran, "k_sort_encode").values()) == 2 and sum(fam(ran, "k_sort_scatter").values()) == 1      # [0, 50): one digit
    # a key column whose values are all equal: no scatter; COUNT(*) alone: the column-less reduce
    _, ran = check(group_plan(cols, [(1, DESC)], [(STAR, 0, I64), (KEY, 1, I64)]))
    assert fam(ran, "k_sort_encode") and not fam(ran, "k_sort_scatter") and not fam(ran, "k_sort_count")
    assert ran.get("k_group_reduce<0,true>") == 1 and len(fam(ran, "k_group_reduce")) == 1
    # the scalar aggregate: no sort kernel at all
    _, ran = check(group_plan(cols, [], outs[2:]))
    assert not launches(ran, "k_sort_") and not fam(ran, "k_group_heads") and not fam(ran, "k_group_keys")
    assert set(fam(ran, "k_group_reduce")) == {"k_group_reduce<8,false>", "k_group_reduce<4,false>"}


# ------------------------------------------------------------------ the error contract
def _error(p, ctx=None):
    with pytest.raises(capi.RjError) as e:
        capi.execute(p, ctx or context())
    return e.value.code, str(e.value)


@pytest.mark.parametrize("rows", [300, 0], ids=["rows", "empty-child"])
def test_error_contract(rows):
    """every refusal, also over an empty child: the node is checked before its child's rows are looked at"""
    rng = rng_for("err")
    types = [I32, I64, F64, VC, I32]
    if rows:
        cols = [km.payload(rng, I32, rows, True), km.payload(rng, I64, rows, False), km.payload(rng, F64, rows, True),
                km.payload(rng, VC, rows, False), (I32, rng.integers(0, 10, rows).astype(np.int32))]
    else:
        cols = _typed_empty(types)
    ok = [(KEY, 0, I32), (STAR, 0, I64)]
    bad = lambda keys, outs=ok: _error(group_plan(cols, keys, outs))
    # RJ_ERR_ARG
    for keys, text in (([(5, 0)], "key column out of range"), ([(-1, 0)], "key column out of range"), ([(0, 0), (99, DESC)], "out of range"),
                       ([(0, 4)], "flags"), ([(0, -1)], "flags"), ([(1, 1 | 2 | 8)], "flags")):
        code, msg = bad(keys, [(STAR, 0, I64)])
        assert code == ARG and text in msg, (keys, msg)
    for outs, text in (([(SUM, 5, I64)], "output attr out of range"), ([(KEY, 7, I32)], "output attr out of range"),
                       ([(6, 1, I64)], "unknown function code"), ([(200, 0, I64)], "unknown function code"),
                       ([(KEY, 4, I32)], "not a key"), ([(KEY, 1, I64)], "not a key"), ([(STAR, 1, I64)], "COUNT(*) takes no column"),
                       ([(KEY, 0, I64)], "declared type"), ([(STAR, 0, I32)], "declared type"), ([(COUNT, 1, I32)], "declared type"),
                       ([(SUM, 4, I32)], "declared type"), ([(MIN, 1, I32)], "declared type"), ([(MAX, 2, I64)], "declared type"),
                       ([(MIN, 4, I64)], "declared type")):
        code, msg = bad([(0, 0)], outs)
        assert code == ARG and text in msg, (outs, msg)
    code, msg = bad([], [(KEY, 0, I32)])                  # without keys no column is a key
    assert code == ARG and "not a key" in msg
    # keys announced, none given
    p = group_plan(cols, [(0, 0)], ok)
    cplan, keep = pl.plan_to_c(p)
    cplan.nodes[p.root].right_attr = 0
    c = context()
    out = C.c_void_p()
    rc = c.L.rj_execute(c.h, C.byref(cplan), C.byref(out))
    assert rc == ARG and b"NULL key pointer" in c.L.rj_last_error(c.h)
    del keep
    # RJ_ERR_UNSUPPORTED
    for keys, outs in (([(3, 0)], [(STAR, 0, I64)]), ([(0, 0), (3, DESC)], ok)):
        code, msg = bad(keys, outs)
        assert code == UNSUPPORTED and "VARCHAR key" in msg, msg
    for func in (COUNT, MIN, MAX, SUM):
        code, msg = bad([(0, 0)], [(func, 3, I64 if func in (COUNT, SUM) else VC)])
        assert code == UNSUPPORTED and "VARCHAR" in msg, msg
    code, msg = bad([(0, 0)], [(SUM, 2, I64)])
    assert code == UNSUPPORTED and "FP64" in msg and "SUM" in msg
    code, msg = bad([(k % 3, 0) for k in range(9)], [(STAR, 0, I64)])
    assert code == UNSUPPORTED and "8" in msg
    # eight keys are fine, and so is a VARCHAR column that the node does not name
    got, _ = check(group_plan(cols, [(k % 3, k % 4) for k in range(8)], [(KEY, 2, F64), (STAR, 0, I64), (COUNT, 2, I64), (MAX, 2, F64)]))
    assert (got.num_rows == 0) == (rows == 0)


def test_execute_sharded_refuses_and_a_two_device_context_runs_on_one():
    cols = sized_table(form_sizes(5_000, "random", rng_for("two")), rng_for("two", 2))
    p = group_plan(cols, [(0, DESC | NF)], OUTS)
    got, _ = check(p, devices=[0, 0])
    assert got.num_rows > 1
    ctx = context(devices=[0, 0])
    tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
    try:
        with pytest.raises(capi.RjError) as e:
            ctx.execute_sharded(p, tables)
        assert e.value.code == UNSUPPORTED and "RJ_NODE_GROUP" in str(e.value)
    finally:
        for row in tables:
            for t in row:
                t.release()


def test_empty_child_with_keys_gives_typed_columns_without_pages():
    got, ran = check(group_plan(_typed_empty([I32, I64, F64, VC]), [(0, 0), (2, DESC)], [(KEY, 2, F64), (STAR, 0, I64), (MIN, 1, I64), (KEY, 0, I32)]))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [F64, I64, I64, I32]
    assert all(c.pages.shape[0] == 0 for c in got.columns) and not launches(ran, "k_group_") and not launches(ran, "k_sort_")


# ------------------------------------------------------------------ every compiled instantiation
def test_every_group_instantiation_is_driven():
    import _elfsyms
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.startswith("k_group_")}
    cols = sp.key_table(rng_for("matrix"), GROUP_TILE + 1, [I32, I64, F64])
    reached = set()
    for p in (group_plan(cols, [(0, 0), (1, DESC)], [(KEY, 0, I32), (KEY, 1, I64), (MIN, 0, I32), (MAX, 2, F64)]),
              group_plan(cols, [(2, NF)], [(STAR, 0, I64)]), group_plan(cols, [], [(STAR, 0, I64)]),
              group_plan(cols, [], [(MIN, 0, I32), (MAX, 2, F64)])):
        reached |= set(launches(check(p)[1], "k_group_"))
    assert reached == compiled, sorted(compiled - reached)
