"""Map nodes (RJ_NODE_MAP) on the device, through the C-ABI, against the numpy reference tests/_mapref.py
(tests/test_map_plan.py ties it to a row-at-a-time evaluator and to rj_debug_map_eval on the CPU).
Results are compared bit for bit (pl.canonical_rows; row by row IN ORDER where rj.h promises an order),
and every result column is read by the strict page reader tests/_pagecheck.py first.  No tolerance: +, -,
*, / and the conversions are correctly rounded on both sides, and NaNs come out canonical.

Device path: k_map (csrc/rj_map.hip) evaluates all expressions of a node in one launch over tiles of
MAP_TILE rows (read from csrc/rj_expr.hpp); RJ_TUNE_MAP_GRID caps its grid, so that a small input makes
one workgroup walk several tiles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _elfsyms
import _mapref
import _pagecheck as pc
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
import test_map_plan as mp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
KEY, STAR, SUM = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_SUM
ARG, UNSUPPORTED = 1, 5
_CSRC = os.path.join(os.path.dirname(km.LIB), "csrc")
MAP_TILE = int(re.search(r"constexpr int MAP_TILE\s*=\s*(\d+);", open(os.path.join(_CSRC, "rj_expr.hpp")).read()).group(1))
_HPP = open(os.path.join(_CSRC, "rj_device.hpp")).read()
ROWS32, ROWS64 = (int(re.search(rf"constexpr uint32_t {n}\s*=\s*(\d+);", _HPP).group(1)) for n in ("ROWS32", "ROWS64"))
VDEV = {"RJ_TUNE_VARCHAR_DEV": "1"}
POISON = [{"RJ_DEBUG_POISON": str(m)} for m in (0x15A, 0x1FF)]
GRIDS = [None, {"RJ_TUNE_MAP_GRID": "1"}, {"RJ_TUNE_MAP_GRID": "3"}]
rng_for, map_plan = mp.rng_for, mp.map_plan
fam = lambda ran, family: {n: c for n, c in ran.items() if n.split("<")[0] == family}
O = ("OUT",)

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


def _canon(rows):
    import struct
    return [tuple(("f64", struct.unpack("<q", struct.pack("<d", v))[0]) if isinstance(v, float) else v for v in r) for r in rows]


def same(got, want, what="", ordered=False):
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    dec = pc.check_table(got)  # the format of every column, then the content
    assert pc.same_as(dec, pl.decode_table(got)), what
    if ordered:
        assert _canon(pl.table_rows(got)) == _canon(pl.table_rows(want)), what
    else:
        assert pc.canonical_rows(dec) == pl.canonical_rows(want), what


def check(p, env=None, what="", ordered=False, **kw):
    got, ran = run(p, env, **kw)
    same(got, _mapref.execute(p), what, ordered)
    return got, ran


# ------------------------------------------------------------------ sizes where the kernel switches branches
SIZES = [1, 63, 64, 65, 255, 256, 257, MAP_TILE - 1, MAP_TILE, MAP_TILE + 1, 5 * MAP_TILE + 17,
         ROWS64 - 1, ROWS64 + 1, ROWS32 - 1, ROWS32 + 1]
GRID_PROG = [("COL", 0), ("INT", 3), ("MUL",), ("INT", 1), ("ADD",), O,             # names its row
             ("COL", 1), ("COL", 0), ("ADD",), O, ("COL", 2), ("F64", 0.5), ("MUL",), ("COL", 0), ("TO_F64",), ("ADD",), O]
GRID_OUTS = [("EXPR", 0, I64), ("EXPR", 1, I64), ("COL", 0, I32), ("EXPR", 2, F64), ("EXPR", 0, I32)]


def grid_table(n, form, rng):
    """position, an INT64 and an FP64 payload; form "nulls": the payloads with NULLs (dense values +
    validity on the device)"""
    cols = [(I32, np.arange(n, dtype=np.int32)), (I64, rng.integers(-2**62, 2**62, n)), (F64, rng.standard_normal(n))]
    if form == "nulls":
        cols = [cols[0]] + [(dt, v, rng.random(n) >= 0.1) for dt, v in cols[1:]]
    return cols


def grid_case(n, form, env=None):
    cols = grid_table(n, form, rng_for("grid", n, form))
    got, ran = check(map_plan(cols, GRID_PROG, GRID_OUTS), env, what=(n, form, env), ordered=True)
    assert sum(fam(ran, "k_map").values()) == 1
    assert pl.decode_table(got)[0][0].tolist() == [3 * i + 1 for i in range(n)]


@pytest.mark.parametrize("form", ["paged", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_size_grid(n, form):
    for env in GRIDS:
        grid_case(n, form, env)


# ------------------------------------------------------------------ the CPU edge grid as columns
def _every(ops, arity=2):
    prog = []
    for op in ops:
        prog += [("COL", k) for k in range(arity)] + [(op,), O]
    return prog


@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_every_op_over_the_edge_grid(dt):
    edges = {I32: mp.I32_EDGES, I64: mp.I_EDGES, F64: mp.F_EDGES}[dt]
    cols = mp.columns_of(mp.pairs(edges), [dt, dt])
    binary = _mapref.ARITH[:4] + _mapref.CMPS + ("COALESCE",) + (() if dt == F64 else ("MOD", "AND", "OR"))
    unary = ("NEG", "ABS", "IS_NULL", "IS_NOT_NULL", "TO_I64", "TO_F64") + (() if dt == F64 else ("NOT",))
    for prog in (_every(binary), _every(unary, 1)):
        kinds = [fa for fa, _, _ in _mapref.run_program(cols, prog, len(cols[0][1]))]
        check(map_plan(cols, prog, _mapref.outputs_for(kinds)), what=(dt, prog[2]), ordered=True)


def test_case_and_literals_over_the_edge_grid():
    conds = [None, 0, 1, (-5) & mp.M64, 1 << 63]
    rows = [(c, a, b) for c in conds for a in mp.I_EDGES for b in (mp.F_EDGES[0], mp.F_EDGES[5], mp.F_EDGES[-3], None)]
    cols = mp.columns_of(rows, [I64, I64, F64])
    prog = [("COL", 0), ("COL", 1), ("INT", -1), ("CASE",), O, ("COL", 0), ("COL", 2), ("F64", 0x7FF8000000000123), ("CASE",), O,
            ("COL", 0), ("NULL", F64), ("COL", 2), ("CASE",), O, ("NULL", I64), ("COL", 1), ("COALESCE",), O,
            ("COL", 1), ("INT", 2**63 - 1), ("ADD",), O, ("COL", 2), ("F64", -0.0), ("MUL",), O]
    check(map_plan(cols, prog, [("EXPR", 0, I64), ("EXPR", 1, F64), ("EXPR", 2, F64), ("EXPR", 3, I64), ("EXPR", 4, I32), ("EXPR", 5, F64)]),
          ordered=True)


# ------------------------------------------------------------------ program shape
def _five(rng, n=3_000):
    return [km.payload(rng, I32, n, True), km.payload(rng, I64, n, False), km.payload(rng, F64, n, True),
            km.payload(rng, VC, n, False), (I32, rng.integers(0, 100, n).astype(np.int32))]


def test_programs_at_the_depth_and_the_op_limit():
    cols = _five(rng_for("limits"))
    for prog in (mp.depth_limit_program(), mp.op_limit_program()):
        kinds = [False] * sum(t == O for t in prog)
        _, ran = check(map_plan(cols, prog, _mapref.outputs_for(kinds)), what=len(prog), ordered=True)
        assert sum(fam(ran, "k_map").values()) == 1


def test_eight_expressions_share_columns_and_one_is_output_twice():
    cols = _five(rng_for("eight"))
    prog = [("COL", 0), ("COL", 4), ("ADD",), O, ("COL", 0), ("COL", 4), ("MUL",), O, ("COL", 1), ("COL", 0), ("SUB",), O,
            ("COL", 2), ("COL", 2), ("MUL",), O, ("COL", 2), ("TO_I64",), O, ("COL", 0), ("IS_NULL",), O,
            ("COL", 1), ("COL", 4), ("MOD",), O, ("COL", 2), ("COL", 0), ("TO_F64",), ("DIV",), O]
    outs = [("EXPR", 7, F64), ("EXPR", 0, I64), ("EXPR", 0, I32), ("EXPR", 0, I64), ("EXPR", 1, I64), ("EXPR", 2, I64), ("EXPR", 3, F64),
            ("EXPR", 4, I64), ("EXPR", 5, I32), ("EXPR", 6, I64), ("EXPR", 3, F64)]
    _, ran = check(map_plan(cols, prog, outs), ordered=True)
    assert sum(fam(ran, "k_map").values()) == 1


@pytest.mark.parametrize("enc,env", [("host", None), ("device", VDEV)])
def test_passthrough_only_launches_nothing_and_varchar_passes_through(enc, env):
    cols = _five(rng_for("pass", enc))
    _, ran = check(map_plan(cols, [], [("COL", 3, VC), ("COL", 0, I32), ("COL", 2, F64), ("COL", 3, VC), ("COL", 1, I64)]), env, ordered=True)
    assert not fam(ran, "k_map") and bool(fam(ran, "k_vc_encode")) == (env is not None)
    # ... and next to computed columns, nullable ones included
    _, ran = check(map_plan(cols, [("COL", 0), ("INT", 1), ("ADD",), O], [("COL", 3, VC), ("EXPR", 0, I64), ("COL", 0, I32), ("COL", 2, F64)]),
                   env, ordered=True)
    assert sum(fam(ran, "k_map").values()) == 1


def test_columns_proven_non_null_come_without_a_validity_array():
    """COALESCE with a literal, IS_NULL and arithmetic over a column without NULLs: encoded by the writer of
    dense columns (k_gather + k_finish_pages), a nullable expression by k_encode_nullable"""
    cols = _five(rng_for("proof"))
    _, ran = check(map_plan(cols, [("COL", 0), ("INT", 0), ("COALESCE",), O, ("COL", 2), ("IS_NULL",), O, ("COL", 1), ("COL", 4), ("MUL",), O],
                            [("EXPR", 0, I64), ("EXPR", 1, I64), ("EXPR", 2, I64)]), ordered=True)
    assert not fam(ran, "k_encode_nullable") and fam(ran, "k_finish_pages")
    _, ran = check(map_plan(cols, [("COL", 1), ("COL", 4), ("DIV",), O], [("EXPR", 0, I64)]), ordered=True)
    assert fam(ran, "k_encode_nullable")


# ------------------------------------------------------------------ nesting
def _pb(rng, n=6_000):
    k = km.key_values(I32, rng.integers(0, 900, n))
    p = [(I32, k, rng.random(n) >= 0.05), km.payload(rng, I64, n, True)]
    b = [(I32, km.key_values(I32, rng.integers(400, 1_400, n // 2)), rng.random(n // 2) >= 0.05), (I32, rng.integers(-50, 50, n // 2).astype(np.int32))]
    return p, b


def _two_scans(pcols, bcols):
    p = pl.Plan()
    sa = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(pcols)])
    sb = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(bcols)])
    p.new_input(pl.make_table(pcols))
    p.new_input(pl.make_table(bcols))
    return p, sa, sb


ALL4 = [(0, I32), (1, I64), (2, I32), (3, I32)]


@pytest.mark.parametrize("kind", ["join", "semi", "anti", "outer", "full"])
def test_map_over_every_join_kind(kind):
    pcols, bcols = _pb(rng_for("over", kind))
    p, sa, sb = _two_scans(pcols, bcols)
    mk = {"join": p.new_join_node, "semi": p.new_semi_join_node, "anti": p.new_anti_join_node, "outer": p.new_outer_join_node,
          "full": p.new_full_outer_join_node}[kind]
    outs = ALL4[:2] if kind in ("semi", "anti") else ALL4
    j = mk(False, sa, sb, 0, 0, outs)
    if len(outs) == 4:  # COALESCE over the padding of the optional side, CASE WHEN x IS NULL
        prog = [("COL", 3), ("INT", -999), ("COALESCE",), O, ("COL", 1), ("IS_NULL",), ("INT", 0), ("COL", 1), ("CASE",), ("COL", 0), ("ADD",), O]
    else:
        prog = [("COL", 0), ("INT", 7), ("MUL",), O, ("COL", 1), ("ABS",), O]
    p.root = p.new_map_node(j, prog, [("EXPR", 0, I64), ("COL", 0, I32), ("EXPR", 1, I64)])
    got, ran = check(p, what=kind)
    assert got.num_rows > 0 and sum(fam(ran, "k_map").values()) == 1


def _scan_plan(cols):
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    p.new_input(pl.make_table(cols))
    return p, sc


def _kcols(rng, n=5_000):
    """a small-domain key, a unique key, an INT64 and an FP64 payload with NULLs"""
    return [(I32, rng.integers(0, 40, n).astype(np.int32)), (I32, rng.permutation(n).astype(np.int32)),
            (I64, rng.integers(-1000, 1000, n), rng.random(n) >= 0.1), (F64, rng.standard_normal(n), rng.random(n) >= 0.1)]


@pytest.mark.parametrize("kind", ["agg", "select", "sort", "group", "window", "map"])
def test_map_over_every_one_child_kind(kind):
    p, sc = _scan_plan(_kcols(rng_for("below", kind)))
    if kind == "agg":
        c, types = p.new_agg_node(sc, 0, [(KEY, 0, I32), (STAR, 0, I64), (SUM, 2, I64)]), [I32, I64, I64]
    elif kind == "select":
        c, types = p.new_select_node(sc, [("LT", 0, 20)], [(0, I32), (1, I32), (2, I64)]), [I32, I32, I64]
    elif kind == "sort":
        c, types = p.new_sort_node(sc, [(1, pl.SORT_DESC)], [(0, I32), (1, I32), (2, I64)], limit=777, offset=5), [I32, I32, I64]
    elif kind == "group":
        c, types = p.new_group_node(sc, [(0, 0)], [(KEY, 0, I32), (STAR, 0, I64), (pl.AGG_MIN, 2, I64)]), [I32, I64, I64]
    elif kind == "window":
        c = p.new_window_node(sc, [(0, 0)], [(1, 0)], [(pl.WIN_COL, 0, I32), (pl.WIN_ROW_NUMBER, 0, I64), (pl.WIN_SUM, 2, I64)])
        types = [I32, I64, I64]
    else:
        c, types = p.new_map_node(sc, [("COL", 2), ("INT", 2), ("MUL",), O], [("COL", 0, I32), ("COL", 1, I32), ("EXPR", 0, I64)]), [I32, I32, I64]
    # rn <= k where k is itself an expression, and arithmetic over a nullable aggregate
    prog = [("COL", 1), ("COL", 0), ("INT", 3), ("ADD",), ("LEQ",), O, ("COL", 2), ("COL", 1), ("TO_I64",), ("SUB",), O]
    p.root = p.new_map_node(c, prog, [("COL", 0, types[0]), ("EXPR", 0, I64), ("EXPR", 1, I64)])
    got, ran = check(p, what=kind)
    assert got.num_rows > 0 and sum(fam(ran, "k_map").values()) == (2 if kind == "map" else 1)


@pytest.mark.parametrize("kind", ["group", "agg", "sort", "select", "window", "join"])
def test_every_kind_over_a_map(kind):
    """SUM(a * b) by GROUP and by AGG, a computed sort key, a selection on a computed column, a window over
    one, a computed column as a join key"""
    cols = _kcols(rng_for("above", kind))
    p, sc = _scan_plan(cols)
    prog = [("COL", 2), ("COL", 1), ("MUL",), O, ("COL", 1), ("INT", 1000), ("MOD",), ("COL", 0), ("SUB",), O]
    m = p.new_map_node(sc, prog, [("COL", 0, I32), ("EXPR", 0, I64), ("EXPR", 1, I32), ("COL", 1, I32)])
    if kind == "group":
        p.root = p.new_group_node(m, [(0, 0)], [(KEY, 0, I32), (SUM, 1, I64), (pl.AGG_MAX, 2, I32)])
    elif kind == "agg":
        p.root = p.new_agg_node(m, 0, [(KEY, 0, I32), (SUM, 1, I64), (STAR, 0, I64)])
    elif kind == "sort":
        p.root = p.new_sort_node(m, [(1, pl.SORT_DESC), (3, 0)], [(1, I64), (3, I32)], limit=500)
    elif kind == "select":
        p.root = p.new_select_node(m, [("GT", 1, 0), ("LT", 2, 100), ("AND",)], [(0, I32), (1, I64), (2, I32)])
    elif kind == "window":
        p.root = p.new_window_node(m, [(0, 0)], [(2, 0), (3, 0)], [(pl.WIN_COL, 0, I32), (pl.WIN_COL, 2, I32), (pl.WIN_SUM, 1, I64), (pl.WIN_RANK, 0, I64)])
    else:
        sb = p.new_scan_node(1, [(0, I32), (1, I32)])
        p.new_input(pl.make_table([(I32, np.arange(-40, 400, dtype=np.int32)), (I32, np.arange(440, dtype=np.int32))]))
        p.root = p.new_join_node(False, m, sb, 2, 0, [(0, I32), (2, I32), (3, I32), (5, I32)])
    got, ran = check(p, what=kind, ordered=kind in ("sort", "group", "window"))
    assert got.num_rows > 0 and sum(fam(ran, "k_map").values()) == 1


# ------------------------------------------------------------------ order at the root, row-exact
NEG1 = [("COL", 1), ("NEG",), O]


def _order_plan(child, outs=None, cols=None):
    """a plan whose root is MAP(-c1, c0, c1) over `child` built on a scan of unique keys"""
    cols = cols or _kcols(rng_for("order"), 3 * MAP_TILE + 9)
    p, sc = _scan_plan(cols)
    c = child(p, sc)
    p.root = p.new_map_node(c, NEG1, outs or [("EXPR", 0, I64), ("COL", 0, I32), ("COL", 1, I32)])
    return p


def test_order_map_over_scan():
    check(_order_plan(lambda p, sc: sc), ordered=True)


def test_order_map_over_sort_without_a_limit():
    """the shortcut that must not be taken: a sort below the root's MAP still sorts"""
    got, ran = check(_order_plan(lambda p, sc: p.new_sort_node(sc, [(1, pl.SORT_DESC)], [(0, I32), (1, I32)])), ordered=True)
    assert fam(ran, "k_sort_scatter") and pl.decode_table(got)[2][0].tolist() == list(range(3 * MAP_TILE + 8, -1, -1))


def test_order_map_over_sort_with_limit_and_offset_computes_the_slice_only():
    p = _order_plan(lambda p, sc: p.new_sort_node(sc, [(1, 0)], [(0, I32), (1, I32)], limit=100, offset=50))
    got, _ = check(p, {"RJ_TUNE_MAP_GRID": "1"}, ordered=True)
    assert pl.decode_table(got)[2][0].tolist() == list(range(50, 150))


def test_order_map_over_group_and_over_window():
    grp = lambda p, sc: p.new_group_node(sc, [(0, pl.SORT_DESC)], [(KEY, 0, I32), (STAR, 0, I64)])
    got, _ = check(_order_plan(grp, [("EXPR", 0, I64), ("COL", 0, I32), ("COL", 1, I64)]), ordered=True)
    assert pl.decode_table(got)[1][0].tolist() == list(range(39, -1, -1))
    win = lambda p, sc: p.new_window_node(sc, [(0, 0)], [(1, pl.SORT_DESC)], [(pl.WIN_COL, 0, I32), (pl.WIN_ROW_NUMBER, 0, I64), (pl.WIN_COL, 1, I32)])
    got, _ = check(_order_plan(win, [("EXPR", 0, I64), ("COL", 0, I32), ("COL", 2, I32), ("COL", 1, I64)]), ordered=True)
    assert pl.decode_table(got)[1][0].tolist() == sorted(pl.decode_table(got)[1][0].tolist())


def test_order_map_over_map_over_sort():
    def child(p, sc):
        s = p.new_sort_node(sc, [(0, 0), (1, pl.SORT_DESC)], [(0, I32), (1, I32)])
        return p.new_map_node(s, [("COL", 1), ("INT", 2), ("MUL",), O], [("COL", 0, I32), ("EXPR", 0, I32)])
    got, ran = check(_order_plan(child), ordered=True)
    assert fam(ran, "k_sort_scatter") and sum(fam(ran, "k_map").values()) == 2


def test_the_same_sort_below_a_map_below_a_join_stays_a_multiset():
    cols = _kcols(rng_for("multiset"), 4_000)
    p, sc = _scan_plan(cols)
    s = p.new_sort_node(sc, [(1, pl.SORT_DESC)], [(0, I32), (1, I32)])
    m = p.new_map_node(s, NEG1, [("EXPR", 0, I64), ("COL", 1, I32)])
    sb = p.new_scan_node(0, [(1, I32)])
    p.root = p.new_join_node(True, m, sb, 1, 0, [(0, I64), (2, I32)])
    got, ran = check(p)
    assert got.num_rows == 4_000 and not fam(ran, "k_sort_scatter")  # (below a join the sort passes its child through)


# ------------------------------------------------------------------ fuzz
def fuzz_case(seed):
    rng = rng_for("fuzz", seed)
    n = int(rng.choice([1, 70, 300, 1_500, MAP_TILE + int(rng.integers(-2, 3)), 2 * MAP_TILE + 77]))
    types = [I32, I64, F64] + [int(rng.choice([I32, I64, F64])) for _ in range(int(rng.integers(0, 3)))]
    rows = mp.random_rows(rng, n)
    cols = mp.columns_of([tuple(r[{I32: 0, I64: 1, F64: 3}[t] + (k >= 3 and t != I32)] for k, t in enumerate(types)) for r in rows], types)
    if rng.random() < 0.3:  # a column without NULLs: paged on the device
        cols[0] = (I32, np.where(cols[0][2], cols[0][1], 0).astype(np.int32))
    cols.append((I32, rng.integers(0, 12, n).astype(np.int32)))  # a grouping / join key
    keycol = len(cols) - 1
    prog, kinds = _mapref.random_program(rng, cols[:-1])
    outs = [("COL", keycol, I32)] + _mapref.outputs_for(kinds, rng)
    p, sc = _scan_plan(cols)
    shape = str(rng.choice(["root", "over-select", "under-group", "under-sort", "under-select", "over-join", "over-sort"]))
    child = sc
    if shape == "over-select":
        child = p.new_select_node(sc, [("LT", keycol, 8)], [(i, c[0]) for i, c in enumerate(cols)])
    elif shape == "over-join":
        sb = p.new_scan_node(1, [(0, I32)])
        p.new_input(pl.make_table([(I32, np.arange(3, 9, dtype=np.int32))]))
        child = p.new_join_node(False, sc, sb, keycol, 0, [(i, c[0]) for i, c in enumerate(cols)])
    elif shape == "over-sort":
        child = p.new_sort_node(sc, [(keycol, pl.SORT_DESC)], [(i, c[0]) for i, c in enumerate(cols)])
    m = p.new_map_node(child, prog, outs)
    p.root = m
    ints = [k for k, o in enumerate(outs) if o[2] in (I32, I64)]
    if shape == "under-group":
        p.root = p.new_group_node(m, [(0, 0)], [(KEY, 0, I32), (STAR, 0, I64)] + [(SUM, k, I64) for k in ints[1:3]])
    elif shape == "under-sort":
        p.root = p.new_sort_node(m, [(0, 0)], [(k, o[2]) for k, o in enumerate(outs)])
    elif shape == "under-select":
        p.root = p.new_select_node(m, [("IS_NOT_NULL", len(outs) - 1), ("GEQ", 0, 2), ("OR",)], [(k, o[2]) for k, o in enumerate(outs)])
    return p, shape


@pytest.mark.parametrize("block", range(15))
def test_fuzz(block):
    """10 seeded cases per block (150 in all): random tables of edge values, random well-typed programs, a
    random surrounding plan; nothing is skipped"""
    for seed in range(10 * block, 10 * block + 10):
        p, shape = fuzz_case(seed)
        check(p, what=(seed, shape), ordered=shape in ("root", "under-group"))


# ------------------------------------------------------------------ dirty memory, instantiations, launches
@pytest.mark.parametrize("env", POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env):
    for n in SIZES:
        for form in ("paged", "nulls"):
            grid_case(n, form, env)
    s = context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


def test_every_map_instantiation_is_driven_and_a_node_launches_once():
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.split("<")[0].startswith("k_map")}
    assert compiled == {"k_map"}, sorted(compiled)
    reached = set()
    for form in ("paged", "nulls"):
        cols = grid_table(MAP_TILE + 1, form, rng_for("matrix", form))
        _, ran = check(map_plan(cols, GRID_PROG, GRID_OUTS), ordered=True)
        assert sum(fam(ran, "k_map").values()) == 1
        reached |= {n for n in ran if n.split("<")[0].startswith("k_map")}
    assert reached == compiled, (sorted(reached), sorted(compiled))


def test_same_plan_twice_on_one_context_and_resident_tables():
    cols = grid_table(20_000, "nulls", rng_for("twice"))
    p = map_plan(cols, GRID_PROG, GRID_OUTS)
    a, _ = run(p)
    b, _ = run(p)
    assert _canon(pl.table_rows(a)) == _canon(pl.table_rows(b))
    want = _mapref.execute(p)
    ctx = context()
    t = ctx.upload(p.inputs[0])
    try:
        for keep in (True, False):
            r = ctx.execute_resident(p, [t], keep_on_device=keep)
            try:
                same(r.to_table(), want, keep, ordered=True)
            finally:
                r.free()
    finally:
        t.release()


# ------------------------------------------------------------------ empty child, the error contract
def test_empty_child_gives_typed_columns_without_pages():
    none = [(I32, np.zeros(0, np.int32)), (I64, np.zeros(0, np.int64)), (VC, [])]
    got, ran = check(map_plan(none, [("COL", 0), ("COL", 1), ("ADD",), O], [("EXPR", 0, I64), ("COL", 2, VC), ("EXPR", 0, I32)]))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [I64, VC, I32] and all(c.pages.shape[0] == 0 for c in got.columns)
    assert not fam(ran, "k_map")


def _error(p, ctx=None):
    with pytest.raises(capi.RjError) as e:
        capi.execute(p, ctx or context())
    return e.value.code, str(e.value)


def test_error_contract(monkeypatch):
    cols = _five(rng_for("err"), 300)  # I32, I64, F64, VARCHAR, I32
    ok = [("COL", 0), ("COL", 4), ("ADD",), O, ("COL", 2), O]
    bad = lambda prog, outs: _error(map_plan(cols, prog, outs))
    monkeypatch.setitem(capi.X_OPS, "BOGUS", 99)
    for prog, outs, text in ((ok, [("EXPR", 0, I64), ("EXPR", 2, F64), ("EXPR", 1, F64)], "names expression 2"),
                             (ok, [("EXPR", 0, I64)], "no output names expression 1"),
                             (ok, [("EXPR", 0, F64), ("EXPR", 1, F64)], "declared type"), (ok, [("EXPR", 0, I64), ("EXPR", 1, I64)], "declared type"),
                             (ok, [("EXPR", 0, VC), ("EXPR", 1, F64)], "declared type"), (ok, [("EXPR", 0, I64), ("EXPR", 1, I32)], "declared type"),
                             (ok, [("EXPR", 0, I64), ("EXPR", 1, F64), ("COL", 1, I32)], "declared type"),
                             (ok, [("EXPR", 0, I64), ("EXPR", 1, F64), ("COL", 5, I32)], "out of range"),
                             (ok, [("EXPR", 0, I64), ("EXPR", 1, F64), (2, 0, I32)], "output code"),
                             ([("BOGUS",), O], [("EXPR", 0, I64)], "opcode"), ([("COL", 9), O], [("EXPR", 0, I64)], "out of range"),
                             ([("COL", 0), ("COL", 2), ("MUL",), O], [("EXPR", 0, I64)], "different types"),
                             ([("COL", 2), ("NOT",), O], [("EXPR", 0, I64)], "integer"), ([("COL", 2), ("COL", 2), ("MOD",), O], [("EXPR", 0, F64)], "MOD"),
                             ([("NULL", I32), O], [("EXPR", 0, I64)], "RJ_X_NULL"), ([("ADD",), O], [("EXPR", 0, I64)], "underflow"),
                             ([("COL", 0), ("COL", 0), O], [("EXPR", 0, I64)], "left on the stack"), ([("COL", 0)], [], "does not end")):
        code, msg = bad(prog, outs)
        assert code == ARG and text in msg, (prog, outs, msg)
    for prog, text in (([("COL", 3), O], "VARCHAR"), ([("COL", 1)] + [("NEG",)] * 127 + [O], "128"), ([("COL", 1)] * 9 + [("ADD",)] * 8 + [O], "deeper")):
        code, msg = bad(prog, [("EXPR", 0, I64)])
        assert code == UNSUPPORTED and text in msg, (prog, msg)
    # ... all of it before the child's rows are looked at: an empty child hides nothing
    empty = [(I32, np.zeros(0, np.int32)), (VC, [])]
    assert _error(map_plan(empty, [("COL", 1), O], [("EXPR", 0, I64)]))[0] == UNSUPPORTED
    assert _error(map_plan(empty, [("ADD",), O], [("EXPR", 0, I64)]))[0] == ARG
    assert _error(map_plan(empty, [("COL", 0), O], []))[0] == ARG


def test_ops_without_a_program_pointer_are_an_argument_error():
    p = map_plan(_five(rng_for("null"), 50), [("COL", 0), O], [("EXPR", 0, I64)])
    cplan, keep = pl.plan_to_c(p)
    cplan.nodes[p.root].right_attr = 0
    c = context()
    out = C.c_void_p()
    rc = c.L.rj_execute(c.h, C.byref(cplan), C.byref(out))
    assert rc == ARG and b"NULL program pointer" in c.L.rj_last_error(c.h)
    del keep


def test_execute_sharded_refuses_and_a_two_device_context_runs_on_one():
    cols = grid_table(5_000, "nulls", rng_for("two"))
    p = map_plan(cols, GRID_PROG, GRID_OUTS)
    ok, why = capi.plan_shardable(p)
    assert not ok and "RJ_NODE_MAP" in why
    got, _ = check(p, devices=[0, 0], ordered=True)
    assert got.num_rows == 5_000
    ctx = context(devices=[0, 0])
    tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
    try:
        with pytest.raises(capi.RjError) as e:
            ctx.execute_sharded(p, tables)
        assert e.value.code == UNSUPPORTED and "RJ_NODE_MAP" in str(e.value)
    finally:
        for row in tables:
            for t in row:
                t.release()
