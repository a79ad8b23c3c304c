"""Selection nodes (RJ_NODE_SELECT) on the device, through the C-ABI, against the numpy reference
tests/_selectref.py (tests/test_select_plan.py ties it to a row-at-a-time evaluator and to the pinned C
oracle on the CPU).  Results up to 50 000 rows are compared row by row (pl.canonical_rows), and every
result column is read by the strict page reader tests/_pagecheck.py first.

Device path: k_select compacts the row ids of the rows that pass (tiles of SEL_TILE rows, read from
csrc/rj_device.hpp), k_gather materialises every distinct output column through them — at the root into
Page images (k_finish_pages), nullable ones through k_encode_nullable, VARCHAR ones through the host or
device encoder.  test_every_select_instantiation_is_driven checks the launch log against the compiled
kernel handles (tests/_elfsyms.py).

A program of at most 64 ops never stacks deeper than 32 (L leaves need L - 1 binary ops), so the depth
limit of 60 that rj.h states cannot be reached: the deepest program here is _selectref.deepest_program."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import _aggref
import _elfsyms
import _filterref
import _pagecheck as pc
import _plangen
import _selectref
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
import test_select_plan as sp
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
KEY, STAR, SUM = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_SUM
_HPP = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
SEL_TILE = int(re.search(r"constexpr int SEL_TILE\s*=\s*(\d+);", _HPP).group(1))
ROWS32, ROWS64 = (int(re.search(rf"constexpr uint32_t {n}\s*=\s*(\d+);", _HPP).group(1)) for n in ("ROWS32", "ROWS64"))
VDEV = {"RJ_TUNE_VARCHAR_DEV": "1"}  # every VARCHAR result column is encoded on the device
POISON = [{"RJ_DEBUG_POISON": str(m)} for m in (0x15A, 0x1FF)]  # tests/test_gpu_poison.py's modes
rng_for, select_plan = sp.rng_for, sp.select_plan
fam = lambda ran, family: {n: c for n, c in ran.items() if n.split("<")[0] == family}

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


def same(got, want, what=""):
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    dec = pc.check_table(got)  # the format of every column, then the content
    assert pc.same_as(dec, pl.decode_table(got)), what
    if want.num_rows <= 50_000 or any(c.type == VC for c in want.columns):
        assert pc.canonical_rows(dec) == pl.canonical_rows(want), what
    else:
        assert pl.table_digest(got) == pl.table_digest(want), what


def check(p, env=None, what="", **kw):
    got, ran = run(p, env, **kw)
    same(got, _selectref.execute(p), what)
    return got, ran


# ------------------------------------------------------------------ sizes where the kernel switches branches
SIZES = [1, 63, 64, 65, 255, 256, 257, SEL_TILE - 1, SEL_TILE, SEL_TILE + 1, 5 * SEL_TILE + 17,
         ROWS64 - 1, ROWS64, ROWS64 + 1, ROWS32 - 1, ROWS32, ROWS32 + 1]
WHICH = ["none", "all", "half", "first", "last", "tile"]


def grid_table(n, form, rng):
    """position, a permutation of the positions, an INT64 payload; form "nulls": every column with
    NULLs (dense values + validity on the device), the first and the last position kept"""
    cols = [(I32, np.arange(n, dtype=np.int32)), (I32, rng.permutation(n).astype(np.int32)),
            (I64, rng.integers(-2**62, 2**62, n))]
    if form == "nulls":
        valid = [rng.random(n) >= 0.1 for _ in cols]
        valid[0][[0, n - 1]] = True
        valid[2][n // 2] = n == 1
        cols = [(dt, v, m) for (dt, v), m in zip(cols, valid)]
    return cols


def grid_program(which, n):
    lo = 0 if n <= SEL_TILE + 1 else 17
    return {"none": [("LT", 0, 0)], "all": [("GEQ", 0, 0), ("IS_NULL", 0), ("OR",)], "half": [("LT", 1, (n + 1) // 2)],
            "first": [("EQ", 0, 0)], "last": [("EQ", 0, n - 1)],
            "tile": [("GEQ", 0, lo), ("LT", 0, lo + SEL_TILE), ("AND",)]}[which], lo


def grid_case(n, form, env=None):
    cols = grid_table(n, form, rng_for("grid", n, form))
    for which in WHICH:
        prog, lo = grid_program(which, n)
        got, ran = check(select_plan(cols, prog, outs=[2, 0]), env, what=(n, form, which))
        assert sum(fam(ran, "k_select").values()) == 1
        if form == "paged":
            assert got.num_rows == {"none": 0, "all": n, "half": (n + 1) // 2, "first": 1, "last": 1,
                                    "tile": min(n - lo, SEL_TILE)}[which]


@pytest.mark.parametrize("form", ["paged", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_size_grid(n, form):
    grid_case(n, form)


@pytest.mark.parametrize("nullable", [False, True], ids=["paged", "nullable"])
@pytest.mark.parametrize("count", [ROWS32 - 1, ROWS32, ROWS32 + 1, ROWS64 - 1, ROWS64, ROWS64 + 1])
def test_survivors_fill_result_pages_to_their_edges(count, nullable):
    n = 3 * SEL_TILE + 5
    rng = rng_for("edges", count, nullable)
    cols = grid_table(n, "paged", rng)
    if nullable:
        cols[0] = (I32, cols[0][1], rng.random(n) >= 0.2)
        cols[2] = (I64, cols[2][1], rng.random(n) >= 0.2)
    got, ran = check(select_plan(cols, [("LT", 1, count)], outs=[0, 2]), what=(count, nullable))
    assert got.num_rows == count
    if not nullable:  # full pages but the last
        assert got.columns[0].pages.shape[0] == -(-count // ROWS32) and got.columns[1].pages.shape[0] == -(-count // ROWS64)
    assert bool(fam(ran, "k_encode_nullable")) == nullable and bool(fam(ran, "k_finish_pages")) != nullable


# ------------------------------------------------------------------ every opcode on every type
CMPS = ("EQ", "NEQ", "LT", "GT", "LEQ", "GEQ")


@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_every_opcode_on_every_type(dt):
    rng = rng_for("ops", dt)
    cols = sp.special_table(rng, 500, [dt, dt, I32])
    lits = [v.item() for v in km.SPECIAL_KEYS[dt]] + ([0.5, -1.0] if dt == F64 else [1, -3])
    progs = [[(op, 0, lit)] for op in CMPS for lit in lits]
    progs += [[("COL_" + op, 0, 1)] for op in CMPS] + [[("IS_NULL", 0)], [("IS_NOT_NULL", 1)]]
    if dt == I32:  # (int32_t)ivalue: 2^32 + 1 is 1, -2^31 - 1 is 2^31 - 1, 2^35 - 4 is -4
        progs += [[("EQ", 0, 2**32 + 1)], [("LT", 0, -2**31 - 1)], [("GEQ", 0, 2**35 - 4)]]
    kept = {}
    for prog in progs:
        got, _ = check(select_plan(cols, prog), what=prog)
        kept[repr(prog[0])] = got.num_rows
    v, m = cols[0][1], cols[0][2]
    assert kept[repr(("COL_EQ", 0, 1))] > 0 and kept[repr(("IS_NULL", 0))] == int((~m).sum()) > 0
    if dt == I32:
        assert kept[repr(("EQ", 0, 2**32 + 1))] == int(((v == 1) & m).sum()) > 0
        assert kept[repr(("LT", 0, -2**31 - 1))] == int(((v < 2**31 - 1) & m).sum()) > 0
    if dt == F64:  # NaN equals nothing, and differs from everything that is not NULL
        assert kept[repr(("EQ", 0, float("nan")))] == 0 and kept[repr(("NEQ", 0, float("nan")))] == int(m.sum())


# ------------------------------------------------------------------ program structure
@functools.lru_cache(maxsize=None)
def big_table():
    return sp.special_table(rng_for("big"), 10_000)


@pytest.mark.parametrize("block", range(10))
def test_random_programs(block):
    """21 seeded programs per block (210 in all) of 1 .. 64 ops over one 10 000-row table on one context;
    every block has a 64-op program, block 0 the deepest stack 64 ops allow."""
    rng = rng_for("programs", block)
    cols = big_table()
    progs = [_selectref.random_program(rng, cols, 64 if i == 0 else int(rng.integers(1, 65))) for i in range(20)]
    progs.append(_selectref.deepest_program(rng, cols, 64 if block == 0 else 2 * int(rng.integers(1, 33))))
    if block == 0:
        assert _selectref.max_depth(progs[-1]) == 32 and len(progs[-1]) == 64
    kept = 0
    for prog in progs:
        got, _ = check(select_plan(cols, prog, outs=[0, 4, 2]), what=(block, prog))
        kept += got.num_rows
    assert kept > 0


def test_not_over_null_rows_the_one_leaf_program_and_the_empty_program():
    cols = [(I32, np.array([5, 7, 0, -1], np.int32), np.array([1, 1, 0, 1], bool)), (I64, np.array([10, 20, 30, 40]))]
    got, _ = check(select_plan(cols, [("LT", 0, 6)]))
    assert pl.sorted_rows(got) == [(-1, 40), (5, 10)]
    got, _ = check(select_plan(cols, [("LT", 0, 6), ("NOT",)]))
    assert pl.sorted_rows(got) == [(7, 20), (None, 30)]           # NOT (x < 6) holds for NULL x
    got, ran = check(select_plan(cols, []))
    assert pl.sorted_rows(got) == [(-1, 40), (5, 10), (7, 20), (None, 30)]
    assert not fam(ran, "k_select")                               # a projection launches no selection


# ------------------------------------------------------------------ projection
def _five(rng, n=3_000):
    return [km.payload(rng, I32, n, True), km.payload(rng, I64, n, False), km.payload(rng, F64, n, True),
            km.payload(rng, VC, n, False), (I32, rng.integers(0, 100, n).astype(np.int32))]


def test_projection_reorders_repeats_and_drops_columns():
    cols = _five(rng_for("proj"))
    got, ran = check(select_plan(cols, [("LT", 4, 40)], outs=[2, 0, 0, 1, 2]))  # the predicate column is not output
    assert 0 < got.num_rows < 3_000
    assert sum(fam(ran, "k_gather").values()) == 3              # a column named twice is gathered once
    check(select_plan(cols, [], outs=[1, 1, 2, 0]))             # ... and without a program
    none, _ = run(select_plan(cols, [("LT", 4, 40)], outs=[]))  # no column at all: the row count
    assert none.num_rows == got.num_rows and not none.columns


@pytest.mark.parametrize("enc,env", [("host", None), ("device", VDEV)])
def test_varchar_passes_through_to_the_root(enc, env):
    cols = _five(rng_for("vc", enc))
    for prog in ([("GEQ", 4, 50)], []):
        got, ran = check(select_plan(cols, prog, outs=[3, 0, 3]), env, what=(enc, prog))
        assert got.num_rows > 0 and bool(fam(ran, "k_vc_encode")) == (env is not None)


# ------------------------------------------------------------------ composition
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
OVER = {  # kind -> (output_attrs of the node, program over them)
    "join": (ALL4, [("GT", 3, 0), ("IS_NULL", 1), ("OR",)]),
    "semi": (ALL4[:2], [("LT", 1, 0)]),
    "anti": (ALL4[:2], [("LT", 1, 0), ("IS_NULL", 0), ("OR",)]),
    "outer": (ALL4, [("IS_NULL", 2), ("GT", 3, 25), ("OR",)]),        # the optional side's NULLs
    "full": (ALL4, [("IS_NULL", 0), ("IS_NULL", 2), ("OR",), ("COL_EQ", 0, 2), ("LT", 3, -40), ("AND",), ("OR",)]),
}


def _binary(p, kind, build_left, l, r, outs):
    mk = {"join": p.new_join_node, "semi": p.new_semi_join_node, "anti": p.new_anti_join_node,
          "outer": p.new_outer_join_node, "full": p.new_full_outer_join_node}[kind]
    return mk(build_left, l, r, 0, 0, outs)


@pytest.mark.parametrize("kind", list(OVER))
def test_select_over_every_join_kind(kind):
    pcols, bcols = _pb(rng_for("over", kind))
    p, sa, sb = _two_scans(pcols, bcols)
    outs, prog = OVER[kind]
    j = _binary(p, kind, False, sa, sb, outs)  # the right child is built: filter / optional side
    p.root = p.new_select_node(j, prog, [(i, t) for i, t in reversed(outs)])
    got, ran = check(p, what=kind)
    assert 0 < got.num_rows < _selectref.evaluate(p, j)[0] and fam(ran, "k_select")


@pytest.mark.parametrize("having", ["count", "sum-is-null"])
def test_having(having):
    rng = rng_for("having", having)
    pcols, _ = _pb(rng)
    dead = pcols[0][1] == pcols[0][1][0]
    pcols[1] = (I64, pcols[1][1], pcols[1][2] & ~dead)  # one group without any value
    p = pl.Plan()
    sc = p.new_scan_node(0, [(0, I32), (1, I64)])
    g = p.new_agg_node(sc, 0, [(KEY, 0, I32), (STAR, 0, I64), (SUM, 1, I64)])
    prog = [("GT", 1, 7)] if having == "count" else [("IS_NULL", 2)]
    p.root = p.new_select_node(g, prog, [(0, I32), (1, I64), (2, I64)])
    p.new_input(pl.make_table(pcols))
    got, _ = check(p, what=having)
    assert 0 < got.num_rows < _selectref.evaluate(p, g)[0]
    if having == "count":
        assert all(r[1] > 7 for r in pl.table_rows(got))


def test_select_over_select():
    cols = _five(rng_for("twice"))
    p = select_plan(cols, [("LT", 4, 70)], outs=[4, 0, 2])
    p.root = p.new_select_node(p.root, [("GEQ", 0, 30), ("IS_NOT_NULL", 1), ("AND",)], [(2, F64), (1, I32)])
    got, ran = check(p)
    assert got.num_rows > 0 and sum(fam(ran, "k_select").values()) == 2


@pytest.mark.parametrize("build_left", [True, False], ids=["built", "probed"])
@pytest.mark.parametrize("kind", list(OVER) + ["agg"])
def test_parents_use_a_selected_nullable_column_as_their_key(kind, build_left):
    pcols, bcols = _pb(rng_for("under", kind, build_left))
    p, sa, sb = _two_scans(pcols, bcols)
    s = p.new_select_node(sa, [("LT", 1, 0), ("IS_NULL", 1), ("OR",)], [(0, I32), (1, I64)])  # the key stays nullable
    if kind == "agg":
        p.root = p.new_agg_node(s, 0, [(KEY, 0, I32), (STAR, 0, I64), (SUM, 1, I64)])
    else:
        outs = OVER[kind][0]
        if kind in ("semi", "anti") and build_left:   # the selection is the filter side: B's columns come out
            outs = [(2, I32), (3, I32)]
        if kind == "outer" and build_left:
            outs = [(2, I32), (3, I32), (0, I32), (1, I64)]
        p.root = _binary(p, kind, build_left, s, sb, outs)
    got, ran = check(p, what=(kind, build_left))
    assert got.num_rows > 0 and fam(ran, "k_select")


def test_outer_join_where_optional_key_is_null_is_the_anti_join_on_the_device():
    pcols, bcols = _pb(rng_for("identity"))
    p, sa, sb = _two_scans(pcols, bcols)
    o = p.new_outer_join_node(False, sa, sb, 0, 0, [(0, I32), (1, I64), (2, I32)])
    p.root = p.new_select_node(o, [("IS_NULL", 2)], [(0, I32), (1, I64)])
    got, _ = check(p)
    a, sa, sb = _two_scans(pcols, bcols)
    a.root = a.new_anti_join_node(False, sa, sb, 0, 0, [(0, I32), (1, I64)])
    anti, _ = run(a)
    assert 0 < got.num_rows == anti.num_rows and pl.canonical_rows(got) == pl.canonical_rows(anti)


# ---- the mixed-plan fuzz of tests/_plangen.py, with selections
def _copy(plan):
    q = pl.Plan()
    q.nodes, q.inputs, q.root = list(plan.nodes), list(plan.inputs), plan.root
    return q


def _program_over(rng, cols):
    if not any(c[0] in _selectref.NP_OF for c in cols):
        return []
    return _selectref.random_program(rng, cols, int(rng.integers(1, 12)))


@pytest.mark.parametrize("seed", range(40))
def test_mixed_plan_with_a_selection_over_the_root(seed):
    p, _ = fm.case(seed)
    rng = rng_for("root", seed)
    q = _copy(p)
    _, cols = _aggref.evaluate(p)
    q.root = q.new_select_node(p.root, _program_over(rng, cols), [(i, c[0]) for i, c in enumerate(cols)])
    check(q, what=seed)


def _python_rows(cols):
    n = cols[0][1].shape[0] if cols else 0
    cell = lambda v: v if isinstance(v, (bytes, type(None))) else v.item()
    return [tuple(cell(c[1][r]) if c[2][r] else None for c in cols) for r in range(n)]


@pytest.mark.parametrize("seed", range(40))
def test_mixed_plan_with_a_selection_over_every_scan(seed):
    """Expected: the same plan over base tables filtered on the host by the row-at-a-time evaluator
    (tests/test_select_plan.py), through _aggref — _selectref takes no part."""
    p, _ = fm.case(seed)
    rng = rng_for("scans", seed)
    dev, host = _copy(p), _copy(p)
    for i in _plangen.reachable(p):
        node = p.nodes[i]
        if _plangen.kind_of(node) != "scan":
            continue
        cols = _filterref._scan(p, node)
        types = [c[0] for c in cols]
        prog = _program_over(rng, cols)
        # device: the scan moves to the end of the node list, a selection over it takes its place
        dev.nodes.append(node)
        dev.nodes[i] = pl.PlanNode(pl.SelectNode(len(dev.nodes) - 1, prog), [(k, t) for k, t in enumerate(types)])
        # host: a filtered copy of the base table as an input of its own
        t = p.inputs[node.data.base_table_id]
        keep = np.array([sp.eval_row(prog, r, types) for r in _python_rows(cols)], dtype=bool) if cols else np.ones(t.num_rows, bool)
        fcols = []
        for c, d in zip(t.columns, pl.decode_table(t)):
            if c.type == VC:
                fcols.append((VC, [s for s, k in zip(d, keep) if k]))
            else:
                fcols.append((c.type, np.asarray(d[0])[keep], np.asarray(d[1], dtype=bool)[keep]))
        ft = pl.make_table(fcols) if keep.any() else pl.ColumnarTable(0, [pl.Column(c.type) for c in t.columns])
        host.nodes[i] = pl.PlanNode(pl.ScanNode(len(host.inputs)), list(node.output_attrs))
        host.new_input(ft)
    got, _ = run(dev)
    same(got, _aggref.execute(host), seed)


# ------------------------------------------------------------------ empty child and empty result
def _typed_and_empty(t, types):
    assert t.num_rows == 0 and [c.type for c in t.columns] == types and all(c.pages.shape[0] == 0 for c in t.columns)


def test_empty_child_and_empty_result():
    none = [(I32, np.zeros(0, np.int32)), (I64, np.zeros(0, np.int64)), (VC, [])]
    some = [(I32, np.arange(500, dtype=np.int32)), (I64, np.arange(500)), km.payload(rng_for("e"), VC, 500, False)]
    for cols, prog in ((none, [("LT", 0, 5)]), (none, []), (some, [("LT", 0, 0)])):
        got, _ = check(select_plan(cols, prog, outs=[1, 2, 0]), what=(len(cols[2][1]), prog))
        _typed_and_empty(got, [I64, VC, I32])
    # below a join: nothing to build, nothing to probe, and an outer join that pads every preserved row
    for kind, build_left, rows in (("join", True, 0), ("join", False, 0), ("outer", True, 500), ("anti", True, 500)):
        p, sa, sb = _two_scans(some[:2], some[:2])
        s = p.new_select_node(sa, [("LT", 0, 0)], [(0, I32), (1, I64)])
        outs = [(2, I32), (3, I64)] if kind == "anti" else [(0, I32), (1, I64), (2, I32)]
        p.root = _binary(p, kind, build_left, s, sb, outs)
        got, _ = check(p, what=(kind, build_left))
        assert got.num_rows == rows
        if not rows:
            _typed_and_empty(got, [t for _, t in outs])


# ------------------------------------------------------------------ the error contract
def _error(p, ctx=None):
    with pytest.raises(capi.RjError) as e:
        capi.execute(p, ctx or context())
    return e.value.code, str(e.value)


ARG, UNSUPPORTED = 1, 5


def test_error_contract(monkeypatch):
    cols = _five(rng_for("err"), 300)  # I32, I64, F64, VARCHAR, I32
    bad = lambda prog, outs=None: _error(select_plan(cols, prog, outs))
    # ---- RJ_ERR_UNSUPPORTED: VARCHAR leaves, more than 64 ops
    for prog in ([("EQ", 3, b"v1")], [("IS_NULL", 3)], [("LIKE", 3, b"v%")], [("COL_EQ", 3, 3)], [("COL_LT", 0, 3)]):
        code, msg = bad(prog)
        assert code == UNSUPPORTED and "VARCHAR" in msg, (prog, msg)
    code, msg = bad([("IS_NULL", 0)] + [("NOT",)] * 64)
    assert code == UNSUPPORTED and "64" in msg
    check(select_plan(cols, [("IS_NULL", 0)] + [("NOT",)] * 63))  # (64 ops are fine)
    # ---- RJ_ERR_ARG
    monkeypatch.setitem(capi.F_OPS, "BOGUS", 20)
    monkeypatch.setitem(capi.F_OPS, "BOGUS2", -1)
    for prog, text in (([("BITMAP", np.zeros(64, np.uint8))], "RJ_F_HOST_BITMAP"),
                       ([("LT", 5, 1)], "out of range"), ([("LT", -1, 1)], "out of range"), ([("IS_NULL", 99)], "out of range"),
                       ([("COL_EQ", 0, 5)], "out of range"), ([("COL_EQ", 0, -1)], "out of range"),
                       ([("COL_EQ", 0, 1)], "different types"), ([("COL_GEQ", 1, 2)], "different types"),
                       ([("LIKE", 0, b"a%")], "LIKE"),
                       ([("AND",)], "malformed"), ([("NOT",)], "malformed"), ([("LT", 0, 1), ("LT", 0, 2)], "malformed"),
                       ([("LT", 0, 1), ("AND",)], "malformed"), ([("LT", 0, 1), ("LT", 0, 2), ("OR",), ("OR",)], "malformed"),
                       ([("BOGUS", 0, 0)], "opcode"), ([("BOGUS2", 0, 0)], "opcode")):
        code, msg = bad(prog)
        assert code == ARG and text in msg, (prog, msg)
    p = select_plan(cols, [("LT", 0, 1)])
    p.nodes[p.root].output_attrs[1] = (1, I32)  # the child column is INT64
    code, msg = _error(p)
    assert code == ARG and "declared type" in msg
    p = select_plan(cols, [("LT", 0, 1)])
    p.nodes[p.root].output_attrs[0] = (7, I32)
    code, msg = _error(p)
    assert code == ARG and "output attr out of range" in msg
    # ... all of it before the child's rows are looked at: an empty child hides nothing
    empty = [(I32, np.zeros(0, np.int32)), (VC, [])]
    assert _error(select_plan(empty, [("IS_NULL", 1)]))[0] == UNSUPPORTED
    assert _error(select_plan(empty, [("AND",)]))[0] == ARG


def test_ops_without_a_program_pointer_are_an_argument_error():
    p = select_plan(_five(rng_for("null"), 50), [("LT", 0, 1)])
    cplan, keep = pl.plan_to_c(p)
    cplan.nodes[p.root].right_attr = 0
    c = context()
    out = C.c_void_p()
    rc = c.L.rj_execute(c.h, C.byref(cplan), C.byref(out))
    assert rc == ARG and b"NULL program pointer" in c.L.rj_last_error(c.h)
    del keep


def test_execute_sharded_refuses_and_a_two_device_context_runs_on_one():
    cols = grid_table(5_000, "nulls", rng_for("two"))
    p = select_plan(cols, [("LT", 1, 2_000)])
    got, _ = check(p, devices=[0, 0])
    assert got.num_rows > 0
    ctx = context(devices=[0, 0])
    tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
    try:
        with pytest.raises(capi.RjError) as e:
            ctx.execute_sharded(p, tables)
        assert e.value.code == UNSUPPORTED and "RJ_NODE_SELECT" in str(e.value)
    finally:
        for row in tables:
            for t in row:
                t.release()


def test_resident_tables_and_results_kept_on_the_device():
    cols = grid_table(50_000, "nulls", rng_for("resident"))
    p = select_plan(cols, [("LT", 1, 20_000), ("IS_NULL", 2), ("OR",)])
    want = _selectref.execute(p)
    ctx = context()
    t = ctx.upload(p.inputs[0])
    try:
        for keep in (True, False):
            r = ctx.execute_resident(p, [t], keep_on_device=keep)
            try:
                if keep:
                    assert all(r.device_pages(c) for c in range(r.num_cols))
                same(r.to_table(), want, keep)
            finally:
                r.free()
    finally:
        t.release()


# ------------------------------------------------------------------ dirty memory, the same plan twice
@pytest.mark.parametrize("env", POISON, ids=["0x15a", "0x1ff"])
def test_on_poisoned_block_cache(env):
    for n in (SEL_TILE - 1, SEL_TILE + 1):
        for form in ("paged", "nulls"):
            grid_case(n, form, env)
    pcols, bcols = _pb(rng_for("poison"))
    p, sa, sb = _two_scans(pcols, bcols)
    outs, prog = OVER["outer"]
    p.root = p.new_select_node(_binary(p, "outer", False, sa, sb, outs), prog, outs)
    check(p, env)
    s = context(env).pool()
    assert s["fills"] > 0 and s["filled_bytes"] > 0, s


def test_same_plan_twice_on_one_context():
    p = select_plan(big_table(), [("LT", 0, 1), ("COL_NEQ", 1, 4), ("OR",)], outs=[0, 1, 2])
    a, _ = run(p)
    b, _ = run(p)
    assert a.num_rows == b.num_rows > 0 and pl.canonical_rows(a) == pl.canonical_rows(b)


# ------------------------------------------------------------------ every compiled instantiation
def test_every_select_instantiation_is_driven():
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.split("<")[0].startswith("k_select")}
    assert compiled == {"k_select"}, sorted(compiled)
    reached = set()
    for form in ("paged", "nulls"):
        cols = grid_table(SEL_TILE + 1, form, rng_for("matrix", form))
        _, ran = check(select_plan(cols, [("LT", 1, 100), ("COL_GT", 0, 1), ("OR",)]))
        reached |= {n for n in ran if n.split("<")[0].startswith("k_select")}
    assert reached == compiled, (sorted(reached), sorted(compiled))
