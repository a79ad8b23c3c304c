"""Selection nodes (RJ_NODE_SELECT) without a GPU: marshalling, the header, the sharding refusal, and
the numpy reference tests/_selectref.py pinned three ways — against a row-at-a-time evaluator
(_csvgen.eval_filter, extended here for the column comparisons and the INT32 literal rule) on random
programs over tables with NULLs and the special values of every type, against the pinned C oracle's
Table::from_csv for literal-only programs, and through the oracle's inner join by two identities."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import _csvgen
import _filterref
import _oracle
import _selectref
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
TYPES = [I32, I64, F64, I32, I64, F64]


def rng_for(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def special_table(rng, n, types=TYPES, null_p=0.12):
    """Columns of `types` with NULLs; small domains so that comparisons and column pairs hit, and the
    special values of km.SPECIAL_KEYS (NaN, +-inf, -0.0, subnormals, the integer extremes) in each."""
    cols = []
    for dt in types:
        if dt == F64:
            v = rng.integers(-4, 5, n).astype(np.float64) * 0.5
        else:
            v = rng.integers(-4, 5, n).astype(km.NP_OF[dt])
        sp = km.SPECIAL_KEYS[dt]
        at = rng.choice(n, min(n, 2 * sp.shape[0]), replace=False)
        v[at] = np.resize(sp, at.shape[0])
        cols.append((dt, v, rng.random(n) >= null_p))
    return cols


def select_plan(cols, program, outs=None):
    """Scan(cols) -> SELECT program; outs: child columns in output order (default: all)."""
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    outs = range(len(cols)) if outs is None else outs
    p.root = p.new_select_node(sc, program, [(i, cols[i][0]) for i in outs])
    p.new_input(pl.make_table(cols))
    return p


def rows_of(cols):
    n = cols[0][1].shape[0]
    return [tuple(c[1][r].item() if c[2][r] else None for c in cols) for r in range(n)]


def eval_row(program, row, types):
    """_csvgen.eval_filter with the two rules it does not know: a column comparison becomes a literal
    comparison of this row (false if the right side is NULL), an INT32 literal is cut to 32 bits."""
    local = []
    for term in program:
        if term[0].startswith("COL_"):
            y = row[term[2]]
            local.append((term[0][4:], term[1], y) if y is not None else ("IS_NULL", term[1]))
            if y is None:  # false whatever the left side is: x IS NULL AND x IS NOT NULL
                local += [("IS_NOT_NULL", term[1]), ("AND",)]
        elif term[0] in _selectref.CMP and types[term[1]] == I32:
            local.append((term[0], term[1], (int(term[2]) + 2**31) % 2**32 - 2**31))
        else:
            local.append(term)
    return _csvgen.eval_filter(local, row, 0)


# ------------------------------------------------------------------ interface
def test_marshalling_carries_the_program_in_right_and_right_attr():
    cols = special_table(rng_for("m"), 20)
    prog = [("LT", 0, 3), ("COL_GEQ", 1, 4), ("AND",), ("IS_NULL", 2), ("NOT",), ("OR",)]
    p = select_plan(cols, prog, outs=[2, 0, 0])
    cp, keep = pl.plan_to_c(p)
    nd = cp.nodes[p.root]
    assert nd.kind == pl.NODE_SELECT == 7 and nd.left == 0 and nd.n_out == 3
    assert nd.right == len(prog) and nd.right_attr != 0
    ops = C.cast(C.c_void_p(nd.right_attr), C.POINTER(capi.rj_filter_op))
    assert [ops[k].op for k in range(len(prog))] == [2, 19, 9, 6, 11, 10]
    assert (ops[1].column, ops[1].ivalue) == (1, 4) and (ops[0].column, ops[0].ivalue) == (0, 3)
    assert [nd.out_idx[k] for k in range(3)] == [2, 0, 0] and [nd.out_type[k] for k in range(3)] == [F64, I32, I32]
    # the empty program: a projection, no pointer needed
    cp2, keep2 = pl.plan_to_c(select_plan(cols, []))
    assert cp2.nodes[1].kind == 7 and cp2.nodes[1].right == 0 and cp2.nodes[1].right_attr == 0
    assert [capi.F_OPS["COL_" + o] for o in ("EQ", "NEQ", "LT", "GT", "LEQ", "GEQ")] == list(range(14, 20))
    del keep, keep2


def test_header_declares_the_kind_the_opcodes_and_the_accessors():
    h = open(os.path.join(os.path.dirname(km.LIB), "..", "include", "rj.h")).read()
    for text in ("RJ_NODE_SELECT = 7", "RJ_F_COL_EQ = 14", "RJ_F_COL_GEQ = 19", "#define RJ_SELECT_N_OPS(node)",
                 "#define RJ_SELECT_OPS(node)"):
        assert text in h, text


def test_abi_version_is_unchanged():
    assert capi.load().rj_abi_version() == 3


def test_plan_shardable_refuses_selections():
    cols = special_table(rng_for("s"), 50, [I32, I32], null_p=0)
    ok, why = capi.plan_shardable(select_plan(cols, [("LT", 0, 2)]))
    assert not ok and "RJ_NODE_SELECT" in why
    q = pl.Plan()  # ... under a join
    a = q.new_scan_node(0, [(0, I32), (1, I32)])
    s = q.new_select_node(a, [("LT", 0, 2)], [(0, I32)])
    b = q.new_scan_node(0, [(0, I32)])
    q.root = q.new_join_node(True, s, b, 0, 0, [(0, I32)])
    q.new_input(pl.make_table(cols))
    ok, why = capi.plan_shardable(q)
    assert not ok and "RJ_NODE_SELECT" in why


def test_library_holds_the_selection_kernel():
    import _elfsyms
    assert "k_select" in {_elfsyms.short_name(n).split("<")[0] for n in _elfsyms.kernel_handles(km.LIB)}


# ------------------------------------------------------------------ the reference, pinned
@pytest.mark.parametrize("block", range(10))
def test_reference_agrees_with_a_row_at_a_time_evaluator(block):
    """25 random programs per block (250 in all), 1 .. 64 ops, over a table of every type with NULLs
    and special values; block 0 also holds the deepest program 64 ops allow."""
    rng = rng_for("rows", block)
    cols = special_table(rng, 300)
    rows = rows_of(cols)
    progs = [_selectref.random_program(rng, cols, int(rng.integers(1, 65))) for _ in range(25)]
    if block == 0:
        progs.append(_selectref.deepest_program(rng, cols))
        assert _selectref.max_depth(progs[-1]) == 32
    kept = 0
    for prog in progs:
        want = np.array([eval_row(prog, r, TYPES) for r in rows], dtype=bool)
        got = _selectref.mask(cols, prog)
        assert np.array_equal(got, want), prog
        kept += int(got.sum())
        n, out = _selectref.evaluate(select_plan(cols, prog, outs=[5, 0]))
        assert n == int(want.sum())
        assert pl.canonical_rows(_selectref.to_table(n, out)) == pl.canonical_rows(
            pl.table_from_rows([(r[5], r[0]) for r, w in zip(rows, want) if w], [F64, I32]))
    assert kept > 0


def test_reference_rules_by_hand():
    """NOT over NULL, the INT32 literal cut, NaN, a literal given as bits, either side NULL."""
    nan = float("nan")
    cols = [(I32, np.array([5, 7, 0, -1], np.int32), np.array([1, 1, 0, 1], bool)),
            (F64, np.array([nan, 1.5, -0.0, 2.0]), np.array([1, 1, 1, 0], bool)),
            (I32, np.array([5, 8, 0, -1], np.int32), np.array([1, 1, 1, 0], bool))]
    m = lambda prog: _selectref.mask(cols, prog).tolist()
    assert m([("LT", 0, 6)]) == [True, False, False, True]
    assert m([("LT", 0, 6), ("NOT",)]) == [False, True, True, False]           # the NULL row passes NOT (x < 6)
    assert m([("EQ", 0, 2**32 + 5)]) == [True, False, False, False]            # (int32_t)ivalue
    assert m([("EQ", 0, 2**32 - 1)]) == [False, False, False, True]
    assert m([("EQ", 1, nan)]) == [False] * 4 and m([("NEQ", 1, nan)]) == [True, True, True, False]
    assert m([("EQ", 1, 0.0)]) == [False, False, True, False]                  # -0.0 == 0.0
    bits = int(np.array([1.5]).view(np.int64)[0])
    assert m([("GEQ", 1, bits)]) == [False, True, False, False]                # an int literal is the double's bits
    assert m([("COL_EQ", 0, 2)]) == [True, False, False, False]
    assert m([("COL_NEQ", 0, 2)]) == [False, True, False, False]
    assert m([]) == [True] * 4


@pytest.mark.parametrize("seed", range(12))
def test_reference_is_tied_to_the_oracles_from_csv(seed):
    """Literal-only programs: select(scan T, prog) has the rows of the oracle's Table::from_csv of
    T's CSV text under the same program."""
    rng = rng_for("csv", seed)
    types = [I32, I64, F64, I32][: 2 + seed % 3]
    rows = _csvgen.random_rows(rng, int(rng.integers(1, 250)), types, null_p=0.15)
    prog = _csvgen.random_filter(rng, rows, types, depth=1 + seed % 4)
    want = _oracle.from_csv(_csvgen.to_csv(rng, rows), types, prog)
    t = pl.table_from_rows(rows, types)
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, dt) for i, dt in enumerate(types)])
    p.root = p.new_select_node(sc, prog, [(i, dt) for i, dt in enumerate(types)])
    p.new_input(t)
    got = _selectref.execute(p)
    assert got.num_rows == want.num_rows
    assert pl.canonical_rows(got) == pl.canonical_rows(want)


def _key_table(rng, kt, n, dom):
    k = km.key_values(kt, rng.integers(0, dom, n))
    k[: km.SPECIAL_KEYS[kt].shape[0]] = km.SPECIAL_KEYS[kt]
    return [(kt, k, rng.random(n) >= 0.1), km.payload(rng, I64, n, True)]


@pytest.mark.parametrize("kt", [I32, I64])
def test_key_equals_literal_is_the_oracles_join_with_a_one_row_table(kt):
    rng = rng_for("eq", kt)
    cols = _key_table(rng, kt, 400, 12)
    c = int(cols[0][1][200])
    j = pl.Plan()
    a = j.new_scan_node(0, [(0, kt), (1, I64)])
    b = j.new_scan_node(1, [(0, kt)])
    j.root = j.new_join_node(False, a, b, 0, 0, [(0, kt), (1, I64)])
    j.new_input(pl.make_table(cols))
    j.new_input(pl.make_table([(kt, np.array([c], dtype=km.NP_OF[kt]))]))
    want = _oracle.execute(j)
    got = _selectref.execute(select_plan(cols, [("EQ", 0, c)]))
    assert got.num_rows == want.num_rows > 0
    assert pl.canonical_rows(got) == pl.canonical_rows(want)


@pytest.mark.parametrize("kt", [I32, I64, F64])
def test_outer_join_where_optional_key_is_null_is_the_anti_join(kt):
    """select(outer(P, B), B.key IS NULL) -> P's columns is anti(P, B); the rows it leaves out are the
    oracle's inner join of P with B's distinct keys."""
    rng = rng_for("anti", kt)
    pcols = _key_table(rng, kt, 500, 40)
    bk = km.key_values(kt, rng.integers(20, 60, 300))
    bvalid = rng.random(300) >= 0.1
    p = pl.Plan()
    sp = p.new_scan_node(0, [(0, kt), (1, I64)])
    sb = p.new_scan_node(1, [(0, kt)])
    o = p.new_outer_join_node(False, sp, sb, 0, 0, [(0, kt), (1, I64), (2, kt)])   # P LEFT JOIN B
    p.root = p.new_select_node(o, [("IS_NULL", 2)], [(0, kt), (1, I64)])
    p.new_input(pl.make_table(pcols))
    p.new_input(pl.make_table([(kt, bk, bvalid)]))
    got = _selectref.execute(p)
    a = pl.Plan()
    a.nodes = p.nodes[:2]
    a.inputs = p.inputs
    a.root = a.new_anti_join_node(False, 0, 1, 0, 0, [(0, kt), (1, I64)])
    want = _filterref.execute(a)
    assert got.num_rows == want.num_rows > 0
    assert pl.canonical_rows(got) == pl.canonical_rows(want)
    j = pl.Plan()
    j.new_scan_node(0, [(0, kt), (1, I64)])
    j.new_scan_node(1, [(0, kt)])
    j.root = j.new_join_node(False, 0, 1, 0, 0, [(0, kt), (1, I64)])
    j.new_input(p.inputs[0])
    j.new_input(pl.make_table([(kt, np.unique(bk[bvalid]))]))
    matched = _oracle.execute(j)
    assert matched.num_rows > 0
    assert sorted(pl.canonical_rows(got) + pl.canonical_rows(matched), key=repr) == sorted(
        pl.canonical_rows(pl.make_table(pcols)), key=repr)


def test_reference_evaluates_nested_plans():
    """HAVING over an aggregation over a selection, under a join."""
    rng = rng_for("nest")
    n = 400
    cols = [(I32, rng.integers(0, 30, n).astype(np.int32), np.ones(n, bool)), (I64, rng.integers(0, 100, n), np.ones(n, bool))]
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    w = p.new_select_node(a, [("GEQ", 1, 50)], [(0, I32), (1, I64)])
    g = p.new_agg_node(w, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64)])
    h = p.new_select_node(g, [("GT", 1, 5)], [(0, I32), (1, I64)])
    b = p.new_scan_node(0, [(0, I32)])
    p.root = p.new_semi_join_node(False, h, b, 0, 0, [(0, I32), (1, I64)])
    p.new_input(pl.make_table(cols))
    k, v = cols[0][1], cols[1][1]
    want = sorted((int(x), int(((k == x) & (v >= 50)).sum())) for x in np.unique(k) if ((k == x) & (v >= 50)).sum() > 5)
    assert pl.sorted_rows(_selectref.execute(p)) == want and want
