"""Window nodes (RJ_NODE_WINDOW) without a GPU: marshalling, the header, the sharding refusal, the
kernel handles, and the numpy reference tests/_windowref.py pinned against a row-at-a-time second
reference: a dictionary of partitions filled row by row, each ordered by a comparator sort with the
sort tests' comparison rules, every frame walked row by row — written from the prose of include/rj.h
("Equality and order", "Frame", the function table), not from the encoding."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import _windowref
import test_gpu_kernel_matrix as km
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
COL, ROWNO, RANK, DENSE, STAR, COUNT, SUM, MIN, MAX = (pl.WIN_COL, pl.WIN_ROW_NUMBER, pl.WIN_RANK, pl.WIN_DENSE_RANK,
                                                       pl.WIN_COUNT_STAR, pl.WIN_COUNT, pl.WIN_SUM, pl.WIN_MIN, pl.WIN_MAX)
rng_for, ALL_FLAGS, EDGES, bits_of, f64_of = sp.rng_for, sp.ALL_FLAGS, sp.EDGES, sp.bits_of, sp.f64_of
CANON_NAN = 0x7FF8000000000000


def window_plan(cols, part_keys, order_keys, outputs):
    """Scan(cols) -> WINDOW; outputs = [(func, column, result type)]"""
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    p.root = p.new_window_node(sc, part_keys, order_keys, outputs)
    p.new_input(pl.make_table(cols))
    return p


def all_outputs(types, rng=None):
    """every ranking function, COUNT(*), every column passed through and under every legal function"""
    outs = [(ROWNO, 0, I64), (RANK, 0, I64), (DENSE, 0, I64), (STAR, 0, I64)]
    for c, dt in enumerate(types):
        outs += [(COL, c, dt), (COUNT, c, I64), (MIN, c, dt), (MAX, c, dt)] + ([(SUM, c, I64)] if dt != F64 else [])
    if rng is not None:
        outs = [outs[i] for i in rng.permutation(len(outs))[: int(rng.integers(0, len(outs) + 1))]]
    return outs


# ------------------------------------------------------------------ the second reference, from the prose
def canon_value(v, dt):
    if dt == F64:
        if math.isnan(v):
            return f64_of(CANON_NAN)
        if v == 0:
            return 0.0
    return v


def signed_bits(x):
    b = bits_of(x)
    return b - (2**64 if b >> 63 else 0)


def window_by_rows(cols, part_keys, order_keys, outputs):
    """-> result rows IN ORDER, doubles as ("f64", bits), None = NULL."""
    types = [c[0] for c in cols]
    rows = sp.python_rows(cols) if cols and cols[0][1].shape[0] else []

    def partition_of(row):   # NULL equals NULL per column, -0.0 equals +0.0, NaN equals NaN
        g = []
        for c, _ in part_keys:
            v = row[c]
            g.append(None if v is None else ("nan" if types[c] == F64 and math.isnan(v) else canon_value(v, types[c])))
        return tuple(g)

    parts = {}
    for r, row in enumerate(rows):
        parts.setdefault(partition_of(row), []).append(r)
    by_part = functools.cmp_to_key(lambda a, b: sp.compare_rows(rows[parts[a][0]], rows[parts[b][0]], part_keys, types))
    by_order = functools.cmp_to_key(lambda i, j: sp.compare_rows(rows[i], rows[j], order_keys, types))
    out = []
    for g in sorted(parts, key=by_part):
        members = sorted(parts[g], key=by_order)        # stable: ties keep the child's order
        peers = lambda i, j: sp.compare_rows(rows[members[i]], rows[members[j]], order_keys, types) == 0
        for at, r in enumerate(members):
            first_peer = at
            while first_peer > 0 and peers(first_peer - 1, at):
                first_peer -= 1
            last_peer = at
            while last_peer + 1 < len(members) and peers(last_peer + 1, at):
                last_peer += 1
            frame = members[: last_peer + 1]
            res = []
            for func, c, rt in outputs:
                if func == ROWNO:
                    v = at + 1
                elif func == RANK:
                    v = first_peer + 1
                elif func == DENSE:
                    v = 1 + sum(1 for k in range(1, at + 1) if not peers(k - 1, k))
                elif func == STAR:
                    v = len(frame)
                elif func == COL:
                    v = rows[r][c]
                    if v is not None and types[c] == F64:   # its own bits: read them off the column
                        v = ("f64", int(np.ascontiguousarray(cols[c][1]).view(np.int64)[r]))
                else:
                    dt = types[c]
                    vals = [rows[m][c] for m in frame if rows[m][c] is not None]
                    if func == COUNT:
                        v = len(vals)
                    elif not vals:
                        v = None
                    elif func == SUM:
                        v = (sum(vals) + 2**63) % 2**64 - 2**63
                    else:
                        best = vals[0]
                        for x in vals[1:]:
                            o = sp.compare_values(x, best, dt)
                            if (o < 0 and func == MIN) or (o > 0 and func == MAX):
                                best = x
                        v = canon_value(best, dt)
                res.append(("f64", signed_bits(v)) if isinstance(v, float) else v)
            out.append(tuple(res))
    return out


TYPES = [I32, I64, F64, I32, F64]


def random_keys(rng, lo, hi):
    return [(int(rng.integers(0, len(TYPES))), int(rng.integers(0, 4))) for _ in range(int(rng.integers(lo, hi)))]


@pytest.mark.parametrize("block", range(8))
def test_reference_agrees_with_the_row_at_a_time_partitions(block):
    """12 seeded window nodes per block: zero to two partition keys and zero to two order keys of all
    three types, all flags, NULLs, heavy ties, the edge values of every type (both zeros, several NaNs)
    among keys and values — position by position, doubles by their bits."""
    rng = rng_for("rows", block)
    n = int(rng.integers(1, 200)) if block else 0
    cols = sp.key_table(rng, n, TYPES, domain=int(rng.integers(1, 5))) if n else [(dt, np.zeros(0, km.NP_OF[dt]), np.zeros(0, bool)) for dt in TYPES]
    for _ in range(12):
        part, order = random_keys(rng, 0, 3), random_keys(rng, 0, 3)
        outputs = all_outputs(TYPES, rng)
        got_n, out = _windowref.window(cols, part, order, outputs, n)
        want = window_by_rows(cols, part, order, outputs)
        assert got_n == n == len(want)
        assert _windowref.rel_rows(out, n) == want, (part, order, outputs)


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_every_function_on_every_key_type_under_every_flag_set(dt, flags):
    """the edge list of the type (NULL, both zeros, four NaNs) as partition key, as order key and as value"""
    rng = rng_for("each", dt, flags)
    n = 120
    cols = sp.key_table(rng, n, [dt, dt, dt], domain=2)
    outputs = all_outputs([dt, dt, dt])
    for part, order in (([(0, flags)], [(1, flags)]), ([], [(0, flags)]), ([(1, flags)], []), ([(0, flags), (1, flags ^ DESC)], [(2, flags)])):
        got_n, out = _windowref.window(cols, part, order, outputs, n)
        assert _windowref.rel_rows(out, got_n) == window_by_rows(cols, part, order, outputs), (part, order)


def test_reference_rules_by_hand():
    nan = float("nan")
    f = lambda x: ("f64", signed_bits(x))
    #                      part  order  value
    cols = [(I32, np.array([1, 1, 1, 1, 2, 2, 0, 0], dtype=np.int32), np.array([1, 1, 1, 1, 1, 1, 0, 0], bool)),
            (F64, np.array([0.0, 5.0, -0.0, nan, 1.0, 1.0, -nan, 7.0]), np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)),
            (I64, np.array([2**62, 2**62, 2**62, 3, 0, 9, 4, 5]), np.array([1, 1, 1, 1, 0, 1, 1, 1], bool))]
    outs = [(COL, 2, I64), (ROWNO, 0, I64), (RANK, 0, I64), (DENSE, 0, I64), (STAR, 0, I64), (COUNT, 2, I64), (SUM, 2, I64), (MIN, 2, I64),
            (MAX, 1, F64)]
    n, out = _windowref.window(cols, [(0, 0)], [(1, 0)], outs)
    wrap = (3 * 2**62 + 2**63) % 2**64 - 2**63
    assert _windowref.rel_rows(out, n) == [
        # partition 1: the zeros are peers (stable: +0.0 first), then 5.0, then the NaN above it
        (2**62, 1, 1, 1, 2, 2, 2**63 - 2**64, 2**62, f(0.0)), (2**62, 2, 1, 1, 2, 2, 2**63 - 2**64, 2**62, f(0.0)),
        (2**62, 3, 3, 2, 3, 3, wrap, 2**62, f(5.0)), (3, 4, 4, 3, 4, 4, wrap + 3, 3, ("f64", CANON_NAN)),
        # partition 2: two peers, one NULL value: COUNT 1, the frame is both rows
        (None, 1, 1, 1, 2, 1, 9, 9, f(1.0)), (9, 2, 1, 1, 2, 1, 9, 9, f(1.0)),
        # the NULL partition comes last; its order key: the NaN, then NULL
        (4, 1, 1, 1, 1, 1, 4, 4, ("f64", CANON_NAN)), (5, 2, 2, 2, 2, 2, 9, 4, ("f64", CANON_NAN))]
    # without order keys the frame is the whole partition and all its rows are peers
    n, out = _windowref.window(cols, [(0, DESC | NF)], [], [(COL, 0, I32), (ROWNO, 0, I64), (RANK, 0, I64), (STAR, 0, I64), (SUM, 2, I64)])
    assert _windowref.rel_rows(out, n) == [(None, 1, 1, 2, 9), (None, 2, 1, 2, 9), (2, 1, 1, 2, 9), (2, 2, 1, 2, 9)] + \
        [(1, k, 1, 4, wrap + 3) for k in (1, 2, 3, 4)]
    # no key at all: one partition in the child's order
    n, out = _windowref.window(cols, [], [], [(ROWNO, 0, I64), (DENSE, 0, I64), (COUNT, 2, I64), (COL, 1, F64)])
    got = _windowref.rel_rows(out, n)
    assert [r[:3] for r in got] == [(k + 1, 1, 7) for k in range(8)]
    assert [r[3] for r in got][:3] == [f(0.0), f(5.0), f(-0.0)] and got[7][3] is None    # its own bits
    # a running value that goes NULL -> value
    run = [(I32, np.zeros(4, dtype=np.int32), np.ones(4, bool)), (I32, np.arange(4, dtype=np.int32), np.ones(4, bool)),
           (I32, np.array([7, 7, -5, 1], dtype=np.int32), np.array([0, 0, 1, 1], bool))]
    n, out = _windowref.window(run, [(0, 0)], [(1, 0)], [(SUM, 2, I64), (MIN, 2, I32), (COUNT, 2, I64)])
    assert _windowref.rel_rows(out, n) == [(None, None, 0), (None, None, 0), (-5, -5, 1), (-4, -5, 2)]
    # a column in both lists orders nothing; a repeated key neither
    a = _windowref.window(cols, [(0, 0)], [(0, DESC), (1, 0), (1, DESC)], outs)
    b = _windowref.window(cols, [(0, 0)], [(1, 0)], outs)
    assert _windowref.rel_rows(a[1], a[0]) == _windowref.rel_rows(b[1], b[0])
    none = [(dt, v[:0], m[:0]) for dt, v, m in cols]
    assert _windowref.window(none, [(0, 0)], [], outs, 0)[0] == 0


def test_reference_evaluates_nested_plans():
    """top-3 per partition (a selection over ROW_NUMBER), a grouping by DENSE_RANK, a window over a window"""
    rng = rng_for("nest")
    n = 500
    cols = [(I32, rng.integers(0, 20, n).astype(np.int32), np.ones(n, bool)), (I64, rng.permutation(n).astype(np.int64), np.ones(n, bool))]
    k, v = cols[0][1], cols[1][1]
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    w = p.new_window_node(a, [(0, 0)], [(1, DESC)], [(COL, 0, I32), (COL, 1, I64), (ROWNO, 0, I64)])
    p.root = p.new_select_node(w, [("LEQ", 2, 3)], [(0, I32), (1, I64), (2, I64)])
    p.new_input(pl.make_table(cols))
    want = sorted((int(x), int(y), r + 1) for x in np.unique(k) for r, y in enumerate(sorted(v[k == x], reverse=True)[:3]))
    assert pl.sorted_rows(_windowref.execute(p)) == want
    q = pl.Plan()
    a = q.new_scan_node(0, [(0, I32), (1, I64)])
    w = q.new_window_node(a, [], [(0, 0)], [(DENSE, 0, I64), (COL, 0, I32)])
    q.root = q.new_group_node(w, [(0, 0)], [(pl.AGG_KEY, 0, I64), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_MIN, 1, I32)])
    q.new_input(pl.make_table(cols))
    uniq = np.unique(k)
    assert pl.table_rows(_windowref.execute(q)) == [(d + 1, int((k == x).sum()), int(x)) for d, x in enumerate(uniq)]
    r = pl.Plan()
    a = r.new_scan_node(0, [(0, I32), (1, I64)])
    w = r.new_window_node(a, [(0, 0)], [], [(COL, 0, I32), (STAR, 0, I64)])
    r.root = r.new_window_node(w, [], [(1, DESC), (0, 0)], [(COL, 0, I32), (COL, 1, I64), (RANK, 0, I64)])
    r.new_input(pl.make_table(cols))
    sizes = sorted(((int((k == x).sum()), int(x)) for x in uniq), key=lambda t: (-t[0], t[1]))
    want, at = [], 0
    for size, x in sizes:
        want += [(x, size, at + 1)] * size
        at += size
    assert pl.table_rows(_windowref.execute(r)) == want


# ------------------------------------------------------------------ interface
def test_marshalling_round_trips_keys_and_outputs():
    cols = sp.key_table(rng_for("m"), 20, [I32, I64, F64])
    p = window_plan(cols, [(2, DESC), (0, NF)], [(1, 0), (2, 0), (1, DESC | NF)], [(COL, 2, F64), (ROWNO, 0, I64), (MAX, 1, I64), (STAR, 0, I64)])
    cp, keep = pl.plan_to_c(p)
    nd = cp.nodes[p.root]
    assert nd.kind == pl.NODE_WINDOW == 10 and nd.left == 0 and nd.n_out == 4
    assert nd.right == 5 and nd.left_attr == 2 and nd.right_attr != 0
    ks = C.cast(C.c_void_p(nd.right_attr), C.POINTER(pl.rj_sort_key))
    assert [(ks[k].column, ks[k].flags) for k in range(5)] == [(2, 1), (0, 2), (1, 0), (2, 0), (1, 3)]
    assert [nd.out_idx[k] for k in range(4)] == [pl.win_out(COL, 2), pl.win_out(ROWNO, 0), pl.win_out(MAX, 1), pl.win_out(STAR, 0)]
    assert [nd.out_idx[k] for k in range(4)] == [2, 1 << 56, (8 << 56) | 1, 4 << 56]
    assert [nd.out_type[k] for k in range(4)] == [F64, I64, I64, I64]
    assert [pl.win_func(nd.out_idx[k]) for k in range(4)] == [0, 1, 8, 4] and pl.win_col(nd.out_idx[2]) == 1
    assert (COL, ROWNO, RANK, DENSE, STAR, COUNT, SUM, MIN, MAX) == tuple(range(9))
    # no keys: a NULL pointer
    cp2, keep2 = pl.plan_to_c(window_plan(cols, [], [], [(STAR, 0, I64)]))
    nd = cp2.nodes[1]
    assert nd.kind == 10 and nd.right == 0 and nd.left_attr == 0 and nd.right_attr == 0 and nd.n_out == 1
    d = p.nodes[p.root].data
    assert isinstance(d, pl.WindowNode) and d.part_keys == [(2, 1), (0, 2)] and d.order_keys == [(1, 0), (2, 0), (1, 3)]
    del keep, keep2


def test_header_declares_the_kind_the_accessors_and_the_functions():
    h = open(os.path.join(os.path.dirname(km.LIB), "..", "include", "rj.h")).read()
    for text in ("RJ_NODE_WINDOW = 10", "#define RJ_WINDOW_N_KEYS(node) ((node)->right)",
                 "#define RJ_WINDOW_KEYS(node) ((const rj_sort_key*)(uintptr_t)(node)->right_attr)",
                 "#define RJ_WINDOW_N_PART(node) ((node)->left_attr)",
                 "#define RJ_WIN_OUT(func, col) (((uint64_t)(func) << 56) | (uint64_t)(col))",
                 "#define RJ_WIN_FUNC(x) ((uint32_t)((uint64_t)(x) >> 56))", "#define RJ_WIN_COL(x) ((uint64_t)(x) & 0x00ffffffffffffffull)",
                 "typedef enum rj_win_func {", "RJ_WIN_ROW_NUMBER = 1", "RJ_WIN_RANK       = 2", "RJ_WIN_DENSE_RANK = 3",
                 "RJ_WIN_COUNT_STAR = 4", "RJ_WIN_COUNT      = 5", "RJ_WIN_SUM        = 6", "RJ_WIN_MIN        = 7", "RJ_WIN_MAX        = 8",
                 "RANGE BETWEEN UNBOUNDED PRECEDING AND", "LAG / LEAD / FIRST_VALUE / NTILE"):
        assert text in h, text
    assert capi.load().rj_abi_version() == 3


def test_plan_shardable_refuses_window_nodes():
    cols = sp.key_table(rng_for("s"), 50, [I32, I32], null_p=0)
    ok, why = capi.plan_shardable(window_plan(cols, [(0, 0)], [(1, 0)], [(COL, 0, I32), (ROWNO, 0, I64)]))
    assert not ok and "RJ_NODE_WINDOW" in why
    q = pl.Plan()  # ... under a join
    a = q.new_scan_node(0, [(0, I32), (1, I32)])
    w = q.new_window_node(a, [(0, DESC)], [], [(COL, 0, I32)])
    b = q.new_scan_node(0, [(0, I32)])
    q.root = q.new_join_node(True, w, b, 0, 0, [(0, I32)])
    q.new_input(pl.make_table(cols))
    ok, why = capi.plan_shardable(q)
    assert not ok and "RJ_NODE_WINDOW" in why


def test_library_holds_the_window_kernels_and_no_new_group_or_sort_kernel():
    import _elfsyms
    names = {_elfsyms.short_name(n) for n in _elfsyms.kernel_handles(km.LIB)}
    assert {"k_win_one_head", "k_win_marks", "k_win_carry", "k_win_ranks", "k_win_tails<4>", "k_win_tails<8>", "k_win_tail_carry",
            "k_win_scan<4>", "k_win_scan<8>", "k_win_column"} == {n for n in names if n.startswith("k_win_")}
    assert {"k_group_heads<4>", "k_group_heads<8>", "k_group_scan", "k_group_keys<4>", "k_group_keys<8>", "k_group_init",
            "k_group_reduce<0,true>", "k_group_reduce<4,true>", "k_group_reduce<8,true>", "k_group_reduce<0,false>", "k_group_reduce<4,false>",
            "k_group_reduce<8,false>", "k_group_column"} == {n for n in names if n.startswith("k_group_")}
    assert {"k_sort_encode<4>", "k_sort_encode<8>", "k_sort_count<0>", "k_sort_count<1>", "k_sort_count<2>", "k_sort_scan",
            "k_sort_scatter<0>", "k_sort_scatter<1>", "k_sort_scatter<2>", "k_sort_iota"} == {n for n in names if n.startswith("k_sort_")}
    assert not any(n.split("<")[0].startswith("k_win_") for n in km.FAMILIES)
    hpp = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
    assert "constexpr int WIN_QUARTER = GROUP_TILE / GROUP_WAVES;" in hpp
    doc = open(os.path.join(os.path.dirname(km.LIB), "..", "INTEGRATION.md")).read()
    assert "RJ_TUNE_WIN_GRID" in doc
