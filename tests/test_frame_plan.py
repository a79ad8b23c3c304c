"""ROWS frames, LAG / LEAD / FIRST_VALUE / LAST_VALUE and NTILE of window nodes on the CPU: the numpy
reference tests/_frameref.py against a row-at-a-time walk over a dictionary of partitions (Python
integers, frames as list slices, written from the prose of include/rj.h), the two host twins of the
kernels' frame arithmetic (rj_debug_win_frame, rj_debug_win_ntile) against Python integers, the
marshalling of RJ_WINDOW_ARGS, the header and the compiled kernel sets."""
import ctypes as C
import functools
import itertools
import math
import os

import numpy as np
import pytest

import _frameref
import test_gpu_kernel_matrix as km
import test_sort_plan as sp
import test_window_plan as wp
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
COL, ROWNO, RANK, DENSE, STAR, COUNT, SUM, MIN, MAX = wp.COL, wp.ROWNO, wp.RANK, wp.DENSE, wp.STAR, wp.COUNT, wp.SUM, wp.MIN, wp.MAX
LAG, LEAD, FIRST, LAST, NTILE = pl.WIN_LAG, pl.WIN_LEAD, pl.WIN_FIRST_VALUE, pl.WIN_LAST_VALUE, pl.WIN_NTILE
RSTAR, RCOUNT, RSUM, RMIN, RMAX = pl.WIN_ROWS_COUNT_STAR, pl.WIN_ROWS_COUNT, pl.WIN_ROWS_SUM, pl.WIN_ROWS_MIN, pl.WIN_ROWS_MAX
UNB_P, UNB_F = pl.WIN_UNBOUNDED_PRECEDING, pl.WIN_UNBOUNDED_FOLLOWING
rng_for, window_plan = sp.rng_for, wp.window_plan
FRAMES = [(-1, -1), (1, 1), (0, 0), (-1, 1), (-6, 0), (0, 6), (-63, 0), (-64, 0), (-65, 0), (-1024, 1024), (-5000, -4000), (UNB_P, 0), (0, UNB_F),
          (UNB_P, UNB_F), (UNB_P, -1), (1, UNB_F), (-2**40, 2**40)]


def frame_outputs(types, frames, rng=None, offsets=(0, 1, 2, 7), buckets=(1, 2, 3, 64)):
    """every function from WIN_LAG on over every column it is legal on, under every frame / offset / bucket count"""
    outs = [(NTILE, 0, I64, n, 0) for n in buckets] + [(RSTAR, 0, I64, lo, hi) for lo, hi in frames]
    for c, dt in enumerate(types):
        outs += [(f, c, dt, k, 0) for f in (LAG, LEAD) for k in offsets]
        for lo, hi in frames:
            outs += [(FIRST, c, dt, lo, hi), (LAST, c, dt, lo, hi), (RCOUNT, c, I64, lo, hi), (RMIN, c, dt, lo, hi), (RMAX, c, dt, lo, hi)]
            outs += [(RSUM, c, I64, lo, hi)] if dt != F64 else []
    if rng is not None:
        outs = [outs[i] for i in rng.permutation(len(outs))[: int(rng.integers(1, 25))]]
    return outs


# ------------------------------------------------------------------ the second reference, from the prose
def frame_by_rows(cols, part_keys, order_keys, outputs):
    """-> result rows IN ORDER, doubles as ("f64", bits), None = NULL; the functions below WIN_LAG through
    test_window_plan.window_by_rows"""
    types = [c[0] for c in cols]
    rows = sp.python_rows(cols) if cols and cols[0][1].shape[0] else []
    old = wp.window_by_rows(cols, part_keys, order_keys, [o for o in outputs if o[0] < LAG])

    def partition_of(row):
        g = []
        for c, _ in part_keys:
            v = row[c]
            g.append(None if v is None else ("nan" if types[c] == F64 and math.isnan(v) else wp.canon_value(v, types[c])))
        return tuple(g)

    def own_bits(r, c):
        v = rows[r][c]
        if v is not None and types[c] == F64:
            return ("f64", int(np.ascontiguousarray(cols[c][1]).view(np.int64)[r]))
        return v

    parts = {}
    for r, row in enumerate(rows):
        parts.setdefault(partition_of(row), []).append(r)
    by_part = functools.cmp_to_key(lambda a, b: sp.compare_rows(rows[parts[a][0]], rows[parts[b][0]], part_keys, types))
    by_order = functools.cmp_to_key(lambda i, j: sp.compare_rows(rows[i], rows[j], order_keys, types))
    out = []
    for g in sorted(parts, key=by_part):
        members = sorted(parts[g], key=by_order)        # stable: ties keep the child's order
        N = len(members)
        for at in range(N):
            res, old_row = [], iter(old[len(out)])
            for o in outputs:
                func, c = o[0], o[1]
                if func < LAG:
                    res.append(next(old_row))
                    continue
                lo, hi = o[3], o[4]
                if func == NTILE:
                    buckets = [b + 1 for b in range(min(lo, N)) for _ in range(N // lo + (1 if b < N % lo else 0))]
                    assert len(buckets) == N
                    res.append(buckets[at])
                    continue
                if func in (LAG, LEAD):
                    s = at - lo if func == LAG else at + lo
                    res.append(own_bits(members[s], c) if 0 <= s < N else None)
                    continue
                first, last = max(0, at + lo), min(N - 1, at + hi)
                frame = members[first:last + 1] if first <= last else []
                if func == RSTAR:
                    v = len(frame)
                elif func in (FIRST, LAST):
                    v = own_bits(frame[0] if func == FIRST else frame[-1], c) if frame else None
                else:
                    dt = types[c]
                    vals = [rows[m][c] for m in frame if rows[m][c] is not None]
                    if func == RCOUNT:
                        v = len(vals)
                    elif not vals:
                        v = None
                    elif func == RSUM:
                        v = (sum(vals) + 2**63) % 2**64 - 2**63
                    else:
                        best = vals[0]
                        for x in vals[1:]:
                            cmp = sp.compare_values(x, best, dt)
                            if (cmp < 0 and func == RMIN) or (cmp > 0 and func == RMAX):
                                best = x
                        v = wp.canon_value(best, dt)
                res.append(("f64", wp.signed_bits(v)) if isinstance(v, float) else v)
            out.append(tuple(res))
    return out


TYPES = [I32, I64, F64, I32, F64]
SMALL_FRAMES = [(-1, -1), (1, 1), (0, 0), (-1, 1), (-6, 0), (0, 6), (-3, -2), (2, 5), (UNB_P, 0), (0, UNB_F), (UNB_P, UNB_F), (UNB_P, -1), (1, UNB_F),
                (-2**40, 2**40), (-2**63 + 1, 2**63 - 2)]


@pytest.mark.parametrize("block", range(8))
def test_reference_agrees_with_the_row_at_a_time_partitions(block):
    """10 seeded window nodes per block over keys of all three types with NULLs, heavy ties and the edge
    values of every type, old and new functions mixed — position by position, doubles by their bits
    (window() also cross-checks its two ways of computing every column)"""
    rng = rng_for("frame-rows", block)
    n = int(rng.integers(1, 160)) if block else 0
    cols = sp.key_table(rng, n, TYPES, domain=int(rng.integers(1, 5))) if n else [(dt, np.zeros(0, km.NP_OF[dt]), np.zeros(0, bool)) for dt in TYPES]
    for _ in range(10):
        part, order = wp.random_keys(rng, 0, 3), wp.random_keys(rng, 0, 3)
        outputs = frame_outputs(TYPES, SMALL_FRAMES, rng, offsets=(0, 1, 2, 7, n, 2**63 - 1), buckets=(1, 2, 3, 64, max(n, 1), n + 1, 2**40))
        outputs += [wp.all_outputs(TYPES)[i] for i in rng.permutation(10)[:3]]
        got_n, out = _frameref.window(cols, part, order, outputs, n)
        want = frame_by_rows(cols, part, order, outputs)
        assert got_n == n == len(want)
        assert _frameref.rel_rows(out, n) == want, (part, order, outputs)


def test_reference_rules_by_hand():
    nan = float("nan")
    f = lambda x: ("f64", wp.signed_bits(x))
    #                      part                order            value
    cols = [(I32, np.array([1, 1, 1, 1, 1, 2, 2], dtype=np.int32), np.ones(7, bool)), (I32, np.arange(7, dtype=np.int32), np.ones(7, bool)),
            (I64, np.array([2**63 - 1, 5, 0, 2**63 - 1, 1, -2**63, 7]), np.array([1, 0, 0, 1, 1, 1, 0], bool)),
            (F64, np.array([-0.0, nan, 2.0, 0.0, -1.0, 3.0, 4.0]), np.array([1, 1, 1, 1, 0, 1, 1], bool))]
    outs = [(LAG, 2, I64, 1, 0), (LEAD, 3, F64, 2, 0), (RSUM, 2, I64, -1, 0), (RMIN, 2, I64, -2, -1), (RMAX, 2, I64, 0, UNB_F), (RCOUNT, 2, I64, -1, 1),
            (NTILE, 0, I64, 2, 0), (RMAX, 3, F64, -1, 0), (FIRST, 3, F64, -1, 0), (RSTAR, 0, I64, 1, 2)]
    n, out = _frameref.window(cols, [(0, 0)], [(1, 0)], outs)
    top, low = 2**63 - 1, -2**63
    assert _frameref.rel_rows(out, n) == [
        # partition 1 (5 rows: buckets 1 1 1 2 2); INT64_MAX under MIN next to NULLs is a value; the sum of two maxima wraps ... not here: NULLs between
        (None, f(2.0), top, None, top, 1, 1, f(0.0), ("f64", -2**63), 2),
        (top, f(0.0), top, top, top, 1, 1, ("f64", wp.CANON_NAN), ("f64", -2**63), 2),
        (None, None, None, top, top, 1, 1, ("f64", wp.CANON_NAN), f(nan), 2),
        (None, None, top, None, top, 2, 2, f(2.0), f(2.0), 1),
        (top, None, low, top, 1, 2, 2, f(0.0), f(0.0), 0),
        # partition 2: INT64_MIN under MAX is a value; the frame behind the last row is empty
        (None, None, low, None, low, 1, 1, f(3.0), f(3.0), 1),
        (low, None, low, low, None, 1, 2, f(4.0), f(3.0), 0)]
    assert f(nan) == ("f64", wp.CANON_NAN)          # (the table's NaN happens to be the canonical one)


def test_reference_evaluates_nested_plans():
    """x - LAG(x) through a MAP above, a selection LEAD IS NULL above, a window over a window"""
    rng = rng_for("frame-nest")
    n = 400
    cols = [(I32, rng.integers(0, 15, n).astype(np.int32), np.ones(n, bool)), (I64, rng.permutation(n).astype(np.int64), np.ones(n, bool))]
    k, v = cols[0][1], cols[1][1]
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    w = p.new_window_node(a, [(0, 0)], [(1, 0)], [(COL, 0, I32), (COL, 1, I64), (LAG, 1, I64, 1, 0)])
    p.root = p.new_map_node(w, [("COL", 1), ("COL", 2), ("SUB",), ("OUT",)], [("COL", 0, I32), ("EXPR", 0, I64)])
    p.new_input(pl.make_table(cols))
    want = []
    for x in np.unique(k):
        s = sorted(v[k == x].tolist())
        want += [(int(x), None)] + [(int(x), b - a_) for a_, b in zip(s, s[1:])]
    key = lambda r: (r[0], -1 if r[1] is None else r[1])
    assert sorted(pl.table_rows(_frameref.to_table(*_frameref.evaluate(p))), key=key) == sorted(want, key=key)
    q = pl.Plan()
    a = q.new_scan_node(0, [(0, I32), (1, I64)])
    w = q.new_window_node(a, [(0, 0)], [(1, 0)], [(COL, 0, I32), (COL, 1, I64), (LEAD, 1, I64, 1, 0)])
    q.root = q.new_select_node(w, [("IS_NULL", 2)], [(0, I32), (1, I64)])
    q.new_input(pl.make_table(cols))
    assert sorted(pl.table_rows(_frameref.to_table(*_frameref.evaluate(q)))) == sorted((int(x), int(v[k == x].max())) for x in np.unique(k))
    r = pl.Plan()
    a = r.new_scan_node(0, [(0, I32), (1, I64)])
    w = r.new_window_node(a, [(0, 0)], [(1, 0)], [(COL, 0, I32), (RSUM, 1, I64, -1, 0)])
    r.root = r.new_window_node(w, [], [(1, 0), (0, 0)], [(COL, 1, I64), (RMAX, 1, I64, UNB_P, 0), (STAR, 0, I64)])
    r.new_input(pl.make_table(cols))
    n2, out = _frameref.evaluate(r)
    rows = _frameref.rel_rows(out, n2)
    assert n2 == n and all(row[0] == row[1] and row[2] >= i + 1 for i, row in enumerate(rows))   # sorted ascending: the running maximum is the row


# ------------------------------------------------------------------ the host twins of the kernels' arithmetic
def test_debug_win_frame_against_python_integers():
    at = [0, 1, 63, 64, 2**32 - 17]
    offs = [-2**63, -2**32, -65, -1, 0, 1, 64, 2**32, 2**63 - 1]
    checked = empty = 0
    for i, ps, pe in itertools.product(at, at, at):
        for lo, hi in itertools.product(offs, offs):
            if lo > hi:
                continue
            a, b = max(ps, i + lo), min(pe, i + hi)
            got = capi.win_frame(i, ps, pe, lo, hi)
            assert got == ((a, b) if a <= b else None), (i, ps, pe, lo, hi)
            checked += 1
            empty += got is None
    assert checked == 125 * 45 and 0 < empty < checked
    # the reference's frames are the same arithmetic
    a, b = _frameref._frames([0, 0, 2], [1, 1, 2], -1, 0)
    assert (a, b) == ([0, 0, 2], [0, 1, 2])


def test_debug_win_ntile_against_a_brute_force_bucket_list():
    for N in range(1, 71):
        for n in list(range(1, 76)) + [2**63 - 1]:
            q, m = divmod(N, n)
            buckets = [b + 1 for b in range(min(n, N)) for _ in range(q + (1 if b < m else 0))]
            assert len(buckets) == N
            got = [capi.win_ntile(r, N, n) for r in range(N)]
            assert got == buckets == [_frameref.ntile(r, N, n) for r in range(N)], (N, n)
    assert capi.win_ntile(0, 5, 0) == 0 and capi.win_ntile(5, 5, 2) == 0 and capi.win_ntile(0, 1, -3) == 0
    assert capi.win_ntile(2**32 - 18, 2**32 - 17, 2**40) == 2**32 - 17


# ------------------------------------------------------------------ interface
def test_marshalling_fills_the_argument_array_only_when_needed():
    cols = sp.key_table(rng_for("fm"), 20, [I32, I64, F64])
    old = window_plan(cols, [(0, 0)], [(1, 0)], [(COL, 2, F64), (ROWNO, 0, I64), (MAX, 1, I64)])
    cp, keep = pl.plan_to_c(old)
    assert cp.nodes[old.root].base_table_id == 0 and old.nodes[old.root].data.args is None
    outs = [(COL, 2, F64), (LAG, 1, I64, 3, 0), (MAX, 1, I64), (RSUM, 1, I64, UNB_P, -1), (RMIN, 2, F64, -6, UNB_F), (NTILE, 0, I64, 4, 0), (RSUM, 1, I64, -2, 2)]
    p = window_plan(cols, [(2, DESC)], [(1, 0)], outs)
    cp2, keep2 = pl.plan_to_c(p)
    nd = cp2.nodes[p.root]
    assert nd.kind == pl.NODE_WINDOW and nd.n_out == 7 and nd.base_table_id != 0 and nd.left_attr == 1 and nd.right == 2
    args = C.cast(C.c_void_p(nd.base_table_id), C.POINTER(pl.rj_win_arg))
    assert [(args[k].lo, args[k].hi) for k in range(7)] == [(0, 0), (3, 0), (0, 0), (-2**63, -1), (-6, 2**63 - 1), (4, 0), (-2, 2)]
    assert [nd.out_idx[k] for k in range(7)] == [2, (16 << 56) | 1, (8 << 56) | 1, (23 << 56) | 1, (24 << 56) | 2, 20 << 56, (23 << 56) | 1]
    assert [nd.out_type[k] for k in range(7)] == [F64, I64, I64, I64, F64, I64, I64]
    d = p.nodes[p.root].data
    assert d.args == [None, (3, 0), None, (UNB_P, -1), (-6, UNB_F), (4, 0), (-2, 2)]
    assert type(d)(**d.__dict__) == d and pl.WindowNode(0, [], []).args is None      # constructible from its fields, the new one defaulted
    assert _frameref.outputs_of(p.nodes[p.root]) == outs
    assert C.sizeof(pl.rj_win_arg) == 16
    del keep, keep2


def test_constants_header_and_exports():
    assert (pl.WIN_COL, pl.WIN_ROW_NUMBER, pl.WIN_RANK, pl.WIN_DENSE_RANK, pl.WIN_COUNT_STAR, pl.WIN_COUNT, pl.WIN_SUM, pl.WIN_MIN,
            pl.WIN_MAX) == tuple(range(9))
    assert (LAG, LEAD, FIRST, LAST, NTILE, RSTAR, RCOUNT, RSUM, RMIN, RMAX) == tuple(range(16, 26))
    assert (UNB_P, UNB_F) == (-2**63, 2**63 - 1)
    h = open(os.path.join(os.path.dirname(km.LIB), "..", "include", "rj.h")).read()
    for text in ("RJ_WIN_MAX        = 8", "RJ_WIN_LAG = 16, RJ_WIN_LEAD = 17, RJ_WIN_FIRST_VALUE = 18, RJ_WIN_LAST_VALUE = 19, RJ_WIN_NTILE = 20,",
                 "RJ_WIN_ROWS_COUNT_STAR = 21, RJ_WIN_ROWS_COUNT = 22, RJ_WIN_ROWS_SUM = 23, RJ_WIN_ROWS_MIN = 24, RJ_WIN_ROWS_MAX = 25",
                 "typedef struct rj_win_arg { int64_t lo, hi; } rj_win_arg;", "#define RJ_WIN_UNBOUNDED_PRECEDING INT64_MIN",
                 "#define RJ_WIN_UNBOUNDED_FOLLOWING INT64_MAX",
                 "#define RJ_WINDOW_ARGS(node) ((const rj_win_arg*)(uintptr_t)(node)->base_table_id)",
                 "int rj_debug_win_frame(uint64_t i, uint64_t ps, uint64_t pe, int64_t lo, int64_t hi, uint64_t* a, uint64_t* b);",
                 "int64_t rj_debug_win_ntile(uint64_t r, uint64_t N, int64_t n);",
                 "RANGE BETWEEN UNBOUNDED PRECEDING AND", "ROWS frames and LAG / LEAD / FIRST_VALUE / NTILE"):
        assert text in h, text
    assert "Out of scope: ROWS" not in h and "NTH_VALUE" in h and "IGNORE NULLS" in h and "EXCLUDE" in h
    assert "rj_debug_win_frame" in capi.EXPORTS and "rj_debug_win_ntile" in capi.EXPORTS
    L = capi.load()
    assert L.rj_abi_version() == 3 and hasattr(L, "rj_debug_win_frame") and hasattr(L, "rj_debug_win_ntile")


def test_library_holds_the_frame_kernels_and_no_new_window_group_or_sort_kernel():
    import _elfsyms
    names = {_elfsyms.short_name(n) for n in _elfsyms.kernel_handles(km.LIB)}
    assert {"k_frame_pick<4>", "k_frame_pick<8>", "k_frame_ntile", "k_frame_sum", "k_frame_leaves<4>", "k_frame_leaves<8>", "k_frame_levels",
            "k_frame_extreme"} == {n for n in names if n.startswith("k_frame_")}
    assert {"k_win_one_head", "k_win_marks", "k_win_carry", "k_win_ranks", "k_win_tails<4>", "k_win_tails<8>", "k_win_tail_carry",
            "k_win_scan<4>", "k_win_scan<8>", "k_win_column"} == {n for n in names if n.startswith("k_win_")}
    assert {"k_group_heads<4>", "k_group_heads<8>", "k_group_scan", "k_group_keys<4>", "k_group_keys<8>", "k_group_init",
            "k_group_reduce<0,true>", "k_group_reduce<4,true>", "k_group_reduce<8,true>", "k_group_reduce<0,false>", "k_group_reduce<4,false>",
            "k_group_reduce<8,false>", "k_group_column"} == {n for n in names if n.startswith("k_group_")}
    assert {"k_sort_encode<4>", "k_sort_encode<8>", "k_sort_count<0>", "k_sort_count<1>", "k_sort_count<2>", "k_sort_scan",
            "k_sort_scatter<0>", "k_sort_scatter<1>", "k_sort_scatter<2>", "k_sort_iota"} == {n for n in names if n.startswith("k_sort_")}
    hpp = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
    assert "constexpr int FRAME_FANOUT = 16;" in hpp


def test_plan_shardable_still_refuses_window_nodes():
    cols = sp.key_table(rng_for("fs"), 50, [I32, I32], null_p=0)
    ok, why = capi.plan_shardable(window_plan(cols, [(0, 0)], [(1, 0)], [(COL, 0, I32), (LAG, 1, I32, 1, 0), (RMIN, 1, I32, -6, 0)]))
    assert not ok and "RJ_NODE_WINDOW" in why
