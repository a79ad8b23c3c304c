"""Plain numpy reference for window nodes that hold the functions from WIN_LAG on (ROWS frames, LAG /
LEAD / FIRST_VALUE / LAST_VALUE, NTILE; "ROWS frames and LAG / LEAD / FIRST_VALUE / NTILE" in
include/rj.h), test infrastructure for tests/test_frame_plan.py and tests/test_gpu_frame.py.

The functions below WIN_LAG go to tests/_windowref.py, whose order and partition heads are used here
too.  Written from the header's prose: position i of the order lies in the partition [ps, pe], the
frame of (lo, hi) is [a, b] = [max(ps, i + lo), min(pe, i + hi)] in Python integers, empty when
a > b.  Two ways per function:
  by_slices   one slice a : b + 1 per row — for small inputs
  by_prefix   differences of cumulative counts and sums, a doubling table of range minima / maxima
              (the extreme of every span of 2^k positions; a range is two overlapping spans), gathers
              for the picks — for large ones
window() runs both up to CROSS_CHECK rows and asserts that they agree.

evaluate() handles every node kind: every other kind goes to tests/_fsumref.py (the reference that
knows them all) with its children evaluated HERE and handed over as the scans of a temporary plan.
A relation is a list of (type, values, valid) columns as in _filterref."""
from __future__ import annotations

import numpy as np

import _fsumref
import _groupref
import _setopref
import _sortref
import _windowref
from pyrj import plan as pl

NP_OF = _sortref.NP_OF
U64_MAX = np.uint64(2**64 - 1)
UNB_P, UNB_F = pl.WIN_UNBOUNDED_PRECEDING, pl.WIN_UNBOUNDED_FOLLOWING
PICKS = (pl.WIN_LAG, pl.WIN_LEAD, pl.WIN_FIRST_VALUE, pl.WIN_LAST_VALUE)
CROSS_CHECK = 300


def result_type(func, col_type):
    if func < pl.WIN_LAG:
        return _windowref.result_type(func, col_type)
    if func in PICKS or func in (pl.WIN_ROWS_MIN, pl.WIN_ROWS_MAX):
        return col_type
    return pl.INT64


def frame_of(func, lo, hi):
    """the frame a function reads: LAG k = the one row k in front, LEAD k = k behind"""
    if func == pl.WIN_LAG:
        assert lo >= 0 and hi == 0
        return -lo, -lo
    if func == pl.WIN_LEAD:
        assert lo >= 0 and hi == 0
        return lo, lo
    assert lo <= hi and lo != UNB_F and hi != UNB_P
    return lo, hi


def ntile(r, N, n):
    """PostgreSQL's rule in Python integers"""
    q, m = N // n, N % n
    if r < m * (q + 1):
        return r // (q + 1) + 1
    return m + (r - m * (q + 1)) // q + 1


def _frames(ps, pe, lo, hi):
    """-> (a, b) as lists of Python integers, a > b = empty"""
    return ([max(s, i + lo) for i, s in enumerate(ps)], [min(e, i + hi) for i, e in enumerate(pe)])


def by_slices(func, ct, cv, cvalid, enc, ps, pe, lo, hi):
    """-> (values list, valid list); cv / cvalid / enc in the ORDER (None for the column-less functions)"""
    n = len(ps)
    if func == pl.WIN_NTILE:
        return [ntile(i - ps[i], pe[i] - ps[i] + 1, lo) for i in range(n)], [True] * n
    a, b = _frames(ps, pe, *frame_of(func, lo, hi))
    vals, ok = [], []
    for i in range(n):
        empty = a[i] > b[i]
        if func == pl.WIN_ROWS_COUNT_STAR:
            v, o = (0 if empty else b[i] - a[i] + 1), True
        elif func in PICKS:
            s = b[i] if func == pl.WIN_LAST_VALUE else a[i]
            o = not empty and bool(cvalid[s])
            v = cv[s] if o else cv.dtype.type(0)
        else:
            sl = slice(a[i], b[i] + 1) if not empty else slice(0, 0)
            m = cvalid[sl]
            cnt = int(m.sum())
            if func == pl.WIN_ROWS_COUNT:
                v, o = cnt, True
            elif cnt == 0:
                v, o = 0, False
            elif func == pl.WIN_ROWS_SUM:
                v, o = (sum(int(x) for x in cv[sl][m]) + 2**63) % 2**64 - 2**63, True
            else:
                e = enc[sl][m]
                v, o = (e.min() if func == pl.WIN_ROWS_MIN else e.max()), True
        vals.append(v)
        ok.append(o)
    return vals, ok


def _span_table(x, ufunc):
    """t[k][i] = ufunc over x[i : i + 2^k], for every k with 2^k <= len(x)"""
    t = [x]
    k = 1
    while 2 * k <= x.shape[0]:
        t.append(ufunc(t[-1][:-k], t[-1][k:]))
        k *= 2
    return t


def by_prefix(func, ct, cv, cvalid, enc, ps, pe, lo, hi):
    n = ps.shape[0]
    pos = np.arange(n, dtype=np.int64)
    if func == pl.WIN_NTILE:
        N, r = pe - ps + 1, pos - ps
        q, m = N // lo, N % lo
        big = m * (q + 1)
        v = np.where(r < big, r // (q + 1), m + (r - big) // np.maximum(q, 1)) + 1
        return v, np.ones(n, bool)
    lo, hi = frame_of(func, lo, hi)
    cl = lambda x: max(-2**33, min(2**33, x))       # |offset| >= 2^32 is beyond every relation
    a, b = np.maximum(ps, pos + cl(lo)), np.minimum(pe, pos + cl(hi))
    full = a <= b
    a, b = np.where(full, a, 0), np.where(full, b, 0)
    if func == pl.WIN_ROWS_COUNT_STAR:
        return np.where(full, b - a + 1, 0), np.ones(n, bool)
    if func in PICKS:
        s = b if func == pl.WIN_LAST_VALUE else a
        o = full & cvalid[s]
        return np.where(o, cv[s], cv.dtype.type(0)), o
    c0 = np.r_[0, np.cumsum(cvalid.astype(np.int64))]
    cnt = np.where(full, c0[b + 1] - c0[a], 0)
    if func == pl.WIN_ROWS_COUNT:
        return cnt, np.ones(n, bool)
    if func == pl.WIN_ROWS_SUM:
        s0 = np.r_[np.uint64(0), np.cumsum(np.where(cvalid, cv.astype(np.int64), 0).view(np.uint64))]
        return np.where(cnt > 0, (s0[b + 1] - s0[a]).view(np.int64), 0), cnt > 0
    mn = func == pl.WIN_ROWS_MIN
    x = np.where(cvalid, enc, U64_MAX if mn else np.uint64(0))
    t = _span_table(x, np.minimum if mn else np.maximum)
    ln = b - a + 1
    k = np.floor(np.log2(ln)).astype(np.int64)
    out = np.zeros(n, np.uint64)
    for kk in np.unique(k).tolist():
        at = np.flatnonzero(k == kk)
        left, right = t[kk][a[at]], t[kk][b[at] - 2**kk + 1]
        out[at] = np.minimum(left, right) if mn else np.maximum(left, right)
    return out, cnt > 0


def window(cols, part_keys, order_keys, outputs, n=None):
    """cols: the child's columns; outputs: [(func, column, result type)] for the functions below WIN_LAG,
    [(func, column, result type, lo, hi)] from there on -> (rows, columns), in the node's order."""
    n = (cols[0][1].shape[0] if cols else 0) if n is None else n
    part_keys, order_keys = [tuple(k) for k in part_keys], [tuple(k) for k in order_keys]
    old = [tuple(o[:3]) for o in outputs if o[0] < pl.WIN_LAG]
    _, old_cols = _windowref.window(cols, part_keys, order_keys, old, n)
    old_cols = iter(old_cols)
    order = _sortref.order(cols, part_keys + order_keys) if cols else np.arange(n)
    P = _windowref._heads(cols, part_keys, order, n)
    pos = np.arange(n, dtype=np.int64)
    if n:
        ps = np.maximum.accumulate(np.where(P, pos, 0))
        nextp = np.where(P, pos, n)
        pe = np.minimum.accumulate(np.r_[nextp[1:], n][::-1])[::-1] - 1
    else:
        ps = pe = pos
    out = []
    for o in outputs:
        func, c, rt = o[:3]
        if func < pl.WIN_LAG:
            out.append(next(old_cols))
            continue
        lo, hi = int(o[3]), int(o[4])
        ct = cv = cvalid = enc = None
        if func in (pl.WIN_NTILE, pl.WIN_ROWS_COUNT_STAR):
            assert c == 0 and rt == pl.INT64 and (func != pl.WIN_NTILE or (lo >= 1 and hi == 0))
        else:
            ct = cols[c][0]
            assert ct in NP_OF and rt == result_type(func, ct) and not (func == pl.WIN_ROWS_SUM and ct == pl.FP64)
            cv, cvalid = np.asarray(cols[c][1], dtype=NP_OF[ct])[order], np.asarray(cols[c][2], dtype=bool)[order]
            _, enc = _sortref.encode(ct, cv, cvalid, 0)
        v, ok = by_prefix(func, ct, cv, cvalid, enc, ps, pe, lo, hi)
        v, ok = np.asarray(v), np.asarray(ok, dtype=bool)
        if n <= CROSS_CHECK:
            v2, ok2 = by_slices(func, ct, cv, cvalid, enc, ps.tolist(), pe.tolist(), lo, hi)
            assert ok.tolist() == list(ok2), (func, lo, hi)
            bits = lambda x: x.view(np.uint64 if x.dtype.itemsize == 8 else np.uint32)
            assert np.array_equal(bits(v)[ok], bits(np.array(v2, dtype=v.dtype))[ok]), (func, lo, hi)
        if func in (pl.WIN_ROWS_MIN, pl.WIN_ROWS_MAX):
            v = np.where(ok, _groupref.decode(ct, v.astype(np.uint64)), np.zeros(1, dtype=NP_OF[ct]))
        out.append((rt, v.astype(NP_OF[rt]) if v.dtype != NP_OF[rt] else v, ok))
    return n, out


def outputs_of(node):
    args = node.data.args or [None] * len(node.output_attrs)
    return [(pl.win_func(x), pl.win_col(x), t) + (tuple(a) if a is not None else ()) for (x, t), a in zip(node.output_attrs, args)]


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root), as _windowref.evaluate"""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return _windowref.evaluate(plan, idx)
    if isinstance(d, pl.WindowNode):
        n, child = evaluate(plan, d.child)
        return window(child, d.part_keys, d.order_keys, outputs_of(node), n)
    tmp = pl.Plan()
    moved = {}
    for field, kid in _setopref.children(d):
        n, cols = evaluate(plan, kid)
        moved[field] = tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)])
        tmp.new_input(_windowref.to_table(n, cols))
    tmp.nodes.append(pl.PlanNode(type(d)(**{**d.__dict__, **moved}), list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _fsumref.evaluate(tmp)


to_table = _windowref.to_table
rel_rows = _windowref.rel_rows
decoded_rows = _windowref.decoded_rows
