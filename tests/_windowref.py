"""Plain numpy reference for plans that hold window nodes (pl.WindowNode, RJ_NODE_WINDOW in
include/rj.h), test infrastructure for tests/test_window_plan.py and tests/test_gpu_window.py.

A window node is computed here: np.lexsort (stable) orders the child's rows by the encoded keys
(_sortref.order over partition keys + order keys), a row starts a partition where any (NULL digit,
key) pair of a partition key differs from the row before it, and a peer group where that or any pair
of an order key does.  The ranks are arithmetic on the positions of those heads.  The aggregates are
np.add.accumulate / np.minimum.accumulate / np.maximum.accumulate per partition, taken at every row's
PEER END (the frame of rj.h: up to and including the last peer; the whole partition without order
keys, where all its rows are peers).  MIN / MAX accumulate the ENCODED value as an unsigned number and
decode it again (_groupref.decode), so FP64 follows the sort's order and comes back canonical.

evaluate() handles every node kind, so nested plans can be checked: every other kind goes to
tests/_groupref.py with its children evaluated HERE and handed over as the scans of a temporary plan.
A relation is a list of (type, values, valid) columns as in _filterref."""
from __future__ import annotations

import numpy as np

import _filterref
import _groupref
import _sortref
from pyrj import plan as pl

NP_OF = _sortref.NP_OF
U64_MAX = np.uint64(2**64 - 1)
RANKING = (pl.WIN_ROW_NUMBER, pl.WIN_RANK, pl.WIN_DENSE_RANK)


def result_type(func, col_type):
    if func in (pl.WIN_COL, pl.WIN_MIN, pl.WIN_MAX):
        return col_type
    return pl.INT64


def _heads(cols, keys, order, n):
    head = np.zeros(n, dtype=bool)
    if n:
        head[0] = True
    for c, flags in keys:
        nd, key = _sortref.encode(cols[c][0], cols[c][1], cols[c][2], flags)
        nd, key = nd[order], key[order]
        head[1:] |= (nd[1:] != nd[:-1]) | (key[1:] != key[:-1])
    return head


def _accumulate(ufunc, arr, starts, n):
    """ufunc.accumulate over every run [starts[k], starts[k + 1]) of arr"""
    out = arr.copy()
    ends = np.r_[starts[1:], n]
    for b, e in zip(starts.tolist(), ends.tolist()):
        if e - b > 1:
            out[b:e] = ufunc.accumulate(arr[b:e])
    return out


def window(cols, part_keys, order_keys, outputs, n=None):
    """cols: the child's columns; part_keys / order_keys: [(column, flags)]; outputs: [(func, column,
    result type)] -> (rows, columns), the rows ordered by (part_keys, order_keys)."""
    n = (cols[0][1].shape[0] if cols else 0) if n is None else n
    part_keys, order_keys = [tuple(k) for k in part_keys], [tuple(k) for k in order_keys]
    order = _sortref.order(cols, part_keys + order_keys) if cols else np.arange(n)
    P = _heads(cols, part_keys, order, n)
    Q = P | _heads(cols, order_keys, order, n)
    pos = np.arange(n, dtype=np.int64)
    starts = np.flatnonzero(P)
    if n:
        pstart = np.maximum.accumulate(np.where(P, pos, 0))          # the partition's first position
        qstart = np.maximum.accumulate(np.where(Q, pos, 0))          # the first peer
        nextq = np.where(Q, pos, n)                                   # the first Q head BEHIND each position
        nextq = np.minimum.accumulate(np.r_[nextq[1:], n][::-1])[::-1]
        pend = nextq - 1                                              # the last peer
        qcum = np.cumsum(Q)
    else:
        pstart = qstart = pend = qcum = pos
    always = np.ones(n, dtype=bool)
    out = []
    for func, c, rt in outputs:
        if func in RANKING or func == pl.WIN_COUNT_STAR:
            assert c == 0 and rt == pl.INT64
            if func == pl.WIN_ROW_NUMBER:
                v = pos - pstart + 1
            elif func == pl.WIN_RANK:
                v = qstart - pstart + 1
            elif func == pl.WIN_DENSE_RANK:
                v = qcum - qcum[pstart] + 1 if n else pos
            else:
                v = pend - pstart + 1
            out.append((rt, v.astype(np.int64), always))
            continue
        ct, cv, cvalid = cols[c]
        assert rt == result_type(func, ct)
        if func == pl.WIN_COL:
            out.append((ct, np.asarray(cv)[order], np.asarray(cvalid, dtype=bool)[order]))
            continue
        assert ct in NP_OF
        cv, cvalid = np.asarray(cv, dtype=NP_OF[ct])[order], np.asarray(cvalid, dtype=bool)[order]
        cnt = _accumulate(np.add, cvalid.astype(np.int64), starts, n)[pend]
        if func == pl.WIN_COUNT:
            out.append((rt, cnt, always))
        elif func == pl.WIN_SUM:
            assert ct != pl.FP64
            sm = _accumulate(np.add, np.where(cvalid, cv.astype(np.int64), 0).view(np.uint64), starts, n)[pend]
            out.append((rt, np.where(cnt > 0, sm.view(np.int64), 0), cnt > 0))
        else:
            assert func in (pl.WIN_MIN, pl.WIN_MAX)
            _, enc = _sortref.encode(ct, cv, cvalid, 0)
            if func == pl.WIN_MIN:
                r = _accumulate(np.minimum, np.where(cvalid, enc, U64_MAX), starts, n)[pend]
            else:
                r = _accumulate(np.maximum, np.where(cvalid, enc, np.uint64(0)), starts, n)[pend]
            out.append((rt, np.where(cnt > 0, _groupref.decode(ct, r), np.zeros(1, dtype=NP_OF[ct])), cnt > 0))
    return n, out


def outputs_of(node):
    return [(pl.win_func(x), pl.win_col(x), t) for x, t in node.output_attrs]


def children(d):
    if isinstance(d, pl.WindowNode):
        return [("child", d.child)]
    return _groupref.children(d)


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)].  The rows
    of a window node (of a grouping, of a sort) are in ITS order; what another kind makes of them is a
    multiset."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.WindowNode):
        n, child = evaluate(plan, d.child)
        return window(child, d.part_keys, d.order_keys, outputs_of(node), n)
    tmp = pl.Plan()
    moved = {}
    for field, kid in children(d):
        n, cols = evaluate(plan, kid)
        moved[field] = tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)])
        tmp.new_input(_filterref.to_table(n, cols))
    tmp.nodes.append(pl.PlanNode(type(d)(**{**d.__dict__, **moved}), list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _groupref.evaluate(tmp)


to_table = _filterref.to_table
rel_rows = _sortref.rel_rows
decoded_rows = _sortref.decoded_rows


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))
