"""Plain numpy reference for plans that hold grouping nodes (pl.GroupNode, RJ_NODE_GROUP in
include/rj.h), test infrastructure for tests/test_group_plan.py and tests/test_gpu_group.py.

A grouping is computed here: np.lexsort (stable) orders the child's rows by the encoded keys
(_sortref.encode, the rules of rj.h), a row starts a group where any (NULL digit, key) pair differs
from the row before it, and every function is a reduceat over the runs.  MIN / MAX reduce the ENCODED
value as an unsigned number and decode it again, so that FP64 follows the same order (a NaN above
+inf) and comes back canonical; key columns come back canonical too (+0.0 for a zero, one NaN).  The
groups are in the order of the keys.  Without keys there is ONE group, also over no rows.

evaluate() handles every node kind, so nested plans can be checked: every other kind goes to
tests/_sortref.py with its children evaluated HERE and handed over as the scans of a temporary plan.
A relation is a list of (type, values, valid) columns as in _filterref."""
from __future__ import annotations

import numpy as np

import _filterref
import _sortref
from pyrj import plan as pl

NP_OF = _sortref.NP_OF
_TOP = np.uint64(1 << 63)
U64_MAX = np.uint64(2**64 - 1)


def decode(dt, key):
    """the inverse of _sortref.encode(dt, ., ., flags=0) for non-NULL keys -> values of the column's type"""
    key = np.asarray(key, dtype=np.uint64)
    if dt == pl.INT32:
        return (key.astype(np.int64) - 2**31).astype(np.int32)
    if dt == pl.INT64:
        return (key ^ _TOP).view(np.int64)
    return np.where(key >> np.uint64(63) != 0, key ^ _TOP, ~key).view(np.float64)


def canonical(dt, vals, valid):
    """what a key column holds: the decoding of the encoded key, 0 where NULL"""
    _, key = _sortref.encode(dt, vals, valid, 0)
    return np.where(valid, decode(dt, key), np.zeros(1, dtype=NP_OF[dt]))


def result_type(func, col_type):
    if func in (pl.AGG_KEY, pl.AGG_MIN, pl.AGG_MAX):
        return col_type
    return pl.INT64


def group(cols, keys, outputs, n=None):
    """cols: the child's columns; keys: [(column, flags)]; outputs: [(func, column, result type)]
    -> (rows, columns), the groups in the order of the keys."""
    n = (cols[0][1].shape[0] if cols else 0) if n is None else n
    keys = [tuple(k) for k in keys]
    if keys:
        order = _sortref.order(cols, keys)
        head = np.zeros(n, dtype=bool)
        if n:
            head[0] = True
        for c, flags in keys:
            nd, key = _sortref.encode(cols[c][0], cols[c][1], cols[c][2], flags)
            nd, key = nd[order], key[order]
            head[1:] |= (nd[1:] != nd[:-1]) | (key[1:] != key[:-1])
        starts = np.flatnonzero(head)
    else:
        order = np.arange(n)
        starts = np.zeros(1, dtype=np.int64)    # ONE group, whatever the child holds
    ng = starts.shape[0]
    sizes = np.diff(np.r_[starts, n]).astype(np.int64) if ng else np.zeros(0, dtype=np.int64)

    def reduce(ufunc, arr, empty):
        if n == 0:
            return np.full(ng, empty, dtype=arr.dtype)
        return ufunc.reduceat(arr, starts)

    key_cols = {c for c, _ in keys}
    out = []
    for func, c, rt in outputs:
        if func == pl.AGG_COUNT_STAR:
            assert c == 0 and rt == pl.INT64
            out.append((rt, sizes, np.ones(ng, dtype=bool)))
            continue
        ct, cv, cvalid = cols[c]
        assert ct in NP_OF and rt == result_type(func, ct)
        cv, cvalid = np.asarray(cv, dtype=NP_OF[ct])[order], np.asarray(cvalid, dtype=bool)[order]
        if func == pl.AGG_KEY:
            assert c in key_cols
            first = starts if n else np.zeros(0, dtype=np.int64)
            out.append((rt, canonical(ct, cv[first], cvalid[first]), cvalid[first]))
            continue
        cnt = reduce(np.add, cvalid.astype(np.int64), 0)
        if func == pl.AGG_COUNT:
            out.append((rt, cnt, np.ones(ng, dtype=bool)))
        elif func == pl.AGG_SUM:
            assert ct != pl.FP64
            with np.errstate(over="ignore"):
                sm = reduce(np.add, np.where(cvalid, cv.astype(np.int64), 0).view(np.uint64), 0)
            out.append((rt, np.where(cnt > 0, sm.view(np.int64), 0), cnt > 0))
        else:
            assert func in (pl.AGG_MIN, pl.AGG_MAX)
            _, enc = _sortref.encode(ct, cv, cvalid, 0)
            if func == pl.AGG_MIN:
                r = reduce(np.minimum, np.where(cvalid, enc, U64_MAX), U64_MAX)
            else:
                r = reduce(np.maximum, np.where(cvalid, enc, np.uint64(0)), np.uint64(0))
            out.append((rt, np.where(cnt > 0, decode(ct, r), np.zeros(1, dtype=NP_OF[ct])), cnt > 0))
    return ng, out


def outputs_of(node):
    return [(pl.agg_func(x), pl.agg_col(x), t) for x, t in node.output_attrs]


def children(d):
    if isinstance(d, pl.ScanNode):
        return []
    if isinstance(d, (pl.AggNode, pl.SelectNode, pl.SortNode, pl.GroupNode)):
        return [("child", d.child)]
    return [("left", d.left), ("right", d.right)]


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)].  The rows
    of a grouping (and of a sort) are in ITS order; what another kind makes of them is a multiset."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.GroupNode):
        n, child = evaluate(plan, d.child)
        return group(child, d.keys, outputs_of(node), n)
    tmp = pl.Plan()
    moved = {}
    for field, kid in children(d):
        n, cols = evaluate(plan, kid)
        moved[field] = tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)])
        tmp.new_input(_filterref.to_table(n, cols))
    tmp.nodes.append(pl.PlanNode(type(d)(**{**d.__dict__, **moved}), list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _sortref.evaluate(tmp)


to_table = _filterref.to_table
rel_rows = _sortref.rel_rows
decoded_rows = _sortref.decoded_rows


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))
