"""Plain numpy reference for plans that hold set operations (pl.SetOpNode, RJ_NODE_SETOP in include/rj.h),
test infrastructure for tests/test_setop_plan.py and tests/test_gpu_setop.py.

A set operation is computed here.  UNION ALL is the left child's rows followed by the right child's,
bits untouched.  The five other operations put both children's rows one behind the other, order them
with np.lexsort (stable) by the encoded output columns (_sortref.encode, the rules of rj.h: ascending,
NULLs last), cut the order into runs of equal rows, count per run the rows that came from each side and
repeat the run's canonical value (_groupref.canonical) as often as rj.h's table says.  The rows are in
the order of the output columns.

evaluate() handles every node kind, so nested plans can be checked: every other kind goes to
tests/_mapref.py with its children evaluated HERE and handed over as the scans of a temporary plan.
A relation is a list of (type, values, valid) columns as in _filterref."""
from __future__ import annotations

import numpy as np

import _filterref
import _groupref
import _mapref
import _sortref
from pyrj import plan as pl

NP_OF = _sortref.NP_OF
SORTING = (pl.SET_UNION, pl.SET_INTERSECT, pl.SET_INTERSECT_ALL, pl.SET_EXCEPT, pl.SET_EXCEPT_ALL)


def multiplicity(op, l, r):
    """copies of a row value with l copies on the left and r on the right (int64 arrays)"""
    l, r = np.asarray(l, dtype=np.int64), np.asarray(r, dtype=np.int64)
    if op == pl.SET_UNION_ALL:
        return l + r
    if op == pl.SET_UNION:
        return (l + r > 0).astype(np.int64)
    if op == pl.SET_INTERSECT:
        return ((l > 0) & (r > 0)).astype(np.int64)
    if op == pl.SET_INTERSECT_ALL:
        return np.minimum(l, r)
    if op == pl.SET_EXCEPT:
        return ((l > 0) & (r == 0)).astype(np.int64)
    assert op == pl.SET_EXCEPT_ALL, op
    return np.maximum(l - r, 0)


def _concat(a, b):
    """one column of both sides: VARCHAR values are Python objects, everything else numpy of the type"""
    dt = a[0]
    assert dt == b[0], "the two columns of a pair differ in type"
    valid = np.r_[np.asarray(a[2], dtype=bool), np.asarray(b[2], dtype=bool)]
    if dt == pl.VARCHAR:
        vals = np.empty(valid.shape[0], dtype=object)
        vals[:] = list(a[1]) + list(b[1])
        return dt, vals, valid
    return dt, np.r_[np.asarray(a[1], dtype=NP_OF[dt]), np.asarray(b[1], dtype=NP_OF[dt])], valid


def setop(op, lcols, ln, rcols, rn, outputs):
    """outputs: [(left column, right column, type)] -> (rows, columns)"""
    assert 0 <= op <= pl.SET_EXCEPT_ALL and outputs
    cols = []
    for lc, rc, dt in outputs:
        assert lcols[lc][0] == dt == rcols[rc][0], "declared type differs from the paired columns' type"
        cols.append(_concat(lcols[lc], rcols[rc]))
    n = ln + rn
    if op == pl.SET_UNION_ALL:
        return n, cols
    assert all(c[0] in NP_OF for c in cols), "a VARCHAR pair in a sorting operation"
    order = _sortref.order(cols, [(c, 0) for c in range(len(cols))]) if n else np.zeros(0, dtype=np.int64)
    head = np.zeros(n, dtype=bool)
    if n:
        head[0] = True
    for dt, v, valid in cols:
        nd, key = _sortref.encode(dt, v, valid, 0)
        nd, key = nd[order], key[order]
        head[1:] |= (nd[1:] != nd[:-1]) | (key[1:] != key[:-1])
    starts = np.flatnonzero(head)
    if n:
        rows = np.diff(np.r_[starts, n]).astype(np.int64)
        left = np.add.reduceat((order < ln).astype(np.int64), starts)
    else:
        rows = left = np.zeros(0, dtype=np.int64)
    take = np.repeat(starts, multiplicity(op, left, rows - left))  # positions of the order: a run's first row
    out = []
    for dt, v, valid in cols:
        v, valid = v[order][take], valid[order][take]
        out.append((dt, _groupref.canonical(dt, v, valid), valid))
    return int(take.shape[0]), out


def outputs_of(node):
    return [(pl.setop_lcol(x), pl.setop_rcol(x), t) for x, t in node.output_attrs]


def children(d):
    if isinstance(d, pl.SetOpNode):
        return [("left", d.left), ("right", d.right)]
    return _mapref.children(d)


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)].  The rows
    of a set operation are in ITS order; what another kind makes of them is that kind's business."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.SetOpNode):
        ln, lcols = evaluate(plan, d.left)
        rn, rcols = evaluate(plan, d.right)
        return setop(d.op, lcols, ln, rcols, rn, outputs_of(node))
    tmp = pl.Plan()
    moved = {}
    for field, kid in children(d):
        n, cols = evaluate(plan, kid)
        moved[field] = tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)])
        tmp.new_input(_filterref.to_table(n, cols))
    tmp.nodes.append(pl.PlanNode(type(d)(**{**d.__dict__, **moved}), list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _mapref.evaluate(tmp)


to_table = _filterref.to_table
rel_rows = _sortref.rel_rows
decoded_rows = _sortref.decoded_rows


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))
