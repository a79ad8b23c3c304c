"""Plain numpy reference for plans of scans and all five join kinds: inner, semi, anti, outer and
full outer (test infrastructure for tests/test_full_outer_join_plan.py and
tests/test_gpu_full_outer_join.py; _outerref.evaluate does not know the full outer node).

A full outer join (pl.FullOuterJoinNode, include/rj.h) is put together from functions that are
pinned elsewhere:
  1. its matched rows are the inner join's pairs: _outerref.inner_pairs(built key, probed key);
  2. the probed rows without a partner: _filterref.filter_rows(built key, probed key, anti=True),
     with every column of the built child NULL;
  3. the built rows without a partner: _filterref.filter_rows(probed key, built key, anti=True),
     with every column of the probed child NULL.
Every other node kind is evaluated as _outerref does, by this file's own recursion (a child may be
a full outer join).  A relation is a list of columns (type, values, valid) as in _filterref."""
from __future__ import annotations

import numpy as np

import _filterref
import _outerref
from pyrj import plan as pl

_take, _concat, _null = _filterref._take, _outerref._concat, _outerref._null_column


def full_parts(bld_key, prb_key):
    """-> (built rows, probed rows) of the pairs, lone probed rows, lone built rows."""
    brow, prow = _outerref.inner_pairs(bld_key, prb_key)
    lone_p = _filterref.filter_rows(bld_key, prb_key, anti=True)
    lone_b = _filterref.filter_rows(prb_key, bld_key, anti=True)
    return brow, prow, lone_p, lone_b


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)]."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    (_, left), (_, right) = evaluate(plan, d.left), evaluate(plan, d.right)
    both = left + right
    lw = len(left)
    bld, prb = (left, right) if d.build_left else (right, left)
    battr, pattr = (d.left_attr, d.right_attr) if d.build_left else (d.right_attr, d.left_attr)
    for i, dt in node.output_attrs:
        assert both[i][0] == dt
    if isinstance(d, pl.FilterJoinNode):
        rows = _filterref.filter_rows(bld[battr], prb[pattr], d.kind == pl.NODE_ANTI)
        for i, _ in node.output_attrs:
            assert (i >= lw) == d.build_left, "a semi / anti join outputs preserved columns only"
        return int(rows.shape[0]), [_take(both[i], rows) for i, _ in node.output_attrs]
    brow, prow, lone_p, lone_b = full_parts(bld[battr], prb[pattr])
    if isinstance(d, pl.JoinNode):
        lrow, rrow = (brow, prow) if d.build_left else (prow, brow)
        return int(lrow.shape[0]), [_take(both[i], lrow if i < lw else rrow) for i, _ in node.output_attrs]
    out = []
    if isinstance(d, pl.OuterJoinNode):
        for i, dt in node.output_attrs:
            if (i < lw) == d.build_left:
                out.append(_concat(_take(both[i], brow), _null(dt, lone_p.shape[0])))
            else:
                out.append(_concat(_take(both[i], prow), _take(both[i], lone_p)))
        return int(prow.shape[0] + lone_p.shape[0]), out
    assert isinstance(d, pl.FullOuterJoinNode)
    for i, dt in node.output_attrs:
        if (i < lw) == d.build_left:  # a column of the built child
            parts = [_take(both[i], brow), _null(dt, lone_p.shape[0]), _take(both[i], lone_b)]
        else:
            parts = [_take(both[i], prow), _take(both[i], lone_p), _null(dt, lone_b.shape[0])]
        out.append(_concat(_concat(parts[0], parts[1]), parts[2]))
    return int(prow.shape[0] + lone_p.shape[0] + lone_b.shape[0]), out


def split_full(plan: pl.Plan):
    """The root must be a full outer join: -> three (rows, columns) relations in the root's output
    layout: the pairs, the rows padded on the built side, the rows padded on the probed side."""
    node = plan.nodes[plan.root]
    d = node.data
    assert isinstance(d, pl.FullOuterJoinNode)
    n, cols = evaluate(plan)
    (_, left), (_, right) = evaluate(plan, d.left), evaluate(plan, d.right)
    bld, prb = (left, right) if d.build_left else (right, left)
    battr, pattr = (d.left_attr, d.right_attr) if d.build_left else (d.right_attr, d.left_attr)
    brow, _, lone_p, lone_b = full_parts(bld[battr], prb[pattr])
    m, u, v = brow.shape[0], lone_p.shape[0], lone_b.shape[0]
    assert n == m + u + v
    cut = lambda a, b: (b - a, [_take(c, np.arange(a, b)) for c in cols])
    return cut(0, m), cut(m, m + u), cut(m + u, n)


to_table = _filterref.to_table
same = _outerref.same


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))
