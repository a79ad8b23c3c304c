"""Plain numpy reference for plans of scans and all four join kinds: inner, semi, anti and outer
(test infrastructure for tests/test_outer_join_plan.py and tests/test_gpu_outer_join.py; the C
oracle knows inner joins only).

An outer join (pl.OuterJoinNode, include/rj.h) is put together from the two references that exist:
  * its matched rows are the inner join's pairs: _refjoin.join_indices over the key bit patterns
    (NULL and NaN keys dropped, duplicates multiply);
  * its padded rows are the preserved rows ANTI keeps: _filterref.filter_rows(..., anti=True),
    with every optional-side column NULL (valid = False, value 0 / None).
The key type is the optional (build) side's; a preserved key of another type matches nothing.
Results are compared as multisets of rows in which NULL is a value of its own and FP64 goes by
bit pattern: same() below (pl.table_digest, or pl.canonical_rows when a VARCHAR column is there).
A relation is a list of columns (type, values, valid) as in _filterref."""
from __future__ import annotations

import numpy as np

import _filterref
import _refjoin
from pyrj import plan as pl


def _null_column(dt, n):
    if dt == pl.VARCHAR:
        return (dt, np.full(n, None, dtype=object), np.zeros(n, dtype=bool))
    np_dt = {pl.INT32: np.int32, pl.INT64: np.int64, pl.FP64: np.float64}[dt]
    return (dt, np.zeros(n, dtype=np_dt), np.zeros(n, dtype=bool))


def _concat(a, b):
    return (a[0], np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]))


def inner_pairs(build_key, probe_key):
    """-> (build rows, probe rows) of the inner join's pairs."""
    if build_key[0] != probe_key[0] or build_key[1].shape[0] == 0 or probe_key[1].shape[0] == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    bbits, bok = _filterref._usable_keys(build_key)
    pbits, pok = _filterref._usable_keys(probe_key)
    return _refjoin.join_indices(bbits, bok, pbits, pok)


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
        return int(rows.shape[0]), [_filterref._take(both[i], rows) for i, _ in node.output_attrs]
    brow, prow = inner_pairs(bld[battr], prb[pattr])
    if isinstance(d, pl.JoinNode):
        if bld[battr][1].shape[0] == 0 or prb[pattr][1].shape[0] == 0:
            brow = prow = np.zeros(0, dtype=np.int64)
        lrow, rrow = (brow, prow) if d.build_left else (prow, brow)
        return int(lrow.shape[0]), [_filterref._take(both[i], lrow if i < lw else rrow) for i, _ in node.output_attrs]
    assert isinstance(d, pl.OuterJoinNode)
    lone = _filterref.filter_rows(bld[battr], prb[pattr], anti=True)  # preserved rows without a partner
    out = []
    for i, dt in node.output_attrs:
        optional = (i < lw) == d.build_left
        if optional:
            out.append(_concat(_filterref._take(both[i], brow), _null_column(dt, lone.shape[0])))
        else:
            out.append(_concat(_filterref._take(both[i], prow), _filterref._take(both[i], lone)))
    return int(prow.shape[0] + lone.shape[0]), out


def split_outer(plan: pl.Plan):
    """The root must be an outer join: -> (matched rows, padded rows) as two (rows, columns)
    relations in the root's output layout (the padded rows' optional columns are NULL)."""
    node = plan.nodes[plan.root]
    d = node.data
    assert isinstance(d, pl.OuterJoinNode)
    n, cols = evaluate(plan)
    (_, left), (_, right) = evaluate(plan, d.left), evaluate(plan, d.right)
    bld, prb = (left, right) if d.build_left else (right, left)
    battr, pattr = (d.left_attr, d.right_attr) if d.build_left else (d.right_attr, d.left_attr)
    m = inner_pairs(bld[battr], prb[pattr])[0].shape[0]
    head, tail = np.arange(m), np.arange(m, n)
    return (m, [_filterref._take(c, head) for c in cols]), (n - m, [_filterref._take(c, tail) for c in cols])


to_table = _filterref.to_table


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))


def same(got: pl.ColumnarTable, want: pl.ColumnarTable, what=""):
    """Multiset equality of two result tables, NULL as its own value, FP64 by bit pattern."""
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    if any(c.type == pl.VARCHAR for c in want.columns):
        assert pl.canonical_rows(got) == pl.canonical_rows(want), what
    elif want.columns:
        assert pl.table_digest(got) == pl.table_digest(want), what
