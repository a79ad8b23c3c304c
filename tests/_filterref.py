"""Plain numpy reference for plans of scans, inner joins, semi joins and anti joins (test
infrastructure for tests/test_gpu_filter_join.py; the C oracle knows inner joins only).

Key rules (include/rj.h, the same as tests/_refjoin.py for the inner join):
  * the key type is the build / filter side's key type; a probe / preserved key of another type
    matches nothing;
  * INT32 / INT64 keys compare by value, FP64 keys by bit pattern, and a NaN matches nothing;
  * NULL keys match nothing — so ANTI keeps preserved rows with a NULL or NaN key, and a NULL on
    the filter side changes nothing (NOT EXISTS, not NOT IN).
SEMI is `np.isin` over the key bit patterns; ANTI its complement.  Not for inputs holding both
-0.0 and +0.0 keys (see _refjoin.py).  A relation is a list of columns (type, values, valid);
VARCHAR values are an object array of bytes (None = NULL)."""
from __future__ import annotations

import numpy as np

import _refjoin
from pyrj import pages as pg
from pyrj import plan as pl


def _scan(plan: pl.Plan, node):
    t = plan.inputs[node.data.base_table_id]
    cols = []
    for idx, dt in node.output_attrs:
        c = t.columns[idx]
        assert c.type == dt
        if dt == pl.VARCHAR:
            vals = np.empty(t.num_rows, dtype=object)
            vals[:] = pg.unpack_varchar(c.pages, t.num_rows)
            cols.append((dt, vals, np.array([v is not None for v in vals], dtype=bool)))
        else:
            v, m = pg.unpack_fixed(c.pages, t.num_rows, dt)
            cols.append((dt, np.asarray(v), np.asarray(m, dtype=bool)))
    return cols


def _take(col, rows):
    return (col[0], col[1][rows], col[2][rows])


def _usable_keys(col):
    """-> (int64 bit patterns, usable mask) of a fixed-width key column."""
    assert col[0] != pl.VARCHAR, "VARCHAR keys are not part of this reference"
    return _refjoin._key_bits(*col)


def filter_rows(filter_key, preserved_key, anti: bool):
    """Row indices of the preserved side that SEMI (anti=False) / ANTI (anti=True) keeps."""
    n = preserved_key[1].shape[0]
    if preserved_key[0] != filter_key[0] or filter_key[1].shape[0] == 0 or n == 0:
        hit = np.zeros(n, dtype=bool)
    else:
        fbits, fok = _usable_keys(filter_key)
        pbits, pok = _usable_keys(preserved_key)
        hit = pok & np.isin(pbits, fbits[fok])
    return np.flatnonzero(~hit if anti else hit)


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)]."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _scan(plan, node)
    (_, left), (_, right) = evaluate(plan, d.left), evaluate(plan, d.right)
    both = left + right
    lw = len(left)
    if isinstance(d, pl.FilterJoinNode):
        fil, pre = (left, right) if d.build_left else (right, left)
        fattr, pattr = (d.left_attr, d.right_attr) if d.build_left else (d.right_attr, d.left_attr)
        rows = filter_rows(fil[fattr], pre[pattr], d.kind == pl.NODE_ANTI)
        out = []
        for i, dt in node.output_attrs:
            assert (i >= lw) == d.build_left, "a semi / anti join outputs preserved columns only"
            assert both[i][0] == dt
            out.append(_take(both[i], rows))
        return int(rows.shape[0]), out
    assert isinstance(d, pl.JoinNode)
    bk, pk = (left[d.left_attr], right[d.right_attr]) if d.build_left else (right[d.right_attr], left[d.left_attr])
    if bk[0] != pk[0] or bk[1].shape[0] == 0 or pk[1].shape[0] == 0:
        brow = prow = np.zeros(0, dtype=np.int64)
    else:
        bbits, bok = _usable_keys(bk)
        pbits, pok = _usable_keys(pk)
        brow, prow = _refjoin.join_indices(bbits, bok, pbits, pok)
    lrow, rrow = (brow, prow) if d.build_left else (prow, brow)
    out = []
    for i, dt in node.output_attrs:
        assert both[i][0] == dt
        out.append(_take(both[i], lrow if i < lw else rrow))
    return int(lrow.shape[0]), out


def to_table(n, rel) -> pl.ColumnarTable:
    cols = []
    for dt, v, m in rel:
        if dt == pl.VARCHAR:
            cols.append((dt, [x if ok else None for x, ok in zip(v, m)]))
        else:
            cols.append((dt, v, m))
    t = pl.make_table(cols)
    t.num_rows = n
    return t


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))
