"""A second, independent reference for plans of all six node kinds plus scans: one row at a time, in
plain Python (dicts, lists, None for NULL), written from the semantics text of include/rj.h alone.
It shares no code with the numpy references (_refjoin, _filterref, _outerref, _fullref, _aggref);
tests/test_mixed_plan_ref.py holds the two against each other on generated plans.

The rules, as rj.h states them:
  * the key type of a binary node is the BUILT side's; when the other side's key column has another
    type nothing matches: inner and semi give 0 rows, anti every preserved row, outer every
    preserved row padded, full every row of both children padded;
  * INT32 / INT64 keys compare by value, FP64 keys by bit pattern, and a NaN matches nothing;
  * NULL keys match nothing, on either side; ANTI, OUTER and FULL keep such rows as unmatched ones;
  * SEMI emits a preserved row once however many partners it has; duplicates multiply in the others;
  * AGG: one row per distinct key, the rows with a NULL key form one group whose key is NULL; COUNT
    counts non-NULL values; SUM wraps modulo 2^64; SUM / MIN / MAX of a group without a non-NULL
    value are NULL; an empty child gives 0 rows.
A relation is (column types, list of row tuples)."""
from __future__ import annotations

import struct

from pyrj import plan as pl


def _usable(v, dt):
    """The value a key is looked up by, or None when it can match nothing."""
    if v is None:
        return None
    if dt == pl.FP64:
        return None if v != v else struct.pack("<d", v)
    return v


def _binary(kind, build_left, left, right, la, ra, outs):
    (lt, lrows), (rt, rrows) = left, right
    (bt, brows, ba), (pt, prows, pa) = ((lt, lrows, la), (rt, rrows, ra)) if build_left else ((rt, rrows, ra), (lt, lrows, la))
    kt = bt[ba]
    table = {}
    if pt[pa] == kt:  # otherwise no key of the probed side is of the key type
        for b, row in enumerate(brows):
            k = _usable(row[ba], kt)
            if k is not None:
                table.setdefault(k, []).append(b)
    hit = [False] * len(brows)
    pairs = []  # (built row or None, probed row or None)
    for row in prows:
        k = _usable(row[pa], kt)
        partners = table.get(k) if k is not None else None
        if partners:
            if kind == "semi":
                pairs.append((None, row))
            elif kind != "anti":
                for b in partners:
                    hit[b] = True
                    pairs.append((brows[b], row))
        elif kind in ("anti", "outer", "full"):
            pairs.append((None, row))
    if kind == "full":
        pairs += [(brows[b], None) for b in range(len(brows)) if not hit[b]]
    lnull, rnull = (None,) * len(lt), (None,) * len(rt)
    rows = []
    for b, p in pairs:
        l, r = (b, p) if build_left else (p, b)
        cat = (lnull if l is None else l) + (rnull if r is None else r)
        rows.append(tuple(cat[i] for i in outs))
    both = lt + rt
    return [both[i] for i in outs], rows


def _wrap64(x):
    return (x + 2**63) % 2**64 - 2**63


def _agg(child, key, outs):
    """outs: [(func, column, result type)]"""
    _, rows = child
    groups = {}  # key (None = the NULL group) -> rows
    for row in rows:
        groups.setdefault(row[key], []).append(row)
    res = []
    for k, grp in groups.items():
        out = []
        for func, c, _ in outs:
            vals = [r[c] for r in grp if r[c] is not None] if func >= pl.AGG_COUNT else None
            if func == pl.AGG_KEY:
                out.append(k)
            elif func == pl.AGG_COUNT_STAR:
                out.append(len(grp))
            elif func == pl.AGG_COUNT:
                out.append(len(vals))
            elif func == pl.AGG_SUM:
                out.append(_wrap64(sum(vals)) if vals else None)
            elif func == pl.AGG_MIN:
                out.append(min(vals) if vals else None)
            else:
                assert func == pl.AGG_MAX
                out.append(max(vals) if vals else None)
        res.append(tuple(out))
    return [t for _, _, t in outs], res


def evaluate(plan: pl.Plan, idx=None):
    """-> (column types, rows) of node idx (default: the root)."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        t = plan.inputs[d.base_table_id]
        base = pl.table_rows(t)
        cols = [i for i, _ in node.output_attrs]
        return [t.columns[i].type for i in cols], [tuple(r[i] for i in cols) for r in base]
    if isinstance(d, pl.AggNode):
        return _agg(evaluate(plan, d.child), d.key_attr, [(pl.agg_func(x), pl.agg_col(x), t) for x, t in node.output_attrs])
    if isinstance(d, pl.FilterJoinNode):
        kind = "semi" if d.kind == pl.NODE_SEMI else "anti"
    else:
        kind = {pl.JoinNode: "join", pl.OuterJoinNode: "outer", pl.FullOuterJoinNode: "full"}[type(d)]
    types, rows = _binary(kind, d.build_left, evaluate(plan, d.left), evaluate(plan, d.right), d.left_attr, d.right_attr,
                          [i for i, _ in node.output_attrs])
    assert types == [t for _, t in node.output_attrs], "declared types differ from the children's"
    return types, rows


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    types, rows = evaluate(plan)
    return pl.table_from_rows(rows, types)
