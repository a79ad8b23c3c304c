"""Plain numpy reference for plans that hold aggregation nodes (pl.AggNode, RJ_NODE_AGG in
include/rj.h), test infrastructure for tests/test_agg_plan.py and tests/test_gpu_agg.py.

evaluate() handles every node kind, so nested plans can be checked: a scan and the five join kinds
go to tests/_fullref.py (the children's results are handed to it as the inputs of a two-scan plan),
an aggregation is computed here: the rows are sorted by group, every function is a reduceat over the
groups.  NULL keys form one group whose key is NULL; SUM wraps modulo 2^64; SUM / MIN / MAX of a
group without a non-NULL value are NULL.  A relation is a list of (type, values, valid) columns as
in _filterref."""
from __future__ import annotations

import numpy as np

import _filterref
import _fullref
from pyrj import plan as pl

NP_OF = {pl.INT32: np.int32, pl.INT64: np.int64}
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def result_type(func, col_type, key_type):
    if func == pl.AGG_KEY:
        return key_type
    if func in (pl.AGG_MIN, pl.AGG_MAX):
        return col_type
    return pl.INT64


def aggregate(cols, key_attr, outputs):
    """cols: the child's columns; outputs: [(func, column, result type)] -> (rows, columns)."""
    kt, kv, kval = cols[key_attr]
    assert kt in NP_OF, "group keys are INT32 or INT64"
    kv, kval = np.asarray(kv), np.asarray(kval, dtype=bool)
    n = kv.shape[0]
    uniq, inv = np.unique(kv[kval], return_inverse=True)
    has_null = bool((~kval).any())
    ng = uniq.shape[0] + int(has_null)
    gid = np.full(n, uniq.shape[0], dtype=np.int64)
    gid[kval] = inv
    order = np.argsort(gid, kind="stable")
    sg = gid[order]
    starts = np.flatnonzero(np.r_[True, sg[1:] != sg[:-1]]) if n else np.zeros(0, dtype=np.int64)
    assert starts.shape[0] == ng
    out = []
    for func, c, rt in outputs:
        if func == pl.AGG_KEY:
            assert c == key_attr and rt == kt
            vals = np.concatenate([uniq, np.zeros(int(has_null), dtype=uniq.dtype)]).astype(NP_OF[kt])
            valid = np.concatenate([np.ones(uniq.shape[0], dtype=bool), np.zeros(int(has_null), dtype=bool)])
            out.append((rt, vals, valid))
            continue
        if func == pl.AGG_COUNT_STAR:
            assert c == 0 and rt == pl.INT64
            out.append((rt, np.diff(np.r_[starts, n]).astype(np.int64), np.ones(ng, dtype=bool)))
            continue
        ct, cv, cvalid = cols[c]
        assert ct in NP_OF and rt == result_type(func, ct, kt)
        cv, cvalid = np.asarray(cv).astype(np.int64)[order], np.asarray(cvalid, dtype=bool)[order]
        cnt = np.add.reduceat(cvalid.astype(np.int64), starts) if ng else np.zeros(0, dtype=np.int64)
        if func == pl.AGG_COUNT:
            out.append((rt, cnt, np.ones(ng, dtype=bool)))
        elif func == pl.AGG_SUM:
            with np.errstate(over="ignore"):
                sm = np.add.reduceat(np.where(cvalid, cv, 0).view(np.uint64), starts) if ng else np.zeros(0, dtype=np.uint64)
            out.append((rt, np.where(cnt > 0, sm.view(np.int64), 0), cnt > 0))
        else:
            assert func in (pl.AGG_MIN, pl.AGG_MAX)
            if func == pl.AGG_MIN:
                r = np.minimum.reduceat(np.where(cvalid, cv, I64_MAX), starts) if ng else np.zeros(0, dtype=np.int64)
            else:
                r = np.maximum.reduceat(np.where(cvalid, cv, I64_MIN), starts) if ng else np.zeros(0, dtype=np.int64)
            out.append((rt, np.where(cnt > 0, r, 0).astype(NP_OF[ct]), cnt > 0))
    return ng, out


def outputs_of(node):
    return [(pl.agg_func(x), pl.agg_col(x), t) for x, t in node.output_attrs]


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)]."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.AggNode):
        _, child = evaluate(plan, d.child)
        return aggregate(child, d.key_attr, outputs_of(node))
    # a join of any kind: the children's results become the inputs of a plan _fullref knows
    tmp = pl.Plan()
    kids = []
    for side in (d.left, d.right):
        n, cols = evaluate(plan, side)
        kids.append(tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)]))
        tmp.new_input(_filterref.to_table(n, cols))
    dd = type(d)(**{**d.__dict__, "left": kids[0], "right": kids[1]})
    tmp.nodes.append(pl.PlanNode(dd, list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _fullref.evaluate(tmp)


to_table = _filterref.to_table
same = _fullref.same


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))
