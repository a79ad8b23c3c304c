"""Plain numpy reference for ONE equi-join over fixed-width columns (test infrastructure).

For inputs where the oracle is too slow: the oracle restates the reference's hash table, whose
chains grow quadratically when many 64-bit keys share low fmix64 bits — exactly what the
hash-adversarial tests construct.  Here the join is a sort + searchsorted over the key bit patterns:
  * NULL keys drop out on both sides;
  * duplicates on either side multiply;
  * FP64 keys compare by bit pattern and a NaN matches nothing (the device's documented rule,
    csrc/rj_partition.hip hash_keys).  Not for inputs holding both -0.0 and +0.0 keys: the
    reference lets those meet by accident of probing.
The plan is Scan(0) JOIN Scan(1) in either order, with scans selecting columns of the inputs and
the join's output list indexing left outputs ++ right outputs, as in the reference (plan.h)."""
from __future__ import annotations

import numpy as np

from pyrj import hashing as hs
from pyrj import pages as pg
from pyrj import plan as pl


def _scan(plan: pl.Plan, node):
    t = plan.inputs[node.data.base_table_id]
    cols = []
    for idx, dt in node.output_attrs:
        c = t.columns[idx]
        assert c.type == dt and dt != pl.VARCHAR, "fixed-width columns only"
        v, m = pg.unpack_fixed(c.pages, t.num_rows, dt)
        cols.append((dt, v, m))
    return cols


def _key_bits(dt, v, m):
    """-> (int64 key bit patterns, usable mask): NULL and NaN keys are not usable."""
    if dt == pl.FP64:
        bits = np.ascontiguousarray(v).view(np.int64)
        return bits, m & ~hs.is_nan_bits(bits.view(np.uint64))
    return v.astype(np.int64), m.copy()


def join_indices(bkeys, bvalid, pkeys, pvalid):
    """-> (build row, probe row) of every matching pair (any order)."""
    bi = np.flatnonzero(bvalid)
    order = bi[np.argsort(bkeys[bi], kind="stable")]
    bs = bkeys[order]
    pi = np.flatnonzero(pvalid)
    lo = np.searchsorted(bs, pkeys[pi], side="left")
    hi = np.searchsorted(bs, pkeys[pi], side="right")
    cnt = hi - lo
    prow = np.repeat(pi, cnt)
    # position inside each probe row's run of equal build keys
    starts = np.repeat(lo, cnt)
    within = np.arange(prow.shape[0]) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    brow = order[starts + within]
    return brow, prow


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    root = plan.nodes[plan.root]
    j = root.data
    assert isinstance(j, pl.JoinNode), "the root must be a join"
    left, right = plan.nodes[j.left], plan.nodes[j.right]
    assert isinstance(left.data, pl.ScanNode) and isinstance(right.data, pl.ScanNode), "a join of two scans"
    lcols, rcols = _scan(plan, left), _scan(plan, right)
    lk = lcols[j.left_attr]
    rk = rcols[j.right_attr]
    assert lk[0] == rk[0], "both keys of one type"
    lbits, lok = _key_bits(*lk)
    rbits, rok = _key_bits(*rk)
    if j.build_left:
        lrow, rrow = join_indices(lbits, lok, rbits, rok)
    else:
        rrow, lrow = join_indices(rbits, rok, lbits, lok)
    cols = lcols + rcols
    out = []
    for idx, dt in root.output_attrs:
        c = cols[idx]
        rows = lrow if idx < len(lcols) else rrow
        assert c[0] == dt
        out.append((dt, c[1][rows], c[2][rows]))
    t = pl.make_table(out)
    t.num_rows = int(lrow.shape[0])
    return t
