"""Reference for RJ_AGG_FSUM (include/rj.h, RJ_NODE_GROUP), test infrastructure for
tests/test_fsum_plan.py and tests/test_gpu_fsum.py.

Every finite double is a Python integer in units of 2^-1074; a run of values is summed as integers and
rounded by float(Fraction(total, 2**1074)), OverflowError giving +-inf: the rounding is Python's, not a
restatement of the library's.  The rules for NaN, the infinities and a zero sum stand in front of it.
Everything except the FSUM outputs of a grouping is tests/_groupref.py's, and every other node kind goes
down the chain of references (tests/_setopref.py) with its children evaluated HERE."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import _filterref
import _groupref
import _setopref
import _sortref
from pyrj import plan as pl

UNIT = 2**1074
CANON_NAN = 0x7FF8000000000000
PINF, NINF = 0x7FF0000000000000, 0xFFF0000000000000


def units(bits: int) -> int:
    """a finite double's value in units of 2^-1074"""
    e, m = (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1)
    assert e != 0x7FF
    v = (m | 1 << 52) << (e - 1) if e else m
    return -v if bits >> 63 else v


def round_units(total: int) -> int:
    """the bits of `total` units rounded to nearest even as Python rounds a Fraction; a zero is +0.0"""
    if total == 0:
        return 0
    try:
        x = float(Fraction(total, UNIT))
    except OverflowError:
        x = math.inf if total > 0 else -math.inf
    return int(np.float64(x).view(np.uint64))


def fsum_bits(bits, valid=None):
    """FSUM of one group: the values' bits (and validity) -> the result's bits, None = NULL"""
    bits = [int(b) for b in np.asarray(bits, dtype=np.uint64)]
    if valid is not None:
        bits = [b for b, ok in zip(bits, np.asarray(valid, dtype=bool)) if ok]
    if not bits:
        return None
    fin = [b for b in bits if (b >> 52) & 0x7FF != 0x7FF]
    special = [b for b in bits if (b >> 52) & 0x7FF == 0x7FF]
    nan = any(b & ((1 << 52) - 1) for b in special)
    pinf, ninf = PINF in special, NINF in special
    if nan or (pinf and ninf):
        return CANON_NAN
    if pinf or ninf:
        return PINF if pinf else NINF
    return round_units(sum(units(b) for b in fin))


def group(cols, keys, outputs, n=None):
    """_groupref.group with FSUM outputs: (func, column, result type) -> (rows, columns)"""
    n = (cols[0][1].shape[0] if cols else 0) if n is None else n
    rest = [o for o in outputs if o[0] != pl.AGG_FSUM]
    ng, rest_cols = _groupref.group(cols, keys, rest, n)
    if len(rest) == len(outputs):
        return ng, rest_cols
    keys = [tuple(k) for k in keys]
    if keys:   # the runs, as _groupref.group finds them
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
        order, starts = np.arange(n), np.zeros(1, dtype=np.int64)
    assert starts.shape[0] == ng
    ends = np.r_[starts[1:], n]
    sums = {}
    for func, c, rt in outputs:
        if func != pl.AGG_FSUM or c in sums:
            continue
        ct, cv, cvalid = cols[c]
        assert ct == pl.FP64 and rt == pl.FP64
        b = np.asarray(cv, dtype=np.float64).view(np.uint64)[order]
        ok = np.asarray(cvalid, dtype=bool)[order]
        res = [fsum_bits(b[s:e], ok[s:e]) for s, e in zip(starts, ends)]
        vals = np.array([0 if r is None else r for r in res], dtype=np.uint64).view(np.float64)
        sums[c] = (pl.FP64, vals, np.array([r is not None for r in res], dtype=bool))
    it = iter(rest_cols)
    return ng, [sums[o[1]] if o[0] == pl.AGG_FSUM else next(it) for o in outputs]


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)]"""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.GroupNode):
        n, child = evaluate(plan, d.child)
        return group(child, d.keys, _groupref.outputs_of(node), n)
    tmp = pl.Plan()
    moved = {}
    for field, kid in _setopref.children(d):
        n, cols = evaluate(plan, kid)
        moved[field] = tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)])
        tmp.new_input(_filterref.to_table(n, cols))
    tmp.nodes.append(pl.PlanNode(type(d)(**{**d.__dict__, **moved}), list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _setopref.evaluate(tmp)


to_table = _filterref.to_table
rel_rows = _sortref.rel_rows
decoded_rows = _sortref.decoded_rows
