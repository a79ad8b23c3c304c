"""Plain numpy reference for plans that hold sort nodes (pl.SortNode, RJ_NODE_SORT in include/rj.h),
test infrastructure for tests/test_sort_plan.py and tests/test_gpu_sort.py.

A sort is computed here: every key column is encoded in numpy into (NULL digit, unsigned key) by the
rules of rj.h (encode), np.lexsort — which is stable — orders the child's rows by them, the slice
[offset, offset + limit) is cut and the named columns are taken (sort).  evaluate() handles every node
kind, so nested plans can be checked: a selection goes to _selectref.select, every other kind to
tests/_aggref.py with its children evaluated HERE and handed over as the scans of a temporary plan
(what _selectref.evaluate does).  A relation is a list of (type, values, valid) columns as in
_filterref.

same_sorted() is the comparison of a device result with the child's rows that knows what the node
promises about ties (rj.h, "Ties").  tests/test_sort_plan.py pins encode / sort against a row-at-a-time
comparator written from the prose and shows same_sorted rejecting what it must."""
from __future__ import annotations

from collections import Counter

import numpy as np

import _aggref
import _filterref
import _selectref
from pyrj import plan as pl

NP_OF = {pl.INT32: np.int32, pl.INT64: np.int64, pl.FP64: np.float64}
DESC, NULLS_FIRST = pl.SORT_DESC, pl.SORT_NULLS_FIRST
_TOP = np.uint64(1 << 63)


def encode(dt, vals, valid, flags):
    """-> (null digit uint8[n], key uint64[n]): row a sorts before row b iff its pair is the smaller."""
    assert dt in NP_OF, "sort keys are INT32 / INT64 / FP64 columns"
    valid = np.asarray(valid, dtype=bool)
    v = np.asarray(vals, dtype=NP_OF[dt])
    if dt == pl.INT32:
        key = (v.astype(np.int64) + 2**31).astype(np.uint64)
        width = np.uint64(2**32 - 1)
    elif dt == pl.INT64:
        key = v.view(np.uint64) ^ _TOP
        width = np.uint64(2**64 - 1)
    else:
        bits = np.ascontiguousarray(v).view(np.uint64).copy()
        bits[np.isnan(v)] = np.uint64(0x7FF8000000000000)
        bits[v == 0] = np.uint64(0)
        key = np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ _TOP)
        width = np.uint64(2**64 - 1)
    if flags & DESC:
        key = ~key & width
    key = np.where(valid, key, np.uint64(0))
    null_digit = (~valid != bool(flags & NULLS_FIRST)).astype(np.uint8)
    return null_digit, key


def order(cols, keys):
    """-> the stable permutation that sorts the rows of `cols` by keys = [(column, flags)]."""
    n = cols[0][1].shape[0] if cols else 0
    if not keys:
        return np.arange(n)
    lex = []
    for c, flags in reversed(keys):   # np.lexsort: the LAST array is the most significant
        nd, key = encode(cols[c][0], cols[c][1], cols[c][2], flags)
        lex += [key, nd]
    return np.lexsort(lex)


def slice_of(n, limit, offset):
    begin = min(int(offset), n)
    count = n - begin if limit is None else min(int(limit), n - begin)
    return begin, count


def sort(cols, keys, output_attrs, limit=None, offset=0, n=None):
    n = (cols[0][1].shape[0] if cols else 0) if n is None else n
    begin, count = slice_of(n, limit, offset)
    rows = order(cols, keys)[begin:begin + count] if cols else np.arange(count)
    out = []
    for i, dt in output_attrs:
        assert cols[i][0] == dt
        out.append((dt, np.asarray(cols[i][1])[rows], np.asarray(cols[i][2], dtype=bool)[rows]))
    return count, out


def children(d):
    if isinstance(d, pl.ScanNode):
        return []
    if isinstance(d, (pl.AggNode, pl.SelectNode, pl.SortNode)):
        return [("child", d.child)]
    return [("left", d.left), ("right", d.right)]


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)].  The
    rows of a sort are in ITS order; what another kind makes of them is a multiset."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.SortNode):
        n, child = evaluate(plan, d.child)
        return sort(child, d.keys, node.output_attrs, d.limit, d.offset, n)
    if isinstance(d, pl.SelectNode):
        _, child = evaluate(plan, d.child)
        return _selectref.select(child, d.program, node.output_attrs)
    tmp = pl.Plan()
    moved = {}
    for field, kid in children(d):
        n, cols = evaluate(plan, kid)
        moved[field] = tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)])
        tmp.new_input(_filterref.to_table(n, cols))
    tmp.nodes.append(pl.PlanNode(type(d)(**{**d.__dict__, **moved}), list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _aggref.evaluate(tmp)


to_table = _filterref.to_table


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))


# ------------------------------------------------------------------ rows, in order
def _cells(dt, v, m):
    m = np.asarray(m, dtype=bool).tolist()
    if dt == pl.VARCHAR:
        return [x if ok else None for x, ok in zip(list(v), m)]
    if dt == pl.FP64:
        bits = np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.int64).tolist()
        return [("f64", x) if ok else None for x, ok in zip(bits, m)]
    return [x if ok else None for x, ok in zip(np.asarray(v).tolist(), m)]


def rel_rows(cols, n=None):
    """The rows of a relation IN ORDER: None = NULL, a double as ("f64", its bits), VARCHAR as bytes."""
    if not cols:
        return [()] * (n or 0)
    return list(zip(*[_cells(*c) for c in cols]))


def decoded_rows(types, decoded, n):
    """... of decoded result columns (pl.decode_table / _pagecheck.check_table)."""
    cols = []
    for dt, d in zip(types, decoded):
        cols.append((dt, d, [x is not None for x in d]) if isinstance(d, list) else (dt, d[0], d[1]))
    return rel_rows(cols, n)


def canon_key(cell):
    """What the comparison sees of a cell: every NaN is one value, -0.0 is +0.0."""
    if isinstance(cell, tuple):
        bits = cell[1] & (2**64 - 1)
        mag = bits & (2**63 - 1)
        return ("f64", "nan") if mag > 0x7FF0000000000000 else ("f64", 0 if mag == 0 else bits)
    return cell


def same_sorted(got, want_child_rows, keys, limit, offset, exact, outs=None):
    """Is `got` (result rows in order, rel_rows' cells) a correct result of sorting want_child_rows (the
    child's rows IN THE CHILD'S DEVICE ORDER if exact, in any order otherwise; types are read off the
    cells) by keys with the slice?  outs: the child columns the result holds, in order (default: all).
    -> None, or a string that says what is wrong.

    exact (SCAN child: the order is fully determined): rows equal position by position.
    Otherwise, ties being unspecified: (1) the key columns of the result equal the reference's key
    columns position by position — deterministic even with ties; NaNs count as equal, -0.0 equals +0.0;
    (2) for every key value the result rows with that key are a sub-multiset of the child's rows with
    that key; (3) they are the WHOLE group whenever the slice contains the whole group.  Every key
    column has to be among `outs` then, or (1) would have nothing to look at."""
    child = list(want_child_rows)
    width = len(child[0]) if child else 0
    outs = list(range(width)) if outs is None else list(outs)
    n = len(child)

    def cell_cmp_key(cell, flags):
        # (NULL digit, value) with the value as a number whose order is the key's order
        if cell is None:
            return (0 if flags & NULLS_FIRST else 1, 0)
        c = canon_key(cell)
        if isinstance(c, tuple):
            if c[1] == "nan":
                v = 2**64
            else:
                b = c[1]
                v = (~b & (2**64 - 1)) if b >> 63 else b | (1 << 63)
        else:
            v = c
        return (1 if flags & NULLS_FIRST else 0, -v if flags & DESC else v)

    idx = sorted(range(n), key=lambda r: tuple(cell_cmp_key(child[r][c], f) for c, f in keys))  # stable
    begin, count = slice_of(n, limit, offset)
    want = [tuple(child[r][c] for c in outs) for r in idx[begin:begin + count]]
    got = list(got)
    if len(got) != len(want):
        return f"{len(got)} rows, expected {len(want)}"
    if exact:
        for i, (g, w) in enumerate(zip(got, want)):
            if tuple(g) != w:
                return f"row {i}: {g} != {w}"
        return None
    where = []
    for c, _ in keys:
        if c not in outs:
            return f"key column {c} is not among the outputs: the tie-aware comparison cannot see it"
        where.append(outs.index(c))
    keyof = lambda row: tuple(canon_key(row[w]) for w in where)
    for i, (g, w) in enumerate(zip(got, want)):                        # (1)
        if keyof(g) != keyof(w):
            return f"row {i}: key {keyof(g)} != {keyof(w)}"
    have = {}
    for r in child:
        row = tuple(r[c] for c in outs)
        have.setdefault(keyof(row), Counter())[row] += 1
    seen = {}
    for g in got:
        seen.setdefault(keyof(g), Counter())[tuple(g)] += 1
    for k, rows in seen.items():                                       # (2)
        extra = rows - have.get(k, Counter())
        if extra:
            return f"key {k}: rows that the child does not hold (that often): {list(extra.items())[:3]}"
    at = 0
    sorted_keys = [tuple(canon_key(child[r][c]) for c, _ in keys) for r in idx]
    while at < n:                                                      # (3)
        end = at
        while end < n and sorted_keys[end] == sorted_keys[at]:
            end += 1
        if begin <= at and end <= begin + count:
            if seen.get(sorted_keys[at], Counter()) != have[sorted_keys[at]]:
                return f"key {sorted_keys[at]}: the slice holds the whole group, the result does not"
        at = end
    return None
