"""Host-side mirror of the reference's plan/data model, for tests and bench.

Same names and argument meaning as the reference (include/plan.h):
  * ``Column`` / ``ColumnarTable``            — plan.h:60-105
  * ``Plan.new_scan_node/new_join_node/new_input`` — plan.h:118-148
  * ``ScanNode{base_table_id}`` / ``JoinNode{build_left,left,right,left_attr,right_attr}``
    and ``output_attrs = [(index, DataType)]``  — plan.h:32-52
so the parity tests read like reference tests/unit_tests.cpp.  Pages are numpy
``uint8[n_pages, 8192]`` arrays (one row per Page).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import pages as pg

INT32, INT64, FP64, VARCHAR = pg.INT32, pg.INT64, pg.FP64, pg.VARCHAR
TYPE_NAMES = {INT32: "INT32", INT64: "INT64", FP64: "FP64", VARCHAR: "VARCHAR"}
TYPE_IDS = {v: k for k, v in TYPE_NAMES.items()}


@dataclass
class Column:
    type: int
    pages: np.ndarray = field(default_factory=lambda: np.zeros((0, pg.PAGE_SIZE), np.uint8))


@dataclass
class ColumnarTable:
    num_rows: int = 0
    columns: list = field(default_factory=list)


@dataclass
class ScanNode:
    base_table_id: int


@dataclass
class JoinNode:
    build_left: bool
    left: int
    right: int
    left_attr: int
    right_attr: int


# rj_node_kind (include/rj.h)
NODE_SCAN, NODE_JOIN, NODE_SEMI, NODE_ANTI, NODE_OUTER, NODE_FULL, NODE_AGG, NODE_SELECT = 0, 1, 2, 3, 4, 5, 6, 7
NODE_SORT = 8
NODE_GROUP = 9
NODE_WINDOW = 10
NODE_MAP = 11
NODE_SETOP = 12
# rj_sort_key::flags, RJ_SORT_NO_LIMIT
SORT_DESC, SORT_NULLS_FIRST = 1, 2
SORT_NO_LIMIT = 2**64 - 1
# rj_agg_func and the RJ_AGG_OUT / RJ_AGG_FUNC / RJ_AGG_COL encoding of an aggregation's out_idx
AGG_KEY, AGG_COUNT_STAR, AGG_COUNT, AGG_SUM, AGG_MIN, AGG_MAX = 0, 1, 2, 3, 4, 5
AGG_FSUM = 8  # RJ_NODE_GROUP only: the exactly rounded sum of an FP64 column (6 and 7 are not assigned)


def agg_out(func, col):
    return (int(func) << 56) | int(col)


def agg_func(x):
    return int(x) >> 56


def agg_col(x):
    return int(x) & ((1 << 56) - 1)


# rj_win_func and the RJ_WIN_OUT / RJ_WIN_FUNC / RJ_WIN_COL encoding of a window node's out_idx (the
# bit layout of RJ_AGG_OUT)
WIN_COL, WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_COUNT_STAR, WIN_COUNT, WIN_SUM, WIN_MIN, WIN_MAX = range(9)
# ... the functions that take an rj_win_arg (lo, hi): a ROWS frame as signed offsets from the current row,
# LAG / LEAD's offset k or NTILE's bucket count in lo (9 .. 15 are not assigned)
(WIN_LAG, WIN_LEAD, WIN_FIRST_VALUE, WIN_LAST_VALUE, WIN_NTILE, WIN_ROWS_COUNT_STAR, WIN_ROWS_COUNT, WIN_ROWS_SUM, WIN_ROWS_MIN,
 WIN_ROWS_MAX) = range(16, 26)
WIN_UNBOUNDED_PRECEDING, WIN_UNBOUNDED_FOLLOWING = -(2**63), 2**63 - 1


def win_out(func, col):
    return (int(func) << 56) | int(col)


def win_func(x):
    return int(x) >> 56


def win_col(x):
    return int(x) & ((1 << 56) - 1)


# rj_map_func and the RJ_MAP_OUT / RJ_MAP_FUNC / RJ_MAP_ARG encoding of a map node's out_idx (the bit layout
# of RJ_AGG_OUT)
MAP_COL, MAP_EXPR = 0, 1
MAP_OUT_NAMES = {"COL": MAP_COL, "EXPR": MAP_EXPR}


def map_out(func, x):
    return (int(func) << 56) | int(x)


def map_func(x):
    return int(x) >> 56


def map_arg(x):
    return int(x) & ((1 << 56) - 1)


# rj_setop and the RJ_SETOP_OUT / RJ_SETOP_LCOL / RJ_SETOP_RCOL encoding of a set operation's out_idx
SET_UNION_ALL, SET_UNION, SET_INTERSECT, SET_INTERSECT_ALL, SET_EXCEPT, SET_EXCEPT_ALL = range(6)


def setop_out(lcol, rcol):
    return ((int(rcol) & 0xFFFFFFFF) << 32) | (int(lcol) & 0xFFFFFFFF)


def setop_lcol(x):
    return int(x) & 0xFFFFFFFF


def setop_rcol(x):
    return (int(x) >> 32) & 0xFFFFFFFF


@dataclass
class FilterJoinNode:
    """Semi (kind NODE_SEMI) or anti (NODE_ANTI) join: the rows of the preserved child that have
    (or have no) partner in the filter child.  build_left picks the filter side; output_attrs may
    name columns of the preserved side only (include/rj.h)."""
    kind: int
    build_left: bool
    left: int
    right: int
    left_attr: int
    right_attr: int


@dataclass
class OuterJoinNode:
    """Outer join (kind NODE_OUTER): the inner join's rows plus every row of the preserved child
    without a partner, once, with NULL in the optional child's columns.  build_left picks the
    OPTIONAL side (the one that is built); output_attrs may name columns of both sides
    (include/rj.h)."""
    build_left: bool
    left: int
    right: int
    left_attr: int
    right_attr: int


@dataclass
class FullOuterJoinNode:
    """Full outer join (kind NODE_FULL): the inner join's rows plus every row of EITHER child
    without a partner, once, with NULL in the other child's columns.  build_left picks the child
    that is built, an execution hint only; output_attrs may name columns of both sides
    (include/rj.h)."""
    build_left: bool
    left: int
    right: int
    left_attr: int
    right_attr: int


@dataclass
class AggNode:
    """Aggregation (kind NODE_AGG): GROUP BY column key_attr of the one child, one row per distinct
    key, NULL keys one group.  The PlanNode's output_attrs hold (RJ_AGG_OUT(func, column), result
    type) pairs (include/rj.h)."""
    child: int
    key_attr: int


@dataclass
class SelectNode:
    """Selection (kind NODE_SELECT): the rows of the one child for which `program` leaves 1; the
    PlanNode's output_attrs index the child's outputs as a scan's index its base table.  program is
    a postfix filter in the tuple form capi.filter_to_c takes (capi.F_OPS), its columns the child's
    outputs; a column comparison is (op, column, other column).  An empty program keeps every row
    (include/rj.h)."""
    child: int
    program: list


@dataclass
class SortNode:
    """Sort (kind NODE_SORT): ORDER BY keys [LIMIT limit [OFFSET offset]] over the one child; the
    PlanNode's output_attrs index the child's outputs as a selection's do.  keys = [(column, flags)],
    the first most significant, column an output of the child, flags a set of SORT_DESC and
    SORT_NULLS_FIRST (default: ascending, NULLs last).  limit None = no LIMIT.  The row order of the
    result is promised only at the plan's root (include/rj.h)."""
    child: int
    keys: list
    limit: object = None
    offset: int = 0


@dataclass
class GroupNode:
    """Grouping (kind NODE_GROUP): GROUP BY keys, or with keys == [] the scalar aggregate over all
    rows.  keys = [(column, flags)] as a SortNode's; the PlanNode's output_attrs hold
    (RJ_AGG_OUT(func, column), result type) pairs as an AggNode's, over any number of columns; AGG_KEY
    may name any key column.  The groups come out in the order of the keys, promised only at the
    plan's root (include/rj.h)."""
    child: int
    keys: list


@dataclass
class WindowNode:
    """Window functions (kind NODE_WINDOW) OVER (PARTITION BY part_keys ORDER BY order_keys), both
    lists [(column, flags)] as a SortNode's and either may be empty.  The PlanNode's output_attrs hold
    (RJ_WIN_OUT(func, column), result type) pairs; WIN_COL passes a child column through.  The frame is
    SQL's default: up to the current row's last peer with order keys, the whole partition without.  The
    rows come out ordered by (part_keys, order_keys), promised only at the plan's root (include/rj.h).
    `args`: None, or one entry per output, (lo, hi) for a function from WIN_LAG on (its own ROWS frame as
    signed offsets, LAG / LEAD's offset, NTILE's bucket count) and None for any other (RJ_WINDOW_ARGS)."""
    child: int
    part_keys: list
    order_keys: list
    args: list = None


@dataclass
class MapNode:
    """Computed columns (kind NODE_MAP): `program` is a postfix list in the tuple form capi.expr_to_c
    takes (capi.X_OPS) that holds any number of expressions, each ended by ("OUT",); its columns are the
    child's outputs.  The PlanNode's output_attrs hold (RJ_MAP_OUT(func, x), result type) pairs: MAP_COL
    passes child column x through, MAP_EXPR is expression x.  The result has the child's rows in the child's
    order; below the root (or below MAPs only) a sort, grouping or window child keeps its order
    (include/rj.h)."""
    child: int
    program: list


@dataclass
class SetOpNode:
    """Set operation (kind NODE_SETOP): `op` (SET_UNION_ALL ... SET_EXCEPT_ALL) of the children `left` and
    `right`.  The PlanNode's output_attrs hold (RJ_SETOP_OUT(left column, right column), type) pairs: both
    columns must have the declared type.  Rows are equal under the grouping equalities (NULL = NULL,
    -0.0 = +0.0, NaN = NaN); every operation but UNION ALL gives canonical values, ordered by the output
    columns, which is promised only at the plan's root (include/rj.h)."""
    op: int
    left: int
    right: int


@dataclass
class PlanNode:
    data: object
    output_attrs: list  # [(index, DataType)]


class Plan:
    def __init__(self):
        self.nodes: list[PlanNode] = []
        self.inputs: list[ColumnarTable] = []
        self.root: int = 0

    def new_join_node(self, build_left, left, right, left_attr, right_attr, output_attrs):
        self.nodes.append(PlanNode(JoinNode(bool(build_left), left, right, left_attr, right_attr), list(output_attrs)))
        return len(self.nodes) - 1

    def new_semi_join_node(self, build_left, left, right, left_attr, right_attr, output_attrs):
        """WHERE EXISTS: rows of the preserved child (the one build_left does not name) whose key
        has a partner in the filter child, once each."""
        return self._filter_node(NODE_SEMI, build_left, left, right, left_attr, right_attr, output_attrs)

    def new_anti_join_node(self, build_left, left, right, left_attr, right_attr, output_attrs):
        """WHERE NOT EXISTS: rows of the preserved child whose key has no partner in the filter
        child (NULL and NaN keys included)."""
        return self._filter_node(NODE_ANTI, build_left, left, right, left_attr, right_attr, output_attrs)

    def new_outer_join_node(self, build_left, left, right, left_attr, right_attr, output_attrs):
        """LEFT / RIGHT OUTER JOIN.  build_left names the optional side (NULL where a preserved row
        has no partner): `left LEFT JOIN right` is build_left=False, `left RIGHT JOIN right` is
        build_left=True."""
        node = OuterJoinNode(bool(build_left), left, right, left_attr, right_attr)
        self.nodes.append(PlanNode(node, list(output_attrs)))
        return len(self.nodes) - 1

    def new_full_outer_join_node(self, build_left, left, right, left_attr, right_attr, output_attrs):
        """FULL OUTER JOIN.  build_left names the child that is built; the result does not depend
        on it."""
        node = FullOuterJoinNode(bool(build_left), left, right, left_attr, right_attr)
        self.nodes.append(PlanNode(node, list(output_attrs)))
        return len(self.nodes) - 1

    def new_agg_node(self, child, key_attr, outputs):
        """GROUP BY key_attr.  outputs = [(func, column, result type)] with func one of AGG_KEY ...
        AGG_MAX; the column of AGG_COUNT_STAR is 0."""
        oa = [(agg_out(f, c), t) for f, c, t in outputs]
        self.nodes.append(PlanNode(AggNode(child, key_attr), oa))
        return len(self.nodes) - 1

    def new_select_node(self, child, program, output_attrs):
        """WHERE / HAVING / projection: the child's rows that pass `program` (see SelectNode)."""
        self.nodes.append(PlanNode(SelectNode(child, list(program or [])), list(output_attrs)))
        return len(self.nodes) - 1

    def new_sort_node(self, child, keys, output_attrs, limit=None, offset=0):
        """ORDER BY / LIMIT / OFFSET: rows [offset, offset + limit) of the child ordered by `keys`
        (see SortNode)."""
        self.nodes.append(PlanNode(SortNode(child, [tuple(k) for k in keys], limit, offset), list(output_attrs)))
        return len(self.nodes) - 1

    def new_group_node(self, child, keys, outputs):
        """GROUP BY keys ([(column, flags)], [] = one group of all rows).  outputs = [(func, column,
        result type)] as for new_agg_node."""
        oa = [(agg_out(f, c), t) for f, c, t in outputs]
        self.nodes.append(PlanNode(GroupNode(child, [tuple(k) for k in keys]), oa))
        return len(self.nodes) - 1

    def new_window_node(self, child, part_keys, order_keys, outputs):
        """Window functions over PARTITION BY part_keys ORDER BY order_keys ([(column, flags)] each).
        outputs = [(func, column, result type)] with func one of WIN_COL ... WIN_MAX; the column of a
        ranking function and of WIN_COUNT_STAR is 0.  A function from WIN_LAG on is (func, column, result
        type, lo, hi): the ROWS frame as signed offsets (WIN_UNBOUNDED_PRECEDING / _FOLLOWING), LAG / LEAD's
        offset or NTILE's bucket count in lo with hi = 0."""
        oa = [(win_out(o[0], o[1]), o[2]) for o in outputs]
        args = [(int(o[3]), int(o[4])) if len(o) == 5 else None for o in outputs]
        if not any(a is not None for a in args):
            args = None
        self.nodes.append(PlanNode(WindowNode(child, [tuple(k) for k in part_keys], [tuple(k) for k in order_keys], args), oa))
        return len(self.nodes) - 1

    def new_map_node(self, child, program, outputs):
        """Computed columns over `child` (see MapNode).  outputs = [("COL", c, type) | ("EXPR", e, type)]
        (or MAP_COL / MAP_EXPR for the names)."""
        oa = [(map_out(MAP_OUT_NAMES.get(f, f), x), t) for f, x, t in outputs]
        self.nodes.append(PlanNode(MapNode(child, [tuple(t) for t in (program or [])]), oa))
        return len(self.nodes) - 1

    def new_setop_node(self, op, left, right, outputs):
        """UNION / INTERSECT / EXCEPT [ALL] of `left` and `right` (see SetOpNode).  outputs = [(left column,
        right column, type)]."""
        oa = [(setop_out(lc, rc), t) for lc, rc, t in outputs]
        self.nodes.append(PlanNode(SetOpNode(int(op), left, right), oa))
        return len(self.nodes) - 1

    def _filter_node(self, kind, build_left, left, right, left_attr, right_attr, output_attrs):
        node = FilterJoinNode(kind, bool(build_left), left, right, left_attr, right_attr)
        self.nodes.append(PlanNode(node, list(output_attrs)))
        return len(self.nodes) - 1

    def new_scan_node(self, base_table_id, output_attrs):
        self.nodes.append(PlanNode(ScanNode(base_table_id), list(output_attrs)))
        return len(self.nodes) - 1

    def new_input(self, table: ColumnarTable):
        self.inputs.append(table)
        return len(self.inputs) - 1


# ------------------------------------------------------------ table helpers --
def make_table(columns) -> ColumnarTable:
    """columns: list of (dtype, values[, valid]) for fixed width, or
    (VARCHAR, list_of_bytes_or_None).  Pages follow the reference fill rule
    (what ``Table(...).to_columnar()`` produces in the reference tests)."""
    t = ColumnarTable()
    n = None
    for spec in columns:
        dt = spec[0]
        if dt == VARCHAR:
            vals = list(spec[1])
            cn = len(vals)
            t.columns.append(Column(dt, pg.pack_varchar(vals)))
        else:
            vals = np.asarray(spec[1], dtype=pg.NP_DTYPE[dt])
            valid = spec[2] if len(spec) > 2 else None
            cn = vals.shape[0]
            t.columns.append(Column(dt, pg.pack_fixed(vals, valid, dt)))
        if n is None:
            n = cn
        elif n != cn:
            raise ValueError("ragged columns")
    t.num_rows = n or 0
    return t


def table_from_rows(rows, types) -> ColumnarTable:
    """``Table(rows, types).to_columnar()`` of the reference tests: rows is a
    list of tuples with None for NULL."""
    cols = []
    for ci, dt in enumerate(types):
        col = [r[ci] for r in rows]
        if dt == VARCHAR:
            cols.append((dt, [None if v is None else (v.encode() if isinstance(v, str) else v) for v in col]))
        else:
            valid = np.array([v is not None for v in col], dtype=bool)
            vals = np.array([0 if v is None else v for v in col], dtype=pg.NP_DTYPE[dt])
            cols.append((dt, vals, valid))
    t = make_table(cols)
    t.num_rows = len(rows)
    return t


def decode_table(t: ColumnarTable):
    """-> list per column of (values, valid) or list[bytes|None] (VARCHAR)."""
    out = []
    for c in t.columns:
        if c.type == VARCHAR:
            out.append(pg.unpack_varchar(c.pages, t.num_rows))
        else:
            out.append(pg.unpack_fixed(c.pages, t.num_rows, c.type))
    return out


def table_rows(t: ColumnarTable):
    """``Table::from_columnar(t).table()`` as a list of tuples (None = NULL)."""
    cols = decode_table(t)
    rows = []
    for i in range(t.num_rows):
        r = []
        for c, col in zip(t.columns, cols):
            if c.type == VARCHAR:
                r.append(col[i])
            else:
                vals, valid = col
                r.append(vals[i].item() if valid[i] else None)
        rows.append(tuple(r))
    return rows


def _sort_key(row):
    # std::variant ordering is (index, value) with monostate last (index 4);
    # any total order works for multiset comparison
    return tuple((1, 0) if v is None else (0, v) for v in row)


def sorted_rows(t: ColumnarTable):
    return sorted(table_rows(t), key=_sort_key)


def canonical_rows(t: ColumnarTable):
    """sorted_rows with floats replaced by their bit patterns, so that NaN payloads (and
    -0.0 / +0.0) compare by identity of the stored value — for differential tests."""
    import struct

    def canon(v):
        return ("f64", struct.unpack("<q", struct.pack("<d", v))[0]) if isinstance(v, float) else v

    rows = [tuple(canon(v) for v in r) for r in table_rows(t)]
    return sorted(rows, key=lambda r: tuple((2, 0) if v is None else ((1, v[1]) if isinstance(v, tuple) else (0, v)) for v in r))


def table_digest(t: ColumnarTable):
    """Order-independent digest of a fixed-width table: (rows, sum, xor) of a
    64-bit row hash — for sizes where sorting rows in Python is too slow."""
    n = t.num_rows
    h = np.full(n, 0x9E3779B97F4A7C15, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in t.columns:
            if c.type == VARCHAR:
                raise ValueError("digest supports fixed-width columns only")
            vals, valid = pg.unpack_fixed(c.pages, n, c.type)
            if c.type == INT32:
                bits = vals.astype(np.int64).view(np.uint64)  # the declared type is mixed in below
            else:
                bits = np.ascontiguousarray(vals).view(np.uint64)
            x = np.where(valid, bits, np.uint64(0xDEADBEEFCAFEF00D)) + np.uint64(c.type + 1)
            x = x ^ (x >> np.uint64(33))
            x = x * np.uint64(0xFF51AFD7ED558CCD)
            x = x ^ (x >> np.uint64(33))
            h = (h ^ x) * np.uint64(0xC4CEB9FE1A85EC53)
            h = h ^ (h >> np.uint64(29))
        s = int(h.sum(dtype=np.uint64)) if n else 0
        x = int(np.bitwise_xor.reduce(h)) if n else 0
    return (n, s, x)


# ------------------------------------------------------------- C marshalling --
class rj_node(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("build_left", C.c_int32),
        ("base_table_id", C.c_uint64),
        ("left", C.c_uint64),
        ("right", C.c_uint64),
        ("left_attr", C.c_uint64),
        ("right_attr", C.c_uint64),
        ("n_out", C.c_uint64),
        ("out_idx", C.POINTER(C.c_uint64)),
        ("out_type", C.POINTER(C.c_int32)),
    ]


class rj_sort_key(C.Structure):
    _fields_ = [("column", C.c_int32), ("flags", C.c_int32)]


class rj_win_arg(C.Structure):
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64)]


class rj_column(C.Structure):
    _fields_ = [("type", C.c_int32), ("n_pages", C.c_uint64), ("pages", C.POINTER(C.c_void_p))]


class rj_input(C.Structure):
    _fields_ = [("num_rows", C.c_uint64), ("n_cols", C.c_uint64), ("cols", C.POINTER(rj_column))]


class rj_plan(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint64),
        ("nodes", C.POINTER(rj_node)),
        ("n_inputs", C.c_uint64),
        ("inputs", C.POINTER(rj_input)),
        ("root", C.c_uint64),
    ]


def input_to_c(t: ColumnarTable, keep: list) -> rj_input:
    cols = (rj_column * max(1, len(t.columns)))()
    keep.append(cols)
    for ci, c in enumerate(t.columns):
        pages = np.ascontiguousarray(c.pages, dtype=np.uint8).reshape(-1, pg.PAGE_SIZE)
        keep.append(pages)
        n = pages.shape[0]
        ptrs = (C.c_void_p * max(1, n))()
        base = pages.ctypes.data
        for i in range(n):
            ptrs[i] = base + i * pg.PAGE_SIZE
        keep.append(ptrs)
        cols[ci].type = c.type
        cols[ci].n_pages = n
        cols[ci].pages = C.cast(ptrs, C.POINTER(C.c_void_p))
    inp = rj_input()
    inp.num_rows = t.num_rows
    inp.n_cols = len(t.columns)
    inp.cols = C.cast(cols, C.POINTER(rj_column))
    return inp


def plan_to_c(plan: Plan, with_inputs: bool = True):
    """-> (rj_plan, keepalive).  The flattening the C++ shim performs."""
    keep: list = []
    nodes = (rj_node * max(1, len(plan.nodes)))()
    keep.append(nodes)
    for i, n in enumerate(plan.nodes):
        nd = nodes[i]
        k = len(n.output_attrs)
        idx = (C.c_uint64 * max(1, k))(*[a[0] for a in n.output_attrs])
        typ = (C.c_int32 * max(1, k))(*[int(a[1]) for a in n.output_attrs])
        keep += [idx, typ]
        nd.n_out = k
        nd.out_idx = C.cast(idx, C.POINTER(C.c_uint64))
        nd.out_type = C.cast(typ, C.POINTER(C.c_int32))
        if isinstance(n.data, (JoinNode, FilterJoinNode, OuterJoinNode, FullOuterJoinNode)):
            if isinstance(n.data, FilterJoinNode):
                nd.kind = n.data.kind
            elif isinstance(n.data, FullOuterJoinNode):
                nd.kind = NODE_FULL
            else:
                nd.kind = NODE_OUTER if isinstance(n.data, OuterJoinNode) else NODE_JOIN
            nd.build_left = 1 if n.data.build_left else 0
            nd.left, nd.right = n.data.left, n.data.right
            nd.left_attr, nd.right_attr = n.data.left_attr, n.data.right_attr
        elif isinstance(n.data, AggNode):
            nd.kind = NODE_AGG
            nd.left = n.data.child
            nd.left_attr = n.data.key_attr
        elif isinstance(n.data, SelectNode):
            from . import capi  # (capi imports this module)

            ops, n_ops, lits = capi.filter_to_c(n.data.program)
            keep += [ops, lits]
            nd.kind = NODE_SELECT
            nd.left = n.data.child
            nd.right = n_ops  # RJ_SELECT_N_OPS / RJ_SELECT_OPS: the struct cannot grow
            nd.right_attr = C.addressof(ops) if n_ops else 0
        elif isinstance(n.data, SortNode):
            nk = len(n.data.keys)
            karr = (rj_sort_key * max(1, nk))()
            for j, (col, flags) in enumerate(n.data.keys):
                karr[j].column, karr[j].flags = int(col), int(flags)
            keep.append(karr)
            nd.kind = NODE_SORT
            nd.left = n.data.child
            nd.right = nk  # RJ_SORT_N_KEYS / RJ_SORT_KEYS / RJ_SORT_LIMIT / RJ_SORT_OFFSET: the struct cannot grow
            nd.right_attr = C.addressof(karr) if nk else 0
            nd.left_attr = SORT_NO_LIMIT if n.data.limit is None else int(n.data.limit)
            nd.base_table_id = int(n.data.offset)
        elif isinstance(n.data, GroupNode):
            nk = len(n.data.keys)
            karr = (rj_sort_key * max(1, nk))()
            for j, (col, flags) in enumerate(n.data.keys):
                karr[j].column, karr[j].flags = int(col), int(flags)
            keep.append(karr)
            nd.kind = NODE_GROUP
            nd.left = n.data.child
            nd.right = nk  # RJ_GROUP_N_KEYS / RJ_GROUP_KEYS: the struct cannot grow
            nd.right_attr = C.addressof(karr) if nk else 0
        elif isinstance(n.data, WindowNode):
            wkeys = list(n.data.part_keys) + list(n.data.order_keys)
            nk = len(wkeys)
            karr = (rj_sort_key * max(1, nk))()
            for j, (col, flags) in enumerate(wkeys):
                karr[j].column, karr[j].flags = int(col), int(flags)
            keep.append(karr)
            nd.kind = NODE_WINDOW
            nd.left = n.data.child
            nd.right = nk  # RJ_WINDOW_N_KEYS / RJ_WINDOW_KEYS / RJ_WINDOW_N_PART: the struct cannot grow
            nd.right_attr = C.addressof(karr) if nk else 0
            nd.left_attr = len(n.data.part_keys)
            if any(win_func(a[0]) >= WIN_LAG for a in n.output_attrs):  # RJ_WINDOW_ARGS: read only then
                wargs = list(n.data.args or []) + [None] * k
                aarr = (rj_win_arg * max(1, k))()
                for j in range(k):
                    aarr[j].lo, aarr[j].hi = wargs[j] or (0, 0)
                keep.append(aarr)
                nd.base_table_id = C.addressof(aarr)
        elif isinstance(n.data, MapNode):
            from . import capi  # (capi imports this module)

            ops, n_ops = capi.expr_to_c(n.data.program)
            keep.append(ops)
            nd.kind = NODE_MAP
            nd.left = n.data.child
            nd.right = n_ops  # RJ_MAP_N_OPS / RJ_MAP_OPS: the struct cannot grow
            nd.right_attr = C.addressof(ops) if n_ops else 0
        elif isinstance(n.data, SetOpNode):
            nd.kind = NODE_SETOP
            nd.left, nd.right = n.data.left, n.data.right
            nd.left_attr = n.data.op  # RJ_SETOP_OP: the struct cannot grow
        else:
            nd.kind = 0
            nd.base_table_id = n.data.base_table_id
    p = rj_plan()
    p.n_nodes = len(plan.nodes)
    p.nodes = C.cast(nodes, C.POINTER(rj_node))
    p.root = plan.root
    if with_inputs:
        ins = (rj_input * max(1, len(plan.inputs)))()
        keep.append(ins)
        for i, t in enumerate(plan.inputs):
            ins[i] = input_to_c(t, keep)
        p.n_inputs = len(plan.inputs)
        p.inputs = C.cast(ins, C.POINTER(rj_input))
    else:
        p.n_inputs = len(plan.inputs)
        p.inputs = None
    return p, keep
