"""Plain numpy reference for plans that hold selection nodes (pl.SelectNode, RJ_NODE_SELECT in
include/rj.h), test infrastructure for tests/test_select_plan.py and tests/test_gpu_select.py.

evaluate() handles every node kind, so nested plans can be checked.  A selection is computed here:
every leaf of the postfix program is one vectorised mask over the child's columns, AND / OR / NOT
combine masks on a stack, the rows of the last mask are taken from the named columns.  Every other
kind goes to tests/_aggref.py: its children are evaluated HERE and handed over as the scans of a
temporary plan (what _aggref.evaluate does with _fullref).

The predicate rules are rj_table_from_csv's (include/rj.h): a comparison is false on NULL, NOT flips
the bit whatever the row holds, an INT32 column compares with the literal cut to 32 bits, an FP64
column IEEE-wise (a literal given as a Python float is that double; one given as an int is the BITS
of the double, as rj_filter_op::ivalue is), and a column comparison (op, column, other column) is
false when either side is NULL.  A relation is a list of (type, values, valid) columns as in
_filterref."""
from __future__ import annotations

import numpy as np

import _aggref
import _filterref
from pyrj import plan as pl

CMP = {"EQ": np.equal, "NEQ": np.not_equal, "LT": np.less, "GT": np.greater, "LEQ": np.less_equal, "GEQ": np.greater_equal}
NP_OF = {pl.INT32: np.int32, pl.INT64: np.int64, pl.FP64: np.float64}


def literal_of(dtype, lit):
    """The value a literal of a program tuple stands for when it meets a column of `dtype`."""
    if dtype == pl.FP64:
        return np.float64(lit) if isinstance(lit, float) else np.array([int(lit)], dtype=np.int64).view(np.float64)[0]
    lit = int(lit)
    if dtype == pl.INT32:
        return np.int64((lit + 2**31) % 2**32 - 2**31)
    assert -2**63 <= lit < 2**63
    return np.int64(lit)


def mask(cols, program):
    """-> bool[n]: the rows of `cols` for which `program` leaves 1 (every row for an empty one)."""
    n = cols[0][1].shape[0] if cols else 0
    if not program:
        return np.ones(n, dtype=bool)
    st = []
    for term in program:
        op = term[0]
        if op in ("AND", "OR"):
            b, a = st.pop(), st.pop()
            st.append(a & b if op == "AND" else a | b)
        elif op == "NOT":
            st.append(~st.pop())
        elif op in ("IS_NULL", "IS_NOT_NULL"):
            valid = np.asarray(cols[term[1]][2], dtype=bool)
            st.append(~valid if op == "IS_NULL" else valid.copy())
        else:
            dt, x, valid = cols[term[1]]
            assert dt in NP_OF, "predicates go over INT32 / INT64 / FP64 columns"
            valid = np.asarray(valid, dtype=bool)
            if op.startswith("COL_"):
                dt2, y, valid2 = cols[term[2]]
                assert dt2 == dt
                valid = valid & np.asarray(valid2, dtype=bool)
                y = np.asarray(y)
                op = op[4:]
            else:
                y = literal_of(dt, term[2])
            x = np.asarray(x)
            if dt != pl.FP64:
                x, y = x.astype(np.int64), (y.astype(np.int64) if isinstance(y, np.ndarray) else y)
            with np.errstate(invalid="ignore"):
                st.append(valid & CMP[op](x, y))
    assert len(st) == 1
    return st[0]


def select(cols, program, output_attrs):
    rows = np.flatnonzero(mask(cols, program))
    out = []
    for i, dt in output_attrs:
        assert cols[i][0] == dt
        out.append((dt, np.asarray(cols[i][1])[rows], np.asarray(cols[i][2], dtype=bool)[rows]))
    return int(rows.shape[0]), out


def children(d):
    if isinstance(d, pl.ScanNode):
        return []
    if isinstance(d, (pl.AggNode, pl.SelectNode)):
        return [("child", d.child)]
    return [("left", d.left), ("right", d.right)]


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)]."""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.SelectNode):
        _, child = evaluate(plan, d.child)
        return select(child, d.program, node.output_attrs)
    # any other kind: the children's results become the inputs of a plan _aggref knows
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
same = _aggref.same


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))


# ------------------------------------------------------------------ random programs
def random_leaf(rng, cols):
    """One leaf over the INT32 / INT64 / FP64 columns of `cols`: IS [NOT] NULL, a comparison with a
    literal (half of them a value the column holds, an INT32 one now and then outside 32 bits) or
    with another column of the same type."""
    usable = [i for i, c in enumerate(cols) if c[0] in NP_OF]
    c = usable[int(rng.integers(0, len(usable)))]
    dt, vals, _ = cols[c]
    k = rng.random()
    if k < 0.15:
        return (("IS_NULL", "IS_NOT_NULL")[int(rng.integers(0, 2))], c)
    op = ("EQ", "NEQ", "LT", "GT", "LEQ", "GEQ")[int(rng.integers(0, 6))]
    twins = [i for i in usable if i != c and cols[i][0] == dt]
    if k < 0.4 and twins:
        return ("COL_" + op, c, twins[int(rng.integers(0, len(twins)))])
    n = np.asarray(vals).shape[0]
    if n and rng.random() < 0.5:
        lit = np.asarray(vals)[int(rng.integers(0, n))].item()
    elif dt == pl.FP64:
        lit = float(rng.standard_normal()) * 10.0 ** int(rng.integers(-3, 4))
    elif dt == pl.INT32:
        lit = int(rng.integers(-2**31, 2**31))
    else:
        lit = int(rng.integers(-2**63, 2**63 - 1))
    if dt == pl.INT32 and rng.random() < 0.1:
        lit += 2**32 * int(rng.integers(-3, 4))  # (cut back to 32 bits by the comparison)
    return (op, c, float(lit) if dt == pl.FP64 else int(lit))


def random_program(rng, cols, n_ops):
    """A well-formed postfix program of exactly n_ops ops (1 <= n_ops <= 64) over `cols`."""
    prog, depth = [], 0
    while len(prog) < n_ops:
        left = n_ops - len(prog)
        can_leaf = left - 1 >= depth      # a leaf now still leaves room for the ops that fold the stack
        can_bin = depth >= 2
        can_not = depth >= 1 and left - 1 >= depth - 1
        must_fold = left == depth - 1     # only binary ops from here on
        pick = rng.random()
        if can_bin and (must_fold or pick < 0.35 or not (can_leaf or can_not)):
            prog.append((("AND",), ("OR",))[int(rng.integers(0, 2))])
            depth -= 1
        elif can_not and (pick < 0.5 or not can_leaf):
            prog.append(("NOT",))
        else:
            assert can_leaf
            prog.append(random_leaf(rng, cols))
            depth += 1
    assert depth == 1
    return prog


def deepest_program(rng, cols, n_ops=64):
    """The deepest stack n_ops ops allow: n_ops / 2 leaves, then the ops that fold them (a program of
    L leaves needs L - 1 binary ops, so 64 ops never go deeper than 32), one NOT at the end."""
    leaves = n_ops // 2
    prog = [random_leaf(rng, cols) for _ in range(leaves)]
    prog += [(("AND",), ("OR",))[int(rng.integers(0, 2))] for _ in range(leaves - 1)]
    return prog + [("NOT",)] * (n_ops - 2 * leaves + 1)


def max_depth(program):
    d = m = 0
    for term in program:
        d += -1 if term[0] in ("AND", "OR") else 0 if term[0] == "NOT" else 1
        m = max(m, d)
    return m
