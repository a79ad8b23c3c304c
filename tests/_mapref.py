"""Plain numpy reference for plans that hold map nodes (pl.MapNode, RJ_NODE_MAP in include/rj.h), test
infrastructure for tests/test_map_plan.py and tests/test_gpu_map.py.

A map node is computed here, vectorised over the child's rows: an I64 stack value is a uint64 array
(numpy's unsigned arithmetic wraps modulo 2^64), an F64 one a float64 array (IEEE-754 binary64, every op
rounded once, as C's), each with a bool mask of its NULLs.  Integer DIV / MOD are numpy's floored ones
turned into C's truncating ones, with the zero divisor (NULL) and the divisor -1 (no overflow) taken out
first.  RJ_X_OUT replaces every NaN by 0x7ff8000000000000.

evaluate() handles every node kind, so nested plans can be checked: every other kind goes to
tests/_windowref.py with its children evaluated HERE and handed over as the scans of a temporary plan.
The rows of a map node are its child's rows in the child's order (a sort's, a grouping's, a window
node's: their own order).  A relation is a list of (type, values, valid) columns as in _filterref.

random_program() emits seeded well-typed programs within the op and depth limits; EDGE_I64 / EDGE_F64
are the edge values of the issue's grid."""
from __future__ import annotations

import struct

import numpy as np

import _filterref
import _windowref
from pyrj import plan as pl

MAX_OPS, MAX_DEPTH = 128, 8
U = np.uint64
SIGN = U(1 << 63)
CANONICAL_NAN = 0x7FF8000000000000
I64_MIN, I64_MAX = -(2**63), 2**63 - 1
ARITH = ("ADD", "SUB", "MUL", "DIV", "MOD")
CMPS = ("EQ", "NEQ", "LT", "GT", "LEQ", "GEQ")


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits & (2**64 - 1)))[0]


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


EDGE_I64 = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX, -(2**31), 2**31 - 1, 2**31, -(2**31) - 1, 3, -7, 10**18]
EDGE_F64_BITS = [bits_of(v) for v in (0.0, -0.0, 5e-324, float("inf"), float("-inf"), 2.0**53 + 1, 2.0**63, -(2.0**63), 0.1, 1.0 / 3.0,
                                        1.0, -2.5, 3.0, 7.0, 1e308, 1e-308)]
EDGE_F64_BITS += [0x7FF8000000000001, 0xFFF0000000000123,  # two NaNs, payloads and signs differ
                  bits_of(2.0**63) - 1,                     # the double below 2^63
                  bits_of(-(2.0**63)) + 1]                  # the double below -2^63 (outside the INT64 range)


def _i64(a):
    return a.view(np.int64)


def _divmod_trunc(a, b):
    """C's a / b and a % b on int64 arrays where b is neither 0 nor -1"""
    q, r = a // b, a % b  # floored: r has the sign of b
    fix = (r != 0) & ((r < 0) != (a < 0))
    return np.where(fix, q + 1, q), np.where(fix, r - b, r)


def run_program(cols, program, n):
    """-> [(is_f64, values, null)] per expression: values uint64 (I64) or float64 (F64) arrays of n rows"""
    st, out = [], []
    with np.errstate(all="ignore"):
        for term in program:
            op = term[0]
            if op == "COL":
                dt, v, valid = cols[term[1]]
                v, null = np.asarray(v), ~np.asarray(valid, dtype=bool)
                if dt == pl.FP64:
                    st.append((True, v.astype(np.float64), null))
                else:
                    assert dt in (pl.INT32, pl.INT64)
                    st.append((False, v.astype(np.int64).view(U), null))
            elif op == "INT":
                st.append((False, np.full(n, int(term[1]) % 2**64, dtype=U), np.zeros(n, bool)))
            elif op == "F64":
                x = term[1] if isinstance(term[1], float) else f64(int(term[1]))
                st.append((True, np.full(n, x, dtype=np.float64), np.zeros(n, bool)))
            elif op == "NULL":
                assert term[1] in (pl.INT64, pl.FP64)
                st.append((term[1] == pl.FP64, np.zeros(n, np.float64 if term[1] == pl.FP64 else U), np.ones(n, bool)))
            elif op in ARITH:
                (fb, b, bn), (fa, a, an) = st.pop(), st.pop()
                assert fa == fb
                null = an | bn
                if fa:
                    assert op != "MOD"
                    r = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide}[op](a, b)
                elif op in ("ADD", "SUB", "MUL"):
                    r = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply}[op](a, b)
                else:
                    sa, sb = _i64(a), _i64(b)
                    zero, minus = sb == 0, sb == -1
                    q, m = _divmod_trunc(sa, np.where(zero | minus, 1, sb))
                    q, m = np.where(minus, _i64(U(0) - a), q), np.where(minus, 0, m)
                    r = (q if op == "DIV" else m).astype(np.int64).view(U)
                    null = null | zero
                st.append((fa, r, null))
            elif op in ("NEG", "ABS"):
                fa, a, an = st.pop()
                if fa:
                    b = a.view(U)
                    r = (b ^ SIGN if op == "NEG" else b & ~SIGN).view(np.float64)
                else:
                    r = U(0) - a if op == "NEG" else np.where(_i64(a) < 0, U(0) - a, a)
                st.append((fa, r, an))
            elif op in CMPS:
                (fb, b, bn), (fa, a, an) = st.pop(), st.pop()
                assert fa == fb
                f = {"EQ": np.equal, "NEQ": np.not_equal, "LT": np.less, "GT": np.greater, "LEQ": np.less_equal, "GEQ": np.greater_equal}[op]
                r = f(a, b) if fa else f(_i64(a), _i64(b))
                st.append((False, r.astype(U), an | bn))
            elif op in ("AND", "OR"):
                (fb, b, bn), (fa, a, an) = st.pop(), st.pop()
                assert not fa and not fb
                if op == "AND":
                    decided = (~an & (a == 0)) | (~bn & (b == 0))  # a FALSE operand decides
                    null = ~decided & (an | bn)
                    r = ~decided & ~null
                else:
                    decided = (~an & (a != 0)) | (~bn & (b != 0))  # a TRUE operand decides
                    null = ~decided & (an | bn)
                    r = decided
                st.append((False, r.astype(U), null))
            elif op == "NOT":
                fa, a, an = st.pop()
                assert not fa
                st.append((False, (a == 0).astype(U), an))
            elif op in ("IS_NULL", "IS_NOT_NULL"):
                _, _, an = st.pop()
                st.append((False, (an if op == "IS_NULL" else ~an).astype(U), np.zeros(n, bool)))
            elif op == "COALESCE":
                (fb, b, bn), (fa, a, an) = st.pop(), st.pop()
                assert fa == fb
                st.append((fa, np.where(an, b, a), an & bn))
            elif op == "CASE":
                (fb, b, bn), (fa, a, an), (fc, c, cn) = st.pop(), st.pop(), st.pop()
                assert fa == fb and not fc
                take_a = ~cn & (c != 0)
                st.append((fa, np.where(take_a, a, b), np.where(take_a, an, bn)))
            elif op == "TO_I64":
                fa, a, an = st.pop()
                if fa:
                    inside = (a >= -(2.0**63)) & (a < 2.0**63)  # (False for a NaN)
                    st.append((False, np.where(inside, a, 0.0).astype(np.int64).view(U), an | ~inside))
                else:
                    st.append((False, a, an))
            elif op == "TO_F64":
                fa, a, an = st.pop()
                st.append((True, a if fa else _i64(a).astype(np.float64), an))
            elif op == "OUT":
                fa, a, an = st.pop()
                assert not st, "values left on the stack behind OUT"
                if fa:
                    a = np.where(np.isnan(a), f64(CANONICAL_NAN), a)
                out.append((fa, a, an))
            else:
                raise ValueError(op)
    assert not st
    return out


def outputs_of(node):
    return [(pl.map_func(x), pl.map_arg(x), t) for x, t in node.output_attrs]


def map_node(cols, program, outputs, n):
    """cols: the child's columns; outputs: [(MAP_COL | MAP_EXPR, index, declared type)] -> (rows, columns)"""
    exprs = run_program(cols, program, n)
    used = set()
    out = []
    for func, x, t in outputs:
        if func == pl.MAP_COL:
            assert cols[x][0] == t
            out.append((t, np.asarray(cols[x][1]) if t != pl.VARCHAR else cols[x][1], cols[x][2]))
            continue
        assert func == pl.MAP_EXPR
        fa, a, an = exprs[x]
        used.add(x)
        if fa:
            assert t == pl.FP64
            v = a
        elif t == pl.INT64:
            v = _i64(a)
        else:
            assert t == pl.INT32
            v = (a & U(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        out.append((t, np.where(an, np.zeros(1, v.dtype), v), ~an))
    assert used == set(range(len(exprs))), "an expression that no output names"
    return n, out


def children(d):
    if isinstance(d, pl.MapNode):
        return [("child", d.child)]
    return _windowref.children(d)


def evaluate(plan: pl.Plan, idx=None):
    """-> (rows, columns) of node `idx` (default: the root); columns = [(type, values, valid)]"""
    node = plan.nodes[plan.root if idx is None else idx]
    d = node.data
    if isinstance(d, pl.ScanNode):
        return plan.inputs[d.base_table_id].num_rows, _filterref._scan(plan, node)
    if isinstance(d, pl.MapNode):
        n, child = evaluate(plan, d.child)
        return map_node(child, d.program, outputs_of(node), n)
    tmp = pl.Plan()
    moved = {}
    for field, kid in children(d):
        n, cols = evaluate(plan, kid)
        moved[field] = tmp.new_scan_node(len(tmp.inputs), [(i, c[0]) for i, c in enumerate(cols)])
        tmp.new_input(_filterref.to_table(n, cols))
    tmp.nodes.append(pl.PlanNode(type(d)(**{**d.__dict__, **moved}), list(node.output_attrs)))
    tmp.root = len(tmp.nodes) - 1
    return _windowref.evaluate(tmp)


to_table = _filterref.to_table


def execute(plan: pl.Plan) -> pl.ColumnarTable:
    return to_table(*evaluate(plan))


# ------------------------------------------------------------------ programs
def depth_of(program):
    """the deepest the stack gets"""
    arity = {"COL": 0, "INT": 0, "F64": 0, "NULL": 0, "NEG": 1, "ABS": 1, "NOT": 1, "IS_NULL": 1, "IS_NOT_NULL": 1, "TO_I64": 1,
             "TO_F64": 1, "CASE": 3, "OUT": 1}
    sp = deepest = 0
    for term in program:
        sp -= arity.get(term[0], 2)
        assert sp >= 0
        if term[0] != "OUT":
            sp += 1
        deepest = max(deepest, sp)
    return deepest


def _leaf(rng, cols, want_f64):
    mine = [i for i, c in enumerate(cols) if (c[0] == pl.FP64) == want_f64 and c[0] != pl.VARCHAR]
    r = rng.random()
    if mine and r < 0.7:
        return [("COL", int(rng.choice(mine)))]
    if r < 0.95 or not mine:
        if want_f64:
            return [("F64", int(rng.choice(EDGE_F64_BITS)))] if rng.random() < 0.5 else [("F64", float(rng.integers(-8, 9)) / 4.0)]
        return [("INT", int(rng.choice(EDGE_I64)))] if rng.random() < 0.4 else [("INT", int(rng.integers(-5, 6)))]
    return [("NULL", pl.FP64 if want_f64 else pl.INT64)]


def _tree(rng, cols, want_f64, size, allow):
    """postfix ops of one value of the wanted type: about `size` ops, at most `allow` stack slots"""
    if size <= 1 or allow <= 1 and rng.random() < 0.3:
        return _leaf(rng, cols, want_f64)
    g = lambda f, s, a: _tree(rng, cols, f, s, a)
    rest = size - 1
    cut = lambda: int(rng.integers(1, rest)) if rest > 1 else 1
    forms = ["unary", "cast"]
    if allow >= 2:
        forms += ["arith", "arith", "coalesce"] + ([] if want_f64 else ["cmp", "cmp", "logic", "isnull"])
    elif not want_f64:
        forms += ["isnull", "not"]
    if allow >= 3:
        forms += ["case"]
    form = str(rng.choice(forms))
    if form == "unary":
        return g(want_f64, rest, allow) + [(str(rng.choice(["NEG", "ABS"])),)]
    if form == "not":
        return g(False, rest, allow) + [("NOT",)]
    if form == "cast":
        return g(bool(rng.integers(0, 2)), rest, allow) + [("TO_F64" if want_f64 else "TO_I64",)]
    if form == "isnull":
        return g(bool(rng.integers(0, 2)), rest, allow) + [(str(rng.choice(["IS_NULL", "IS_NOT_NULL"])),)]
    k = cut()
    if form == "arith":
        return g(want_f64, k, allow) + g(want_f64, rest - k, allow - 1) + [(str(rng.choice(ARITH[:4] if want_f64 else ARITH)),)]
    if form == "coalesce":
        return g(want_f64, k, allow) + g(want_f64, rest - k, allow - 1) + [("COALESCE",)]
    if form == "cmp":
        f = bool(rng.integers(0, 2))
        return g(f, k, allow) + g(f, rest - k, allow - 1) + [(str(rng.choice(CMPS)),)]
    if form == "logic":
        return g(False, k, allow) + g(False, rest - k, allow - 1) + [(str(rng.choice(["AND", "OR"])),)]
    third = max(1, rest // 3)
    return g(False, third, allow) + g(want_f64, third, allow - 1) + g(want_f64, max(1, rest - 2 * third), allow - 2) + [("CASE",)]


def random_program(rng, cols, n_exprs=None, max_ops=MAX_OPS, max_depth=MAX_DEPTH):
    """-> (program, [is_f64 per expression]): a well-typed program over the INT32 / INT64 / FP64 columns of
    `cols`, at most max_ops ops and max_depth stack slots"""
    n_exprs = int(rng.integers(1, 5)) if n_exprs is None else n_exprs
    prog, kinds = [], []
    for e in range(n_exprs):
        room = max_ops - len(prog) - 2 * (n_exprs - e - 1) - 1
        want = bool(rng.integers(0, 2))
        t = _tree(rng, cols, want, int(rng.integers(1, max(2, min(room, 40)))), max_depth)
        while len(t) > room:  # (a tree may come out a little above its size: shrink)
            t = _tree(rng, cols, want, max(1, room // 2), max_depth)
            room = max(room, 1)
        prog += t + [("OUT",)]
        kinds.append(want)
    assert len(prog) <= max_ops and depth_of(prog) <= max_depth
    return prog, kinds


def outputs_for(kinds, rng=None):
    """one output per expression: FP64 for an F64 one, INT64 (or, by `rng`, sometimes INT32) for an I64 one"""
    outs = []
    for e, f in enumerate(kinds):
        t = pl.FP64 if f else (pl.INT32 if rng is not None and rng.random() < 0.25 else pl.INT64)
        outs.append(("EXPR", e, t))
    return outs
