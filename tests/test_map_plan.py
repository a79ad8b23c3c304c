"""Map nodes (RJ_NODE_MAP) on the CPU: the numpy reference tests/_mapref.py is pinned two ways — against a
row-at-a-time evaluator written here with Python ints and struct (eval_row), and against
rj_debug_map_eval, which validates a program with the executor's code and evaluates it on one row
through the op functions the kernel calls (csrc/rj_expr.hpp).  No GPU is needed.

The grid: every op on every type over EDGE_I64 / EDGE_F64 (tests/_mapref.py) with NULL in every operand
position, the Kleene tables, the division and cast edges of rj.h, INT32 truncation of a declared type,
300 seeded random programs up to the op and depth limits, and one case per line of the error contract
that concerns the program (the lines about a node's outputs need the executor: tests/test_gpu_map.py)."""
import math
import os
import zlib

import numpy as np
import pytest

import _mapref
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
ARG, UNSUPPORTED = 1, 5
M64 = 2**64 - 1
f64, bits_of = _mapref.f64, _mapref.bits_of
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rng_for(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def signed(u):
    return u - 2**64 if u >= 2**63 else u


# ------------------------------------------------------------------ the row-at-a-time evaluator
def _fdiv(x, y):
    if y != 0.0 or math.isnan(x) or math.isnan(y):
        return x / y if y != 0.0 else float("nan")
    if x == 0.0:
        return float("nan")
    return math.copysign(float("inf"), x) * math.copysign(1.0, y)


def _cmp(op, x, y):
    return {"EQ": x == y, "NEQ": x != y, "LT": x < y, "GT": x > y, "LEQ": x <= y, "GEQ": x >= y}[op]


def eval_row(program, row):
    """row: [(dtype, bits as an unsigned number, is_null)] -> [(is_f64, bits, is_null)] per expression; the
    bits of a NULL are 0.  Integers are Python ints reduced modulo 2^64, doubles go through struct."""
    st, out = [], []
    for term in program:
        op = term[0]
        if op == "COL":
            dt, b, nul = row[term[1]]
            if dt == I32:
                b = (b & 0xFFFFFFFF) - (2**32 if b & 0x80000000 else 0)
            st.append((dt == F64, b & M64, nul))
        elif op == "INT":
            st.append((False, int(term[1]) & M64, False))
        elif op == "F64":
            st.append((True, bits_of(term[1]) if isinstance(term[1], float) else int(term[1]) & M64, False))
        elif op == "NULL":
            st.append((term[1] == F64, 0, True))
        elif op in _mapref.ARITH:
            (fb, b, bn), (fa, a, an) = st.pop(), st.pop()
            assert fa == fb
            nul = an or bn
            if fa:
                x, y = f64(a), f64(b)
                r = bits_of({"ADD": lambda: x + y, "SUB": lambda: x - y, "MUL": lambda: x * y, "DIV": lambda: _fdiv(x, y)}[op]())
            elif op in ("ADD", "SUB", "MUL"):
                r = {"ADD": a + b, "SUB": a - b, "MUL": a * b}[op] & M64
            else:
                x, y = signed(a), signed(b)
                if y == 0:
                    r, nul = 0, True
                else:
                    q = abs(x) // abs(y) * (1 if (x < 0) == (y < 0) else -1)  # truncation toward zero
                    r = (q if op == "DIV" else x - q * y) & M64
            st.append((fa, r, nul))
        elif op in ("NEG", "ABS"):
            fa, a, an = st.pop()
            if fa:
                r = a ^ (1 << 63) if op == "NEG" else a & ~(1 << 63) & M64
            else:
                r = (-signed(a) if op == "NEG" else abs(signed(a))) & M64
            st.append((fa, r, an))
        elif op in _mapref.CMPS:
            (fb, b, bn), (fa, a, an) = st.pop(), st.pop()
            assert fa == fb
            st.append((False, int(_cmp(op, f64(a), f64(b)) if fa else _cmp(op, signed(a), signed(b))), an or bn))
        elif op in ("AND", "OR"):
            (_, b, bn), (_, a, an) = st.pop(), st.pop()
            ta, tb = (None if an else a != 0), (None if bn else b != 0)  # SQL's three values
            if op == "AND":
                r = False if (ta is False or tb is False) else (None if (ta is None or tb is None) else True)
            else:
                r = True if (ta is True or tb is True) else (None if (ta is None or tb is None) else False)
            st.append((False, int(bool(r)), r is None))
        elif op == "NOT":
            _, a, an = st.pop()
            st.append((False, int(a == 0), an))
        elif op in ("IS_NULL", "IS_NOT_NULL"):
            _, _, an = st.pop()
            st.append((False, int(an == (op == "IS_NULL")), False))
        elif op == "COALESCE":
            b, a = st.pop(), st.pop()
            assert a[0] == b[0]
            st.append(b if a[2] else a)
        elif op == "CASE":
            b, a, c = st.pop(), st.pop(), st.pop()
            assert a[0] == b[0] and not c[0]
            st.append(a if (not c[2] and c[1] != 0) else b)
        elif op == "TO_I64":
            fa, a, an = st.pop()
            if fa:
                x = f64(a)
                inside = not math.isnan(x) and -(2.0**63) <= x < 2.0**63
                st.append((False, int(x) & M64 if inside else 0, an or not inside))
            else:
                st.append((False, a, an))
        elif op == "TO_F64":
            fa, a, an = st.pop()
            st.append((True, a if fa else bits_of(float(signed(a))), an))
        else:
            assert op == "OUT"
            fa, a, an = st.pop()
            assert not st
            if fa and math.isnan(f64(a)):
                a = _mapref.CANONICAL_NAN
            out.append((fa, 0 if an else a, an))
    return out


# ------------------------------------------------------------------ the three evaluators side by side
def columns_of(rows, types):
    """rows of (bits | None) -> the (type, values, valid) columns _mapref takes"""
    cols = []
    for c, dt in enumerate(types):
        bits = np.array([0 if r[c] is None else r[c] & M64 for r in rows], dtype=np.uint64)
        valid = np.array([r[c] is not None for r in rows], dtype=bool)
        v = bits.view(np.float64) if dt == F64 else (bits.view(np.int64) if dt == I64 else bits.astype(np.uint32).view(np.int32))
        cols.append((dt, v, valid))
    return cols


def ref_bits(cols, program, n):
    """_mapref on the columns -> per expression (is_f64, [bits], [is_null]), the bits of a NULL 0"""
    out = []
    for fa, a, an in _mapref.run_program(cols, program, n):
        b = np.ascontiguousarray(a).view(np.uint64)
        out.append((fa, np.where(an, np.uint64(0), b).tolist(), an.tolist()))
    return out


def agree(program, rows, types, debug=True):
    """the reference, the row evaluator and (debug) rj_debug_map_eval on every row -> the reference's answer"""
    ref = ref_bits(columns_of(rows, types), program, len(rows))
    for i, r in enumerate(rows):
        row = [(dt, 0 if b is None else b & M64, b is None) for dt, b in zip(types, r)]
        want = eval_row(program, row)
        got = [(fa, bs[i], ns[i]) for fa, bs, ns in ref]
        assert got == want, (program, row, got, want)
        if debug:
            dev = [(k == F64, b, nul) for k, b, nul in capi.map_eval(program, row)]
            assert dev == want, (program, row, dev, want)
    return ref


I_EDGES = [v & M64 for v in _mapref.EDGE_I64] + [None]
F_EDGES = list(_mapref.EDGE_F64_BITS) + [None]
I32_EDGES = [v & 0xFFFFFFFF for v in (-(2**31), -1, 0, 1, 2**31 - 1, 7)] + [None]
pairs = lambda edges: [(a, b) for a in edges for b in edges]


@pytest.mark.parametrize("op", _mapref.ARITH + _mapref.CMPS + ("AND", "OR", "COALESCE"))
def test_binary_op_on_integers_over_the_edge_grid(op):
    agree([("COL", 0), ("COL", 1), (op,), ("OUT",)], pairs(I_EDGES), [I64, I64])
    agree([("COL", 0), ("COL", 1), (op,), ("OUT",)], pairs(I32_EDGES), [I32, I32])


@pytest.mark.parametrize("op", _mapref.ARITH[:4] + _mapref.CMPS + ("COALESCE",))
def test_binary_op_on_doubles_over_the_edge_grid(op):
    agree([("COL", 0), ("COL", 1), (op,), ("OUT",)], pairs(F_EDGES), [F64, F64])


@pytest.mark.parametrize("op", ["NEG", "ABS", "NOT", "IS_NULL", "IS_NOT_NULL", "TO_I64", "TO_F64"])
def test_unary_op_on_every_type_over_the_edge_grid(op):
    agree([("COL", 0), (op,), ("OUT",)], [(a,) for a in I_EDGES], [I64])
    agree([("COL", 0), (op,), ("OUT",)], [(a,) for a in I32_EDGES], [I32])
    if op != "NOT":
        agree([("COL", 0), (op,), ("OUT",)], [(a,) for a in F_EDGES], [F64])


def test_case_with_null_in_every_operand_position():
    conds = [None, 0, 1, (-5) & M64, 1 << 63]
    vals = [None, 0, 7, M64]
    rows = [(c, a, b) for c in conds for a in vals for b in vals]
    ref = agree([("COL", 0), ("COL", 1), ("COL", 2), ("CASE",), ("OUT",)], rows, [I64, I64, I64])
    agree([("COL", 0), ("COL", 1), ("COL", 2), ("CASE",), ("OUT",)],
          [(c, a, b) for c in conds for a in F_EDGES[:6] + [None] for b in (bits_of(2.5), None)], [I64, F64, F64])
    i = rows.index((None, 7, M64))  # a NULL condition takes b
    assert (ref[0][1][i], ref[0][2][i]) == (M64, False)


def test_literals_and_typed_nulls():
    got = capi.map_eval([("INT", -3), ("OUT",), ("F64", -0.0), ("OUT",), ("F64", 0x7FF8000000000009), ("OUT",), ("NULL", I64), ("OUT",),
                         ("NULL", F64), ("OUT",), ("INT", 2**64 - 1), ("OUT",)], [])
    assert got == [(I64, M64 - 2, False), (F64, 1 << 63, False), (F64, _mapref.CANONICAL_NAN, False), (I64, 0, True), (F64, 0, True),
                   (I64, M64, False)]
    agree([("INT", -3), ("OUT",), ("F64", -0.0), ("OUT",), ("NULL", F64), ("OUT",), ("NULL", I64), ("IS_NULL",), ("OUT",)], [()], [])


def test_the_kleene_tables():
    N, rows = None, [(a, b) for a in (None, 0, 1) for b in (None, 0, 1)]
    ref = agree([("COL", 0), ("COL", 1), ("AND",), ("OUT",), ("COL", 0), ("COL", 1), ("OR",), ("OUT",), ("COL", 0), ("NOT",), ("OUT",)],
                rows, [I64, I64])
    val = lambda e, i: None if ref[e][2][i] else ref[e][1][i]
    AND = {(N, N): N, (N, 0): 0, (N, 1): N, (0, N): 0, (0, 0): 0, (0, 1): 0, (1, N): N, (1, 0): 0, (1, 1): 1}
    OR = {(N, N): N, (N, 0): N, (N, 1): 1, (0, N): N, (0, 0): 0, (0, 1): 1, (1, N): 1, (1, 0): 1, (1, 1): 1}
    for i, r in enumerate(rows):
        assert val(0, i) == AND[r] and val(1, i) == OR[r] and val(2, i) == {N: N, 0: 1, 1: 0}[r[0]], r


def test_the_division_and_cast_edges_of_the_contract():
    MIN, MAX = 1 << 63, 2**63 - 1
    one = lambda prog, row: capi.map_eval(prog + [("OUT",)], row)[0]
    i = lambda v: (I64, v & M64, False)
    d = lambda x: (F64, bits_of(x) if isinstance(x, float) else x, False)
    bin_ = lambda op: [("COL", 0), ("COL", 1), (op,)]
    assert one(bin_("DIV"), [i(MIN), i(-1)]) == (I64, MIN, False) and one(bin_("MOD"), [i(MIN), i(-1)]) == (I64, 0, False)
    assert one(bin_("DIV"), [i(7), i(0)])[2] and one(bin_("MOD"), [i(MIN), i(0)])[2]              # a zero divisor: NULL
    assert one(bin_("DIV"), [i(-7), i(2)]) == (I64, (-3) & M64, False) and one(bin_("MOD"), [i(-7), i(2)]) == (I64, M64, False)
    assert one(bin_("DIV"), [i(7), i(-2)]) == (I64, (-3) & M64, False) and one(bin_("MOD"), [i(7), i(-2)]) == (I64, 1, False)
    assert one([("COL", 0), ("NEG",)], [i(MIN)]) == (I64, MIN, False) and one([("COL", 0), ("ABS",)], [i(MIN)]) == (I64, MIN, False)
    assert one(bin_("ADD"), [i(MAX), i(1)]) == (I64, MIN, False) and one(bin_("MUL"), [i(MIN), i(3)]) == (I64, MIN, False)
    assert one(bin_("DIV"), [d(1.0), d(0.0)]) == (F64, bits_of(float("inf")), False)                # x / 0.0 is not NULL
    assert one(bin_("DIV"), [d(-1.0), d(0.0)]) == (F64, bits_of(float("-inf")), False)
    assert one(bin_("DIV"), [d(0.0), d(0.0)]) == (F64, _mapref.CANONICAL_NAN, False)
    assert one(bin_("DIV"), [d(1.0), d(3.0)]) == (F64, 0x3FD5555555555555, False)                   # correctly rounded
    assert one(bin_("DIV"), [d(2.0), d(3.0)]) == (F64, 0x3FE5555555555555, False)
    assert one(bin_("MUL"), [d(5e-324), d(0.5)]) == (F64, 0, False) and one(bin_("MUL"), [d(5e-324), d(2.0)]) == (F64, 2, False)
    assert one([("COL", 0), ("NEG",)], [d(0.0)]) == (F64, 1 << 63, False)                           # -0.0 stays -0.0
    assert one([("COL", 0), ("ABS",)], [d(0xFFF8000000000001)]) == (F64, _mapref.CANONICAL_NAN, False)
    assert one([("COL", 0), ("TO_F64",)], [i(2**53 + 1)]) == (F64, bits_of(2.0**53), False)         # ties to even
    assert one([("COL", 0), ("TO_F64",)], [i(2**53 + 3)]) == (F64, bits_of(2.0**53 + 4), False)
    assert one([("COL", 0), ("TO_F64",)], [i(MAX)]) == (F64, bits_of(2.0**63), False)
    assert one([("COL", 0), ("TO_I64",)], [d(-2.9)]) == (I64, (-2) & M64, False) and one([("COL", 0), ("TO_I64",)], [d(2.9)]) == (I64, 2, False)
    assert one([("COL", 0), ("TO_I64",)], [d(-(2.0**63))]) == (I64, MIN, False)
    assert one([("COL", 0), ("TO_I64",)], [d(bits_of(2.0**63) - 1)]) == (I64, 2**63 - 1024, False)
    for x in (2.0**63, float("inf"), float("-inf"), float("nan"), bits_of(-(2.0**63)) + 1):
        assert one([("COL", 0), ("TO_I64",)], [d(x)]) == (I64, 0, True), x
    assert one([("COL", 0), ("TO_I64",)], [(I32, 0xFFFFFFFF, False)]) == (I64, M64, False)         # INT32 sign-extends
    assert one([("COL", 0), ("TO_F64",)], [d(0x7FF0000000000001)]) == (F64, _mapref.CANONICAL_NAN, False)


def test_a_declared_int32_keeps_the_low_32_bits():
    vals = np.array([2**31, -(2**31) - 1, 2**32 + 5, -1, 2**63 - 1, -(2**63), 0], dtype=np.int64)
    cols = [(I64, vals, np.array([1, 1, 1, 1, 1, 1, 0], bool))]
    n, out = _mapref.map_node(cols, [("COL", 0), ("INT", 0), ("ADD",), ("OUT",)], [(pl.MAP_EXPR, 0, I32), (pl.MAP_EXPR, 0, I64), (pl.MAP_COL, 0, I64)], 7)
    assert out[0][0] == I32 and out[0][1].dtype == np.int32 and out[0][1].tolist() == [-(2**31), 2**31 - 1, 5, -1, -1, 0, 0]
    assert out[0][2].tolist() == out[1][2].tolist() == [True] * 6 + [False] and out[1][1].tolist()[:6] == vals.tolist()[:6]
    for v in vals.tolist():
        (_, b, _), = eval_row([("COL", 0), ("OUT",)], [(I64, v & M64, False)])
        assert (b & 0xFFFFFFFF) == (v & 0xFFFFFFFF)


# ------------------------------------------------------------------ random programs
TYPES = [I32, I64, I64, F64, F64]


def random_rows(rng, n):
    pick = lambda edges, p_null=0.15: None if rng.random() < p_null else edges[int(rng.integers(0, len(edges)))]
    small = [v & M64 for v in range(-4, 5)]
    fsmall = [bits_of(v) for v in (0.5, -1.25, 3.0, 1e-3, -7.0, 2.0**40)]
    return [(pick(I32_EDGES[:-1]), pick(I_EDGES[:-1] + small), pick(small), pick(F_EDGES[:-1] + fsmall), pick(fsmall)) for _ in range(n)]


@pytest.mark.parametrize("block", range(10))
def test_random_programs(block):
    """30 seeded programs per block (300 in all) over 24 rows of edge values; every block holds a program at
    the op limit, block 0 one at the depth limit too"""
    rng = rng_for("programs", block)
    rows = random_rows(rng, 24)
    cols = columns_of(rows, TYPES)
    deepest = longest = 0
    for k in range(30):
        prog, _ = _mapref.random_program(rng, cols, n_exprs=8 if k == 0 else None)
        if k == 1:
            prog = op_limit_program()
        if k == 2 and block == 0:
            prog = depth_limit_program()
        deepest, longest = max(deepest, _mapref.depth_of(prog)), max(longest, len(prog))
        agree(prog, rows, TYPES, debug=k < 10 or k % 5 == 0)
    assert longest == _mapref.MAX_OPS and deepest >= (8 if block == 0 else 3)


def op_limit_program():
    """128 ops: ((c1 + 1) + 1 ...) then OUT, twice"""
    one = [("COL", 1)] + [("INT", 1), ("ADD",)] * 31 + [("OUT",)]
    prog = one + one
    assert len(prog) == _mapref.MAX_OPS
    return prog


def depth_limit_program():
    """c1 + (c1 + (... + c1)): eight values on the stack before the first ADD"""
    prog = [("COL", 1)] * 8 + [("ADD",)] * 7 + [("OUT",)]
    assert _mapref.depth_of(prog) == _mapref.MAX_DEPTH
    return prog


# ------------------------------------------------------------------ the error contract of a program
ROW = [(I32, 1, False), (I64, 2, False), (F64, bits_of(1.5), False), (VC, 0, False)]


def _error(prog, row=ROW):
    with pytest.raises(capi.RjError) as e:
        capi.map_eval(prog, row)
    return e.value.code, str(e.value)


def test_error_contract_of_the_program(monkeypatch):
    monkeypatch.setitem(capi.X_OPS, "BOGUS", 27)
    monkeypatch.setitem(capi.X_OPS, "BOGUS2", -1)
    O = ("OUT",)
    for prog, text in (([("BOGUS",), O], "opcode"), ([("BOGUS2",), O], "opcode"),
                       ([("COL", 4), O], "out of range"), ([("COL", -1), O], "out of range"),
                       ([("COL", 0), ("COL", 2), ("ADD",), O], "different types"), ([("COL", 1), ("COL", 2), ("LT",), O], "different types"),
                       ([("COL", 1), ("COL", 2), ("COALESCE",), O], "different types"),
                       ([("COL", 0), ("COL", 1), ("COL", 2), ("CASE",), O], "different types"),
                       ([("COL", 2), ("COL", 1), ("AND",), O], "integer"), ([("COL", 1), ("COL", 2), ("OR",), O], "integer"),
                       ([("COL", 2), ("NOT",), O], "integer"), ([("COL", 2), ("COL", 1), ("COL", 1), ("CASE",), O], "integer"),
                       ([("COL", 2), ("COL", 2), ("MOD",), O], "MOD on F64"),
                       ([("NULL", I32), O], "RJ_X_NULL"), ([("NULL", VC), O], "RJ_X_NULL"), ([("NULL", 9), O], "RJ_X_NULL"),
                       ([("ADD",), O], "underflow"), ([("COL", 0), ("ADD",), O], "underflow"), ([O], "underflow"),
                       ([("COL", 0), ("NEG",), ("CASE",), O], "underflow"),
                       ([("COL", 0), ("COL", 1), O], "left on the stack"), ([("COL", 0), O, ("COL", 1), ("COL", 1), O], "left on the stack"),
                       ([("COL", 0)], "does not end in RJ_X_OUT"), ([("COL", 0), O, ("COL", 1), ("NEG",)], "does not end in RJ_X_OUT")):
        code, msg = _error(prog)
        assert code == ARG and text in msg, (prog, msg)
    # ---- RJ_ERR_UNSUPPORTED
    code, msg = _error([("COL", 3), O])
    assert code == UNSUPPORTED and "VARCHAR" in msg
    code, msg = _error([("COL", 3), ("IS_NULL",), O])
    assert code == UNSUPPORTED and "VARCHAR" in msg
    code, msg = _error([("COL", 1)] + [("NEG",)] * 127 + [O])
    assert code == UNSUPPORTED and "128" in msg
    assert len(capi.map_eval([("COL", 1)] + [("NEG",)] * 126 + [O], ROW)) == 1  # (128 ops are fine)
    code, msg = _error([("COL", 1)] * 9 + [("ADD",)] * 8 + [O])
    assert code == UNSUPPORTED and "deeper than 8" in msg
    assert capi.map_eval(depth_limit_program(), ROW) == [(I64, 16, False)]      # (eight slots are fine)
    assert capi.map_eval([], ROW) == []                                         # no op at all: nothing to compute


def test_ops_without_a_program_pointer_are_an_argument_error():
    import ctypes as C
    L = capi.load()
    capi.map_eval([], [])  # (sets the argtypes)
    n_out = C.c_uint64(7)
    rc = L.rj_debug_map_eval(None, 3, 0, None, None, None, 0, None, None, None, C.byref(n_out))
    L.rj_last_error.restype, L.rj_last_error.argtypes = C.c_char_p, [C.c_void_p]
    assert rc == ARG and b"NULL program pointer" in L.rj_last_error(None) and n_out.value == 0


# ------------------------------------------------------------------ the plan side
def map_plan(cols, program, outputs):
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    p.root = p.new_map_node(sc, program, outputs)
    p.new_input(pl.make_table(cols))
    return p


def test_plan_to_c_marshals_the_node():
    cols = columns_of(random_rows(rng_for("c"), 5), TYPES)
    prog = [("COL", 1), ("COL", 2), ("MUL",), ("OUT",), ("COL", 3), ("F64", 0.5), ("ADD",), ("OUT",)]
    p = map_plan(cols, prog, [("EXPR", 1, F64), ("COL", 0, I32), ("EXPR", 0, I32), (pl.MAP_EXPR, 0, I64)])
    cplan, keep = pl.plan_to_c(p)
    nd = cplan.nodes[p.root]
    assert nd.kind == pl.NODE_MAP == 11 and nd.left == 0 and nd.right == 8 and nd.right_attr != 0 and nd.n_out == 4
    assert [nd.out_idx[k] for k in range(4)] == [(1 << 56) | 1, 0, 1 << 56, 1 << 56] and [nd.out_type[k] for k in range(4)] == [F64, I32, I32, I64]
    ops, n = capi.expr_to_c(prog)
    assert n == 8 and [(ops[k].op, ops[k].column) for k in (0, 2, 3)] == [(0, 1), (6, 0), (26, 0)] and ops[5].ivalue == bits_of(0.5)
    q = map_plan(cols, [], [("COL", 4, F64)])
    cq, keep2 = pl.plan_to_c(q)
    assert cq.nodes[q.root].right == 0 and cq.nodes[q.root].right_attr == 0
    del keep, keep2


def test_reference_composes_with_the_other_kinds():
    """SUM(a * b) GROUP BY k as MAP + GROUP, and a map over a sort keeps the sort's order"""
    rng = rng_for("compose")
    n = 200
    cols = [(I32, rng.integers(0, 7, n).astype(np.int32)), (I64, rng.integers(-9, 9, n)), (I64, rng.integers(-9, 9, n), rng.random(n) > 0.2)]
    p = pl.Plan()
    sc = p.new_scan_node(0, [(0, I32), (1, I64), (2, I64)])
    m = p.new_map_node(sc, [("COL", 1), ("COL", 2), ("MUL",), ("OUT",)], [("COL", 0, I32), ("EXPR", 0, I64)])
    p.root = p.new_group_node(m, [(0, 0)], [(pl.AGG_KEY, 0, I32), (pl.AGG_SUM, 1, I64)])
    p.new_input(pl.make_table(cols))
    want = {}
    for k, a, b, ok in zip(cols[0][1].tolist(), cols[1][1].tolist(), cols[2][1].tolist(), cols[2][2].tolist()):
        want.setdefault(k, []).extend([a * b] if ok else [])
    assert pl.table_rows(_mapref.execute(p)) == [(k, sum(v) if v else None) for k, v in sorted(want.items())]
    q = pl.Plan()
    sc = q.new_scan_node(0, [(0, I32), (1, I64)])
    s = q.new_sort_node(sc, [(1, pl.SORT_DESC), (0, 0)], [(0, I32), (1, I64)], limit=20)
    q.root = q.new_map_node(s, [("COL", 1), ("NEG",), ("OUT",)], [("EXPR", 0, I64), ("COL", 0, I32)])
    q.new_input(pl.make_table(cols[:2]))
    rows = pl.table_rows(_mapref.execute(q))
    assert rows == [(-a, k) for k, a in sorted(zip(cols[0][1].tolist(), cols[1][1].tolist()), key=lambda r: (-r[1], r[0]))[:20]]


def test_plan_shardable_refuses_map_nodes():
    cols = columns_of(random_rows(rng_for("s"), 5), TYPES)
    ok, why = capi.plan_shardable(map_plan(cols, [("COL", 0), ("OUT",)], [("EXPR", 0, I64)]))
    assert not ok and "RJ_NODE_MAP" in why
    q = pl.Plan()  # ... under a join
    a = q.new_scan_node(0, [(0, I32), (1, I64)])
    m = q.new_map_node(a, [], [("COL", 0, I32)])
    b = q.new_scan_node(0, [(0, I32)])
    q.root = q.new_join_node(True, m, b, 0, 0, [(0, I32)])
    q.new_input(pl.make_table(cols))
    ok, why = capi.plan_shardable(q)
    assert not ok and "RJ_NODE_MAP" in why


def test_header_library_and_documents():
    h = open(os.path.join(ROOT, "include", "rj.h")).read()
    for text in ("RJ_NODE_MAP = 11", "#define RJ_MAP_N_OPS(node) ((node)->right)",
                 "#define RJ_MAP_OPS(node) ((const rj_expr_op*)(uintptr_t)(node)->right_attr)", "#define RJ_MAP_MAX_OPS 128",
                 "#define RJ_MAP_MAX_DEPTH 8", "#define RJ_MAP_OUT(func, x) (((uint64_t)(func) << 56) | (uint64_t)(x))",
                 "typedef struct rj_expr_op {", "RJ_X_OUT = 26", "int rj_debug_map_eval("):
        assert text in h, text
    for name, code in capi.X_OPS.items():
        assert f"RJ_X_{name} = {code}" in h, name
    assert capi.load().rj_abi_version() == 3
    import _elfsyms
    lib = os.path.join(ROOT, "radix-join_amd", "librj.so")
    assert {"k_map"} == {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(lib)) if n.split("<")[0].startswith("k_map")}
    hpp = open(os.path.join(ROOT, "radix-join_amd", "csrc", "rj_expr.hpp")).read()
    assert "constexpr int MAP_TILE = 4096;" in hpp and "#pragma clang fp contract(off)" in hpp
    assert "RJ_TUNE_MAP_GRID" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    log = open(os.path.join(ROOT, "profiles", "map_codeobj.log")).read()
    assert "k_map" in log and "ScratchSize [bytes/lane]: 0" in log
