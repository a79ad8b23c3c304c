"""Set operations (RJ_NODE_SETOP) without a GPU: marshalling, the header, the sharding refusal, and the
numpy reference tests/_setopref.py pinned against a row-at-a-time second reference: a collections.Counter
over canonical tuples per side, written from the prose of include/rj.h ("Row and equality",
"Multiplicities", "Values", "Order"), not from the encoding."""
import functools
import math
import os
from collections import Counter

import numpy as np
import pytest

import _groupref
import _setopref
import test_group_plan as gp
import test_gpu_kernel_matrix as km
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
UNION_ALL, UNION, INTERSECT, INTERSECT_ALL, EXCEPT, EXCEPT_ALL = range(6)
OPS = (UNION_ALL, UNION, INTERSECT, INTERSECT_ALL, EXCEPT, EXCEPT_ALL)
OP_NAMES = ["union_all", "union", "intersect", "intersect_all", "except", "except_all"]
SORTING = OPS[1:]
rng_for, bits_of, f64_of = sp.rng_for, sp.bits_of, sp.f64_of
ROOT = os.path.join(os.path.dirname(km.LIB), "..")


def setop_plan(op, lcols, rcols, outputs):
    """Scan(lcols) <op> Scan(rcols); outputs = [(left column, right column, type)]"""
    p = pl.Plan()
    a = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
    b = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])
    p.root = p.new_setop_node(op, a, b, outputs)
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(rcols))
    return p


def empty_cols(types):
    return [(dt, np.zeros(0, km.NP_OF[dt]), np.zeros(0, bool)) for dt in types]


def random_pairs(rng, ltypes, rtypes, k):
    """k pairs of columns of one type each: any order, repeats allowed"""
    out = []
    while len(out) < k:
        lc = int(rng.integers(0, len(ltypes)))
        same = [c for c, dt in enumerate(rtypes) if dt == ltypes[lc]]
        if same:
            out.append((lc, int(rng.choice(same)), ltypes[lc]))
    return out


# ------------------------------------------------------------------ the second reference, from the prose
def cell(v):
    """a Python value as _sortref.rel_rows shows it"""
    if isinstance(v, float):
        b = bits_of(v)
        return ("f64", b - (2**64 if b >> 63 else 0))
    return v


def copies(op, l, r):
    return {UNION_ALL: l + r, UNION: 1 if l + r > 0 else 0, INTERSECT: 1 if l > 0 and r > 0 else 0, INTERSECT_ALL: min(l, r),
            EXCEPT: 1 if l > 0 and r == 0 else 0, EXCEPT_ALL: max(l - r, 0)}[op]


def by_counter(op, lrows, rrows, outputs):
    """lrows / rrows: Python rows of the children (None = NULL) -> the result rows IN ORDER, as cells"""
    types = [t for _, _, t in outputs]
    lout = [tuple(row[lc] for lc, _, _ in outputs) for row in lrows]
    rout = [tuple(row[rc] for _, rc, _ in outputs) for row in rrows]
    if op == UNION_ALL:
        return [tuple(cell(v) for v in row) for row in lout + rout]

    def canon(row):   # NULL = NULL per column, -0.0 = +0.0, NaN = NaN: the canonical value's cells name the row value
        return tuple(None if v is None else cell(gp.canon_value(v, dt)) for v, dt in zip(row, types))

    value = {}        # canonical cells -> the canonical Python row (what the comparator reads)
    for row in lout + rout:
        value.setdefault(canon(row), tuple(None if v is None else gp.canon_value(v, dt) for v, dt in zip(row, types)))
    left, right = Counter(map(canon, lout)), Counter(map(canon, rout))
    keys = [(c, 0) for c in range(len(types))]
    ordered = sorted(value, key=functools.cmp_to_key(lambda a, b: sp.compare_rows(value[a], value[b], keys, types)))
    out = []
    for k in ordered:
        out += [k] * copies(op, left[k], right[k])
    return out


TYPES = [I32, I64, F64, I32, F64]


@pytest.mark.parametrize("block", range(8))
def test_reference_agrees_with_the_counter(block):
    """10 seeded pairs of children per block, every operation on each: all three types, NULLs, heavy ties, the
    edge values of every type on both sides, reordered and repeated pairs, block 0 with empty sides —
    position by position, doubles by their bits."""
    rng = rng_for("counter", block)
    for it in range(10):
        ln, rn = int(rng.integers(0, 120)), int(rng.integers(0, 120))
        if block == 0:
            ln, rn = [(0, 0), (0, 40), (40, 0)][it % 3]
        dom = int(rng.integers(1, 4))
        lcols = sp.key_table(rng, ln, TYPES, domain=dom) if ln else empty_cols(TYPES)
        rcols = sp.key_table(rng, rn, TYPES, domain=dom) if rn else empty_cols(TYPES)
        lrows, rrows = (sp.python_rows(lcols) if ln else []), (sp.python_rows(rcols) if rn else [])
        outputs = random_pairs(rng, TYPES, TYPES, int(rng.integers(1, 5)))
        for op in OPS:
            n, out = _setopref.setop(op, lcols, ln, rcols, rn, outputs)
            want = by_counter(op, lrows, rrows, outputs)
            assert n == len(want), (OP_NAMES[op], outputs, n, len(want))
            assert _setopref.rel_rows(out, n) == want, (OP_NAMES[op], outputs)


def test_reference_rules_by_hand():
    nan, nnan = f64_of(sp.PAYLOAD_NAN), f64_of(sp.NEG_NAN)
    lcols = [(F64, np.array([0.0, nan, 1.5, 1.5, 2.0, 7.0]), np.array([1, 1, 1, 1, 0, 1], bool)), (I32, np.array([1, 1, 1, 1, 1, 1], np.int32), np.ones(6, bool))]
    rcols = [(F64, np.array([-0.0, nnan, 1.5, 3.0, 9.0]), np.array([1, 1, 1, 0, 1], bool)), (I32, np.array([1, 1, 1, 1, 2], np.int32), np.ones(5, bool))]
    outs = [(0, 0, F64), (1, 1, I32)]
    f = lambda x: ("f64", bits_of(x))
    NAN = ("f64", gp.CANON_NAN)
    rows = lambda op: _setopref.rel_rows(_setopref.setop(op, lcols, 6, rcols, 5, outs)[1])
    assert rows(INTERSECT) == [(f(0.0), 1), (f(1.5), 1), (NAN, 1), (None, 1)]           # -0.0 = +0.0, NaN = NaN, NULL = NULL
    assert rows(INTERSECT_ALL) == [(f(0.0), 1), (f(1.5), 1), (NAN, 1), (None, 1)]       # min(2, 1) copies of 1.5
    assert rows(EXCEPT) == [(f(7.0), 1)]
    assert rows(EXCEPT_ALL) == [(f(1.5), 1), (f(7.0), 1)]
    assert rows(UNION) == [(f(0.0), 1), (f(1.5), 1), (f(7.0), 1), (f(9.0), 2), (NAN, 1), (None, 1)]
    ua = rows(UNION_ALL)                                                                 # bits kept, left then right
    assert len(ua) == 11 and ua[0] == (f(0.0), 1) and ua[6] == (("f64", bits_of(-0.0) - 2**64), 1)
    assert ua[1] == (("f64", sp.PAYLOAD_NAN), 1) and ua[7] == (("f64", sp.NEG_NAN - 2**64), 1) and ua[4] == (None, 1)


@pytest.mark.parametrize("seed", range(6))
def test_identities(seed):
    rng = rng_for("identities", seed)
    ln, rn = int(rng.integers(1, 150)), int(rng.integers(0, 150))
    lcols = sp.key_table(rng, ln, TYPES, domain=2)
    rcols = sp.key_table(rng, rn, TYPES, domain=2) if rn else empty_cols(TYPES)
    outputs = random_pairs(rng, TYPES, TYPES, int(rng.integers(1, 4)))
    width = len(outputs)
    go = lambda op, a=lcols, an=ln, b=rcols, bn=rn, outs=outputs: _setopref.setop(op, a, an, b, bn, outs)
    rows = lambda r: _setopref.rel_rows(r[1], r[0])
    same = [(c, c, t) for c, (_, _, t) in enumerate(outputs)]
    # INTERSECT ALL (+) EXCEPT ALL = left, canonicalised
    left_canon = Counter(rows(go(EXCEPT_ALL, b=empty_cols(TYPES), bn=0)))
    assert Counter(rows(go(INTERSECT_ALL))) + Counter(rows(go(EXCEPT_ALL))) == left_canon
    assert sum(left_canon.values()) == ln
    # UNION = DISTINCT(UNION ALL), through the grouping reference
    un, ucols = go(UNION_ALL)
    dn, dcols = _groupref.group(ucols, [(c, 0) for c in range(width)], [(pl.AGG_KEY, c, t) for c, (_, _, t) in enumerate(outputs)], un)
    assert _groupref.rel_rows(dcols, dn) == rows(go(UNION))
    # EXCEPT = DISTINCT(left) - DISTINCT(right)
    none = empty_cols([t for _, _, t in outputs])
    ldn, ldist = go(UNION, b=empty_cols(TYPES), bn=0)
    rdn, rdist = _setopref.setop(UNION, none, 0, rcols, rn, [(c, rc, t) for c, (_, rc, t) in enumerate(outputs)])
    assert rows(_setopref.setop(EXCEPT_ALL, ldist, ldn, rdist, rdn, same)) == rows(go(EXCEPT))
    # swapping the children changes nothing for UNION / INTERSECT [ALL]
    swapped = [(rc, lc, t) for lc, rc, t in outputs]
    for op in (UNION, INTERSECT, INTERSECT_ALL):
        assert rows(go(op)) == rows(_setopref.setop(op, rcols, rn, lcols, ln, swapped)), OP_NAMES[op]


@pytest.mark.parametrize("op", SORTING, ids=OP_NAMES[1:])
def test_root_order_is_the_order_of_the_output_columns(op):
    rng = rng_for("order", op)
    lcols, rcols = sp.key_table(rng, 200, TYPES, domain=3), sp.key_table(rng, 200, TYPES, domain=3)
    outputs = [(2, 4, F64), (0, 3, I32), (1, 1, I64)]
    n, out = _setopref.evaluate(setop_plan(op, lcols, rcols, outputs))
    types = [t for _, _, t in outputs]
    got = sp.python_rows(out) if n else []
    keys = [(c, 0) for c in range(3)]
    assert n > 0
    for a, b in zip(got, got[1:]):
        r = sp.compare_rows(a, b, keys, types)
        assert r <= 0 and (r < 0 or op in (INTERSECT_ALL, EXCEPT_ALL)), (a, b)     # ascending, NULLs last; strictly without ALL


def test_reference_evaluates_nested_plans():
    """(A UNION B) EXCEPT C under a grouping, and a set operation as a join's build side"""
    rng = rng_for("nested")
    mk = lambda n: [(I32, rng.integers(0, 12, n).astype(np.int32), rng.random(n) > 0.1), (I64, rng.integers(0, 3, n))]
    A, B, Cc = mk(60), mk(50), mk(40)
    p = pl.Plan()
    a, b, c = (p.new_scan_node(i, [(0, I32), (1, I64)]) for i in range(3))
    u = p.new_setop_node(UNION, a, b, [(0, 0, I32), (1, 1, I64)])
    e = p.new_setop_node(EXCEPT, u, c, [(0, 0, I32), (1, 1, I64)])
    p.root = p.new_group_node(e, [(1, 0)], [(pl.AGG_KEY, 1, I64), (pl.AGG_COUNT_STAR, 0, I64)])
    for t in (A, B, Cc):
        p.new_input(pl.make_table(t))
    rows = lambda t: {(k if ok else None, v) for k, ok, v in zip(t[0][1].tolist(), t[0][2].tolist(), t[1][1].tolist())}
    want = Counter(v for _, v in (rows(A) | rows(B)) - rows(Cc))
    assert pl.table_rows(_setopref.execute(p)) == sorted(want.items())
    q = pl.Plan()
    a, b, c = (q.new_scan_node(i, [(0, I32), (1, I64)]) for i in range(3))
    s = q.new_setop_node(INTERSECT, a, b, [(0, 0, I32)])
    q.root = q.new_join_node(True, s, c, 0, 0, [(0, I32), (2, I64)])
    for t in (A, B, Cc):
        q.new_input(pl.make_table(t))
    keys = {k for k, _ in rows(A) if k is not None} & {k for k, _ in rows(B)}
    want = sorted((k, v) for k, ok, v in zip(Cc[0][1].tolist(), Cc[0][2].tolist(), Cc[1][1].tolist()) if ok and k in keys)
    assert sorted(pl.table_rows(_setopref.execute(q))) == want


# ------------------------------------------------------------------ interface
def test_marshalling_round_trips_the_operation_and_the_pairs():
    cols = sp.key_table(rng_for("m"), 20, [I32, I64, F64])
    p = setop_plan(EXCEPT_ALL, cols, cols, [(2, 2, F64), (0, 0, I32), (2, 2, F64)])
    cp, keep = pl.plan_to_c(p)
    nd = cp.nodes[p.root]
    assert nd.kind == pl.NODE_SETOP == 12 and nd.left == 0 and nd.right == 1 and nd.left_attr == pl.SET_EXCEPT_ALL == 5 and nd.n_out == 3
    assert [nd.out_idx[k] for k in range(3)] == [(2 << 32) | 2, 0, (2 << 32) | 2] and [nd.out_type[k] for k in range(3)] == [F64, I32, F64]
    assert pl.setop_out(3, 7) == (7 << 32) | 3 and pl.setop_lcol(pl.setop_out(3, 7)) == 3 and pl.setop_rcol(pl.setop_out(3, 7)) == 7
    assert (pl.SET_UNION_ALL, pl.SET_UNION, pl.SET_INTERSECT, pl.SET_INTERSECT_ALL, pl.SET_EXCEPT, pl.SET_EXCEPT_ALL) == OPS
    d = p.nodes[p.root].data
    assert isinstance(d, pl.SetOpNode) and (d.op, d.left, d.right) == (5, 0, 1)
    assert _setopref.outputs_of(p.nodes[p.root]) == [(2, 2, F64), (0, 0, I32), (2, 2, F64)]
    del keep


def test_header_declares_the_kind_the_operations_and_the_accessors():
    h = open(os.path.join(ROOT, "include", "rj.h")).read()
    for text in ("RJ_NODE_SETOP = 12", "RJ_SET_UNION_ALL = 0, RJ_SET_UNION = 1, RJ_SET_INTERSECT = 2", "RJ_SET_INTERSECT_ALL = 3, RJ_SET_EXCEPT = 4, "
                 "RJ_SET_EXCEPT_ALL = 5", "#define RJ_SETOP_OP(node)        ((node)->left_attr)",
                 "#define RJ_SETOP_OUT(lcol, rcol) (((uint64_t)(rcol) << 32) | (uint64_t)(uint32_t)(lcol))",
                 "#define RJ_SETOP_LCOL(x)         ((uint32_t)(x))", "#define RJ_SETOP_RCOL(x)         ((uint32_t)((uint64_t)(x) >> 32))",
                 "RJ_NODE_WINDOW / RJ_NODE_MAP /\n * RJ_NODE_SETOP"):
        assert text in h, text
    assert capi.load().rj_abi_version() == 3


def test_plan_shardable_refuses_set_operations():
    cols = sp.key_table(rng_for("s"), 50, [I32, I32], null_p=0)
    for op in OPS:
        ok, why = capi.plan_shardable(setop_plan(op, cols, cols, [(0, 0, I32)]))
        assert not ok and "RJ_NODE_SETOP" in why, OP_NAMES[op]
    q = pl.Plan()  # ... under a join
    a = q.new_scan_node(0, [(0, I32), (1, I32)])
    b = q.new_scan_node(0, [(0, I32)])
    s = q.new_setop_node(UNION_ALL, a, b, [(0, 0, I32)])
    q.root = q.new_join_node(True, s, b, 0, 0, [(0, I32)])
    q.new_input(pl.make_table(cols))
    ok, why = capi.plan_shardable(q)
    assert not ok and "RJ_NODE_SETOP" in why


def test_library_holds_the_setop_kernels_and_documents_its_switch():
    import _elfsyms
    names = {_elfsyms.short_name(n) for n in _elfsyms.kernel_handles(km.LIB)}
    assert {"k_setop_concat<4>", "k_setop_concat<8>", "k_setop_left", "k_setop_scan", "k_setop_runs", "k_setop_mult", "k_setop_offsets",
            "k_setop_emit"} == {n for n in names if n.startswith("k_setop_")}
    hpp = open(os.path.join(ROOT, "radix-join_amd", "csrc", "rj_device.hpp")).read()
    assert "constexpr int SETOP_TILE = GROUP_TILE;" in hpp
    assert "RJ_TUNE_SETOP_GRID" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    log = open(os.path.join(ROOT, "profiles", "setop_codeobj.log")).read()
    for k in ("k_setop_concat", "k_setop_left", "k_setop_scan", "k_setop_runs", "k_setop_mult", "k_setop_offsets", "k_setop_emit"):
        assert k in log, k
    assert log.count("ScratchSize [bytes/lane]: 0") == log.count("ScratchSize [bytes/lane]:") >= 8
