"""Sort nodes (RJ_NODE_SORT) without a GPU: marshalling, the header, the sharding refusal, the host
side of the key encoding (rj_debug_sort_key), and the numpy reference tests/_sortref.py pinned against
a row-at-a-time second reference: Python's sorted() with functools.cmp_to_key over a comparator that
is written from the prose of include/rj.h ("Semantics"), not from the encoding."""
import ctypes as C
import functools
import itertools
import math
import os
import struct
import zlib

import numpy as np
import pytest

import _sortref
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
ALL_FLAGS = (0, DESC, NF, DESC | NF)


def rng_for(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


f64_of = lambda bits: struct.unpack("<d", struct.pack("<Q", bits & (2**64 - 1)))[0]
bits_of = lambda x: struct.unpack("<Q", struct.pack("<d", x))[0]

# the edge list of every type, as (python value, its bits as an unsigned number); None = NULL
DBL_MAX, DENORM = 1.7976931348623157e308, 5e-324
QNAN, SNAN, NEG_NAN, PAYLOAD_NAN = 0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000000, 0x7FFFFFFFFFFFFFFF
EDGES = {
    I32: [(v, v & (2**32 - 1)) for v in (-2**31, -1, 0, 1, 2**31 - 1)] + [(None, 0)],
    I64: [(v, v & (2**64 - 1)) for v in (-2**63, -1, 0, 1, 2**63 - 1)] + [(None, 0)],
    F64: [(x, bits_of(x)) for x in (-math.inf, -DBL_MAX, -DENORM, -0.0, 0.0, DENORM, 1.0, DBL_MAX, math.inf)]
         + [(f64_of(b), b) for b in (QNAN, SNAN, NEG_NAN, PAYLOAD_NAN)] + [(None, 0)],
}


# ------------------------------------------------------------------ the second reference, from the prose
def compare_values(a, b, dt):
    """-1 / 0 / 1 for two non-NULL values: INT32 / INT64 by value; FP64 numerically, -0.0 = +0.0, every
    NaN equal to every other NaN and greater than +inf."""
    if dt == F64:
        an, bn = math.isnan(a), math.isnan(b)
        if an or bn:
            return 0 if an and bn else (1 if an else -1)
    return (a > b) - (a < b)


def compare_rows(ra, rb, keys, types):
    """Lexicographic over keys = [(column, flags)], the first most significant; NULLs last unless
    NULLS_FIRST, wherever DESC puts the values."""
    for c, flags in keys:
        a, b = ra[c], rb[c]
        if a is None or b is None:
            if a is None and b is None:
                continue
            first = a is None          # is `ra` the NULL one?
            return (-1 if first else 1) * (1 if flags & NF else -1)
        r = compare_values(a, b, types[c])
        if r:
            return -r if flags & DESC else r
    return 0


def sorted_by_comparator(rows, keys, types, limit=None, offset=0):
    """-> row positions: sorted() is stable, so ties keep the input order."""
    idx = sorted(range(len(rows)), key=functools.cmp_to_key(lambda i, j: compare_rows(rows[i], rows[j], keys, types)))
    begin, count = _sortref.slice_of(len(rows), limit, offset)
    return idx[begin:begin + count]


def key_table(rng, n, types, null_p=0.15, domain=6):
    """Small domains (heavy ties) plus the edge values of every type, NULLs in every column."""
    cols = []
    for dt in types:
        if dt == F64:
            v = rng.integers(-domain, domain, n).astype(np.float64) * 0.5
            edge = np.array([b for _, b in EDGES[F64][:-1]], dtype=np.uint64).view(np.float64)
        else:
            v = rng.integers(-domain, domain, n).astype(km.NP_OF[dt])
            edge = np.array([x for x, _ in EDGES[dt][:-1]], dtype=km.NP_OF[dt])
        at = rng.choice(n, min(n, edge.shape[0]), replace=False)
        v[at] = edge[: at.shape[0]]
        cols.append((dt, v, rng.random(n) >= null_p))
    return cols


def python_rows(cols):
    """rows with Python values (floats as floats: what the comparator reads), None = NULL"""
    n = cols[0][1].shape[0]
    return [tuple(c[1][r].item() if c[2][r] else None for c in cols) for r in range(n)]


def sort_plan(cols, keys, outs=None, limit=None, offset=0):
    """Scan(cols) -> SORT keys; outs: child columns in output order (default: all)."""
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    outs = range(len(cols)) if outs is None else outs
    p.root = p.new_sort_node(sc, keys, [(i, cols[i][0]) for i in outs], limit, offset)
    p.new_input(pl.make_table(cols))
    return p


# ------------------------------------------------------------------ interface
def test_marshalling_round_trips_keys_limit_and_offset():
    cols = key_table(rng_for("m"), 20, [I32, I64, F64])
    p = sort_plan(cols, [(2, DESC), (0, NF), (2, 0)], outs=[1, 1, 0], limit=7, offset=3)
    cp, keep = pl.plan_to_c(p)
    nd = cp.nodes[p.root]
    assert nd.kind == pl.NODE_SORT == 8 and nd.left == 0 and nd.n_out == 3
    assert nd.right == 3 and nd.right_attr != 0 and nd.left_attr == 7 and nd.base_table_id == 3
    ks = C.cast(C.c_void_p(nd.right_attr), C.POINTER(pl.rj_sort_key))
    assert [(ks[k].column, ks[k].flags) for k in range(3)] == [(2, 1), (0, 2), (2, 0)]
    assert [nd.out_idx[k] for k in range(3)] == [1, 1, 0] and [nd.out_type[k] for k in range(3)] == [I64, I64, I32]
    assert C.sizeof(pl.rj_sort_key) == 8
    # no keys, no limit: a NULL pointer and RJ_SORT_NO_LIMIT
    cp2, keep2 = pl.plan_to_c(sort_plan(cols, []))
    nd = cp2.nodes[1]
    assert nd.kind == 8 and nd.right == 0 and nd.right_attr == 0 and nd.left_attr == 2**64 - 1 == pl.SORT_NO_LIMIT
    assert nd.base_table_id == 0
    assert (pl.SORT_DESC, pl.SORT_NULLS_FIRST) == (1, 2)
    del keep, keep2


def test_header_declares_the_kind_the_flags_and_the_accessors():
    h = open(os.path.join(os.path.dirname(km.LIB), "..", "include", "rj.h")).read()
    for text in ("RJ_NODE_SORT = 8", "#define RJ_SORT_DESC 1", "#define RJ_SORT_NULLS_FIRST 2", "#define RJ_SORT_MAX_KEYS 8",
                 "#define RJ_SORT_NO_LIMIT UINT64_MAX", "#define RJ_SORT_N_KEYS(node) ((node)->right)",
                 "#define RJ_SORT_KEYS(node) ((const rj_sort_key*)(uintptr_t)(node)->right_attr)",
                 "#define RJ_SORT_LIMIT(node) ((node)->left_attr)", "#define RJ_SORT_OFFSET(node) ((node)->base_table_id)",
                 "typedef struct rj_sort_key {", "int rj_debug_sort_key("):
        assert text in h, text
    assert capi.load().rj_abi_version() == 3 and "rj_debug_sort_key" in capi.EXPORTS


def test_plan_shardable_refuses_sorts():
    cols = key_table(rng_for("s"), 50, [I32, I32], null_p=0)
    ok, why = capi.plan_shardable(sort_plan(cols, [(0, 0)]))
    assert not ok and "RJ_NODE_SORT" in why
    q = pl.Plan()  # ... under a join
    a = q.new_scan_node(0, [(0, I32), (1, I32)])
    s = q.new_sort_node(a, [(0, DESC)], [(0, I32)], limit=5)
    b = q.new_scan_node(0, [(0, I32)])
    q.root = q.new_join_node(True, s, b, 0, 0, [(0, I32)])
    q.new_input(pl.make_table(cols))
    ok, why = capi.plan_shardable(q)
    assert not ok and "RJ_NODE_SORT" in why


def test_library_holds_the_sort_kernels():
    import _elfsyms
    fams = {_elfsyms.short_name(n).split("<")[0] for n in _elfsyms.kernel_handles(km.LIB)}
    assert {"k_sort_encode", "k_sort_count", "k_sort_scan", "k_sort_scatter", "k_sort_iota"} <= fams
    hpp = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
    assert "constexpr int SORT_TILE = " in hpp


# ------------------------------------------------------------------ the key encoding on the host
@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_host_key_encoding_orders_every_pair_of_edge_values_as_the_comparator_does(dt, flags):
    """The unsigned order of (null_digit, key) is the comparator's order, ties included, for every
    ordered pair of the edge list (NULL among them)."""
    enc = [capi.sort_key(dt, flags, bits, v is None) for v, bits in EDGES[dt]]
    for (i, (a, _)), (j, (b, _)) in itertools.product(enumerate(EDGES[dt]), repeat=2):
        want = compare_rows((a,), (b,), [(0, flags)], [dt])
        got = (enc[i] > enc[j]) - (enc[i] < enc[j])
        assert got == want, (dt, flags, a, b, enc[i], enc[j])
    if dt == I32:
        assert all(key < 2**32 for _, key in enc)      # a 32-bit key: four passes at most
    assert enc[-1][1] == 0                             # a NULL's value bits are zero: NULLs tie


def test_host_key_encoding_is_the_documented_mapping():
    assert capi.sort_key(I32, 0, 5) == (0, 5 ^ 0x80000000)
    assert capi.sort_key(I32, DESC, 5) == (0, ~(5 ^ 0x80000000) & 0xFFFFFFFF)
    assert capi.sort_key(I64, 0, (-7) & (2**64 - 1)) == (0, ((-7) & (2**64 - 1)) ^ (1 << 63))
    assert capi.sort_key(F64, 0, bits_of(1.0)) == (0, bits_of(1.0) | (1 << 63))
    assert capi.sort_key(F64, 0, bits_of(-1.0)) == (0, ~bits_of(-1.0) & (2**64 - 1))
    assert capi.sort_key(F64, 0, bits_of(-0.0)) == capi.sort_key(F64, 0, bits_of(0.0))
    assert len({capi.sort_key(F64, 0, b) for b in (QNAN, SNAN, NEG_NAN, PAYLOAD_NAN)}) == 1
    assert capi.sort_key(F64, NF, 0, True) == (0, 0) and capi.sort_key(F64, NF, 0) == (1, 1 << 63)
    assert capi.sort_key(I64, DESC, 123, True) == (1, 0)
    for dt, flags in ((VC, 0), (7, 0), (I32, 4), (I32, -1)):
        with pytest.raises(capi.RjError) as e:
            capi.sort_key(dt, flags, 0)
        assert e.value.code == 1
    L = capi.load()
    assert L.rj_debug_sort_key(I32, 0, 0, 0, None, None) == 1


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_numpy_encoding_is_the_librarys(dt, flags):
    cols = key_table(rng_for("enc", dt, flags), 200, [dt])
    nd, key = _sortref.encode(dt, cols[0][1], cols[0][2], flags)
    raw = np.ascontiguousarray(cols[0][1]).view(np.uint32 if dt == I32 else np.uint64)
    for r in range(200):
        assert (int(nd[r]), int(key[r])) == capi.sort_key(dt, flags, int(raw[r]), not cols[0][2][r]), r


# ------------------------------------------------------------------ the reference, pinned
TYPES = [I32, I64, F64, I32, F64]


@pytest.mark.parametrize("block", range(8))
def test_reference_agrees_with_the_row_at_a_time_comparator(block):
    """20 seeded sorts per block (160 in all): one to three keys of all three types, both flags, NULLs,
    heavy ties, limits and offsets — position by position, ties included (both sides are stable)."""
    rng = rng_for("cmp", block)
    n = int(rng.integers(1, 260))
    cols = key_table(rng, n, TYPES)
    rows = python_rows(cols)
    inorder = _sortref.rel_rows(cols)
    for _ in range(20):
        keys = [(int(rng.integers(0, len(TYPES))), int(rng.integers(0, 4))) for _ in range(int(rng.integers(1, 4)))]
        limit = None if rng.random() < 0.3 else int(rng.integers(0, n + 3))
        offset = 0 if rng.random() < 0.3 else int(rng.integers(0, n + 3))
        want = sorted_by_comparator(rows, keys, TYPES, limit, offset)
        assert _sortref.order(cols, keys)[slice(*np.cumsum(_sortref.slice_of(n, limit, offset)))].tolist() == want, (keys, limit, offset)
        cnt, out = _sortref.sort(cols, keys, [(4, F64), (0, I32)], limit, offset)
        assert cnt == len(want) and _sortref.rel_rows(out, cnt) == [(inorder[r][4], inorder[r][0]) for r in want]
        # and the tie-aware checker accepts it, both ways
        got = [inorder[r] for r in want]
        assert _sortref.same_sorted(got, inorder, keys, limit, offset, exact=True) is None
        assert _sortref.same_sorted(got, inorder[::-1], keys, limit, offset, exact=False) is None


def test_reference_rules_by_hand():
    nan = float("nan")
    cols = [(F64, np.array([nan, 1.5, -0.0, math.inf, 0.0, -nan, 2.0]), np.array([1, 1, 1, 1, 1, 1, 0], bool)),
            (I32, np.arange(7, dtype=np.int32), np.ones(7, bool))]
    o = lambda keys, **kw: _sortref.sort(cols, keys, [(1, I32)], **kw)[1][0][1].tolist()
    assert o([(0, 0)]) == [2, 4, 1, 3, 0, 5, 6]            # -0.0 = +0.0 (stable), NaNs above +inf and equal, NULL last
    assert o([(0, DESC)]) == [0, 5, 3, 1, 2, 4, 6]         # DESC flips the values, not the NULLs
    assert o([(0, NF)]) == [6, 2, 4, 1, 3, 0, 5]
    assert o([(0, DESC | NF)]) == [6, 0, 5, 3, 1, 2, 4]
    assert o([(0, 0)], limit=2, offset=1) == [4, 1] and o([(0, 0)], limit=0) == [] and o([(0, 0)], offset=7) == []
    assert o([(0, 0)], limit=2**64 - 2, offset=2**64 - 1) == [] and o([(0, 0)], limit=2**64 - 2, offset=5) == [5, 6]
    assert o([], limit=3, offset=2) == [2, 3, 4]           # no keys: the child's own order
    assert o([(0, 0), (0, DESC)]) == o([(0, 0)])           # the same column again orders nothing


def test_reference_evaluates_nested_plans():
    """top-3 groups of an aggregation over a selection; a sort below a semi join is its slice as a set"""
    rng = rng_for("nest")
    n = 500
    cols = [(I32, rng.integers(0, 30, n).astype(np.int32), np.ones(n, bool)), (I64, rng.integers(0, 100, n), np.ones(n, bool))]
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    w = p.new_select_node(a, [("GEQ", 1, 50)], [(0, I32), (1, I64)])
    g = p.new_agg_node(w, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64)])
    p.root = p.new_sort_node(g, [(1, DESC), (0, 0)], [(0, I32), (1, I64)], limit=3)
    p.new_input(pl.make_table(cols))
    k, v = cols[0][1], cols[1][1]
    counts = sorted(((int(x), int(((k == x) & (v >= 50)).sum())) for x in np.unique(k)), key=lambda t: (-t[1], t[0]))
    assert pl.table_rows(_sortref.execute(p)) == counts[:3]
    q = pl.Plan()
    a = q.new_scan_node(0, [(0, I32), (1, I64)])
    s = q.new_sort_node(a, [(0, 0)], [(0, I32)], limit=int((k <= 4).sum()))   # the boundary is a key boundary
    b = q.new_scan_node(0, [(0, I32), (1, I64)])
    q.root = q.new_semi_join_node(True, s, b, 0, 0, [(1, I32), (2, I64)])   # the sort is the filter side
    q.new_input(pl.make_table(cols))
    assert pl.sorted_rows(_sortref.execute(q)) == sorted((int(x), int(y)) for x, y in zip(k, v) if x <= 4)


# ------------------------------------------------------------------ the tie-aware checker rejects what it must
def _tie_case():
    # key, payload: three tie groups, the slice [1, 6) cuts the first and holds the second whole
    child = [(1, 10), (1, 11), (2, 20), (2, 21), (2, 22), (3, 30), (3, 31)]
    keys, limit, offset = [(0, 0)], 5, 1
    return child, keys, limit, offset


def test_checker_accepts_any_member_of_a_cut_tie_group_and_any_order_inside_a_group():
    child, keys, limit, offset = _tie_case()
    for first in ((1, 10), (1, 11)):
        for mid in itertools.permutations([(2, 20), (2, 21), (2, 22)]):
            for last in ((3, 30), (3, 31)):
                assert _sortref.same_sorted([first, *mid, last], child, keys, limit, offset, exact=False) is None
    assert _sortref.same_sorted([(1, 11), (2, 20), (2, 21), (2, 22), (3, 30)], child, keys, limit, offset, exact=True) is None
    assert _sortref.same_sorted([(1, 10), (2, 20), (2, 21), (2, 22), (3, 30)], child, keys, limit, offset, exact=True)


@pytest.mark.parametrize("exact", [False, True])
def test_checker_rejects(exact):
    child, keys, limit, offset = _tie_case()
    good = [(1, 11), (2, 20), (2, 21), (2, 22), (3, 30)]
    bad = lambda got: _sortref.same_sorted(got, child, keys, limit, offset, exact=exact)
    assert bad(good) is None
    assert bad([good[1], good[0]] + good[2:])                                   # a swapped pair (keys out of order)
    assert bad([(1, 12)] + good[1:])                                            # a row from outside the child
    assert bad(good[:3] + [(2, 21)] + good[4:])                                 # a duplicated row: a wrong member of a COMPLETE group
    assert bad([(1, 11), (2, 20), (2, 21), (2, 23), (3, 30)])                   # ... and one the group never held
    assert bad([(1, 11), (2, 20), (2, 21), (2, 22), (3, 30), (3, 31)])          # a row too many
    assert bad(good[:-1])                                                       # a row too few
    assert bad([(1, 11), (2, 20), (2, 21), (2, 22), (3, 30)][::-1])             # the reverse order
    # NULLs and doubles: NaN payloads and the sign of zero are part of a row, not of its key
    f = lambda x: ("f64", bits_of(x))
    child2 = [(f(-0.0), 1), (f(0.0), 2), (("f64", SNAN), 3), (("f64", NEG_NAN), 4), (None, 5)]
    ok = [(f(0.0), 2), (f(-0.0), 1), (("f64", NEG_NAN), 4), (("f64", SNAN), 3), (None, 5)]
    assert _sortref.same_sorted(ok, child2, [(0, 0)], None, 0, exact=False) is None
    assert _sortref.same_sorted(ok, child2, [(0, 0)], None, 0, exact=True)      # exact wants the child's order inside ties
    assert _sortref.same_sorted([(f(0.0), 1)] + ok[1:], child2, [(0, 0)], None, 0, exact=False)   # the sign bit moved to another row
    assert "not among the outputs" in _sortref.same_sorted([(1,)], [(1, 2)], [(1, 0)], None, 0, exact=False, outs=[0])
