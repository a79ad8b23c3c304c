"""Grouping nodes (RJ_NODE_GROUP) without a GPU: marshalling, the header, the sharding refusal, the
host side of the key decoding (rj_debug_sort_key_value), and the numpy reference tests/_groupref.py
pinned against a row-at-a-time second reference: a dictionary of groups filled row by row, written
from the prose of include/rj.h ("Grouping equality", "Values", "Rows", "Order"), not from the encoding."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import _aggref
import _groupref
import test_gpu_kernel_matrix as km
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
DESC, NF = pl.SORT_DESC, pl.SORT_NULLS_FIRST
KEY, STAR, COUNT, SUM, MIN, MAX = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX
rng_for, ALL_FLAGS, EDGES, bits_of, f64_of = sp.rng_for, sp.ALL_FLAGS, sp.EDGES, sp.bits_of, sp.f64_of
CANON_NAN = 0x7FF8000000000000


def group_plan(cols, keys, outputs):
    """Scan(cols) -> GROUP BY keys; outputs = [(func, column, result type)]"""
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    p.root = p.new_group_node(sc, keys, outputs)
    p.new_input(pl.make_table(cols))
    return p


def all_outputs(types, keys, rng=None):
    """every key once, COUNT(*), and every legal function of every column"""
    outs = [(KEY, c, types[c]) for c in dict.fromkeys(c for c, _ in keys)] + [(STAR, 0, I64)]
    for c, dt in enumerate(types):
        outs += [(COUNT, c, I64), (MIN, c, dt), (MAX, c, dt)] + ([(SUM, c, I64)] if dt != F64 else [])
    if rng is not None:
        outs = [outs[i] for i in rng.permutation(len(outs))[: int(rng.integers(0, len(outs) + 1))]]
    return outs


# ------------------------------------------------------------------ the second reference, from the prose
def canon_value(v, dt):
    """a group's canonical value: +0.0 for a zero, one NaN for every NaN, the value itself otherwise"""
    if dt == F64:
        if math.isnan(v):
            return f64_of(CANON_NAN)
        if v == 0:
            return 0.0
    return v


def group_by_dictionary(rows, types, keys, outputs):
    """rows: Python values (None = NULL) -> result rows IN ORDER, doubles as ("f64", bits)."""
    def group_of(row):   # NULL equals NULL per column, -0.0 equals +0.0, NaN equals NaN
        g = []
        for c, _ in keys:
            v = row[c]
            g.append(None if v is None else ("nan" if types[c] == F64 and math.isnan(v) else canon_value(v, types[c])))
        return tuple(g)

    def value_order(a, b, dt):   # the order MIN / MAX use: by value; a NaN is above +inf
        return sp.compare_values(a, b, dt)

    groups = {}
    if not keys:
        groups[()] = []          # the scalar aggregate: one group, also of no rows
    for row in rows:
        groups.setdefault(group_of(row), []).append(row)
    # the order of the groups: lexicographic over the keys under their flags
    member = {g: (members[0] if members else None) for g, members in groups.items()}
    ordered = sorted(groups, key=functools.cmp_to_key(lambda a, b: sp.compare_rows(member[a], member[b], keys, types) if keys else 0))
    out = []
    for g in ordered:
        members, res = groups[g], []
        for func, c, rt in outputs:
            if func == STAR:
                res.append(len(members))
                continue
            dt = types[c]
            if func == KEY:
                v = members[0][c]
                v = None if v is None else canon_value(v, dt)
            else:
                vals = [m[c] for m in members if m[c] is not None]
                if func == COUNT:
                    v = len(vals)
                elif not vals:
                    v = None
                elif func == SUM:
                    v = (sum(vals) + 2**63) % 2**64 - 2**63
                else:
                    best = vals[0]
                    for x in vals[1:]:
                        r = value_order(x, best, dt)
                        if (r < 0 and func == MIN) or (r > 0 and func == MAX):
                            best = x
                    v = canon_value(best, dt)
            res.append(("f64", bits_of(v) - (2**64 if bits_of(v) >> 63 else 0)) if isinstance(v, float) else v)
        out.append(tuple(res))
    return out


TYPES = [I32, I64, F64, I32, F64]


@pytest.mark.parametrize("block", range(8))
def test_reference_agrees_with_the_row_at_a_time_dictionary(block):
    """15 seeded groupings per block: zero to three keys of all three types, all flags, NULLs, heavy
    ties, the edge values of every type — position by position, doubles by their bits."""
    rng = rng_for("dict", block)
    n = int(rng.integers(0, 260)) if block else 0
    cols = sp.key_table(rng, n, TYPES, domain=int(rng.integers(1, 5))) if n else [(dt, np.zeros(0, km.NP_OF[dt]), np.zeros(0, bool)) for dt in TYPES]
    rows = sp.python_rows(cols) if n else []
    for _ in range(15):
        keys = [(int(rng.integers(0, len(TYPES))), int(rng.integers(0, 4))) for _ in range(int(rng.integers(0, 4)))]
        outputs = all_outputs(TYPES, keys, rng)
        ng, out = _groupref.group(cols, keys, outputs, n)
        want = group_by_dictionary(rows, TYPES, keys, outputs)
        assert ng == len(want), (keys, ng, len(want))
        assert _groupref.rel_rows(out, ng) == want, (keys, outputs)


def test_reference_rules_by_hand():
    nan = float("nan")
    cols = [(F64, np.array([nan, 1.5, -0.0, math.inf, 0.0, -nan, 2.0, 1.5]), np.array([1, 1, 1, 1, 1, 1, 0, 1], bool)),
            (I32, np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.int32), np.array([1, 1, 1, 1, 0, 1, 1, 0], bool)),
            (I64, np.array([2**62, 2**62, 2**62, 2**62, -1, 5, 2**62, 2**62]), np.ones(8, bool))]
    f = lambda x: ("f64", bits_of(x))
    ng, out = _groupref.group(cols, [(0, 0)], [(KEY, 0, F64), (STAR, 0, I64), (COUNT, 1, I64), (SUM, 1, I64), (MIN, 1, I32)])
    # zeros (-0.0 = +0.0, comes out +0.0), 1.5 twice, +inf, the NaNs (one value, the canonical one), NULL last
    assert _groupref.rel_rows(out, ng) == [(f(0.0), 2, 1, 3, 3), (f(1.5), 2, 1, 2, 2), (f(math.inf), 1, 1, 4, 4),
                                           (("f64", CANON_NAN), 2, 2, 7, 1), (None, 1, 1, 7, 7)]
    ng, out = _groupref.group(cols, [(0, DESC | NF)], [(KEY, 0, F64)])
    assert _groupref.rel_rows(out, ng) == [(None,), (("f64", CANON_NAN),), (f(math.inf),), (f(1.5),), (f(0.0),)]
    # the scalar aggregate; SUM wraps; FP64 MIN / MAX: a NaN above +inf, canonical values
    ng, out = _groupref.group(cols, [], [(STAR, 0, I64), (SUM, 2, I64), (MIN, 0, F64), (MAX, 0, F64), (MAX, 1, I32)])
    assert _groupref.rel_rows(out, ng) == [(8, (6 * 2**62 + 4 + 2**63) % 2**64 - 2**63, f(0.0), ("f64", CANON_NAN), 7)]
    none = [(dt, v[:0], m[:0]) for dt, v, m in cols]
    ng, out = _groupref.group(none, [], [(STAR, 0, I64), (COUNT, 1, I64), (SUM, 2, I64), (MIN, 0, F64)], 0)
    assert _groupref.rel_rows(out, ng) == [(0, 0, None, None)]              # ONE row over no rows
    assert _groupref.group(none, [(1, 0)], [(KEY, 1, I32), (STAR, 0, I64)], 0)[0] == 0
    # (NULL, 1), (1, NULL), (NULL, NULL): three groups; DISTINCT = no aggregate
    two = [(I32, np.array([0, 1, 0, 0, 1], dtype=np.int32), np.array([0, 1, 0, 0, 1], bool)),
           (I32, np.array([1, 0, 0, 1, 0], dtype=np.int32), np.array([1, 0, 0, 1, 0], bool))]
    ng, out = _groupref.group(two, [(0, 0), (1, 0)], [(KEY, 0, I32), (KEY, 1, I32)])
    assert _groupref.rel_rows(out, ng) == [(1, None), (None, 1), (None, None)]
    # the same column again groups nothing and orders nothing
    a = _groupref.group(cols, [(1, 0), (1, DESC)], [(KEY, 1, I32), (STAR, 0, I64)])
    b = _groupref.group(cols, [(1, 0)], [(KEY, 1, I32), (STAR, 0, I64)])
    assert _groupref.rel_rows(a[1], a[0]) == _groupref.rel_rows(b[1], b[0])


@pytest.mark.parametrize("seed", range(12))
def test_reference_agrees_with_the_aggregation_reference_on_one_integer_key(seed):
    rng = rng_for("agg", seed)
    n = int(rng.integers(1, 400))
    kt, vt = [I32, I64][seed % 2], [I32, I64][(seed // 2) % 2]
    cols = [(kt, rng.integers(-4, 4, n).astype(km.NP_OF[kt]), rng.random(n) >= 0.2),
            (vt, rng.integers(-2**31, 2**31, n).astype(km.NP_OF[vt]), rng.random(n) >= 0.3)]
    outputs = [(KEY, 0, kt), (STAR, 0, I64), (COUNT, 1, I64), (SUM, 1, I64), (MIN, 1, vt), (MAX, 1, vt), (KEY, 0, kt)]
    a = _groupref.to_table(*_groupref.group(cols, [(0, int(rng.integers(0, 4)))], outputs))
    b = _aggref.to_table(*_aggref.aggregate(cols, 0, outputs))
    assert pl.canonical_rows(a) == pl.canonical_rows(b)


def test_reference_evaluates_nested_plans():
    """a grouping over a selection under a sort under another grouping; a join on a key it produced"""
    rng = rng_for("nest")
    n = 600
    cols = [(I32, rng.integers(0, 30, n).astype(np.int32), np.ones(n, bool)), (I64, rng.integers(0, 100, n), np.ones(n, bool))]
    k, v = cols[0][1], cols[1][1]
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    w = p.new_select_node(a, [("GEQ", 1, 50)], [(0, I32), (1, I64)])
    g = p.new_group_node(w, [(0, 0)], [(KEY, 0, I32), (STAR, 0, I64)])
    s = p.new_sort_node(g, [(1, DESC), (0, 0)], [(0, I32), (1, I64)])
    p.root = p.new_group_node(s, [(1, DESC)], [(KEY, 1, I64), (STAR, 0, I64), (MIN, 0, I32)])
    p.new_input(pl.make_table(cols))
    counts = {int(x): int(((k == x) & (v >= 50)).sum()) for x in np.unique(k[v >= 50])}
    want = [(c, sum(1 for y in counts.values() if y == c), min(x for x, y in counts.items() if y == c))
            for c in sorted(set(counts.values()), reverse=True)]
    assert pl.table_rows(_groupref.execute(p)) == want
    q = pl.Plan()
    a = q.new_scan_node(0, [(0, I32), (1, I64)])
    g = q.new_group_node(a, [(0, 0)], [(KEY, 0, I32), (MAX, 1, I64)])
    b = q.new_scan_node(0, [(0, I32)])
    q.root = q.new_join_node(True, g, b, 0, 0, [(0, I32), (1, I64)])
    q.new_input(pl.make_table(cols))
    assert pl.sorted_rows(_groupref.execute(q)) == sorted((int(x), int(v[k == x].max())) for x in k)


# ------------------------------------------------------------------ interface
def test_marshalling_round_trips_keys_and_outputs():
    cols = sp.key_table(rng_for("m"), 20, [I32, I64, F64])
    p = group_plan(cols, [(2, DESC), (0, NF), (2, 0)], [(KEY, 2, F64), (STAR, 0, I64), (MAX, 1, I64)])
    cp, keep = pl.plan_to_c(p)
    nd = cp.nodes[p.root]
    assert nd.kind == pl.NODE_GROUP == 9 and nd.left == 0 and nd.n_out == 3
    assert nd.right == 3 and nd.right_attr != 0
    ks = C.cast(C.c_void_p(nd.right_attr), C.POINTER(pl.rj_sort_key))
    assert [(ks[k].column, ks[k].flags) for k in range(3)] == [(2, 1), (0, 2), (2, 0)]
    assert [nd.out_idx[k] for k in range(3)] == [pl.agg_out(KEY, 2), pl.agg_out(STAR, 0), pl.agg_out(MAX, 1)]
    assert [nd.out_idx[k] for k in range(3)] == [2, 1 << 56, (5 << 56) | 1]
    assert [nd.out_type[k] for k in range(3)] == [F64, I64, I64]
    # no keys: a NULL pointer
    cp2, keep2 = pl.plan_to_c(group_plan(cols, [], [(STAR, 0, I64)]))
    nd = cp2.nodes[1]
    assert nd.kind == 9 and nd.right == 0 and nd.right_attr == 0 and nd.n_out == 1
    assert isinstance(p.nodes[p.root].data, pl.GroupNode) and p.nodes[p.root].data.keys == [(2, 1), (0, 2), (2, 0)]
    del keep, keep2


def test_header_declares_the_kind_the_accessors_and_the_decoder():
    h = open(os.path.join(os.path.dirname(km.LIB), "..", "include", "rj.h")).read()
    for text in ("RJ_NODE_GROUP = 9", "#define RJ_GROUP_N_KEYS(node) ((node)->right)",
                 "#define RJ_GROUP_KEYS(node) ((const rj_sort_key*)(uintptr_t)(node)->right_attr)",
                 "int rj_debug_sort_key_value(int32_t type, int32_t flags, uint64_t key, uint64_t* bits);", "MIN(title)"):
        assert text in h, text
    assert capi.load().rj_abi_version() == 3 and "rj_debug_sort_key_value" in capi.EXPORTS


def test_plan_shardable_refuses_groupings():
    cols = sp.key_table(rng_for("s"), 50, [I32, I32], null_p=0)
    ok, why = capi.plan_shardable(group_plan(cols, [(0, 0)], [(KEY, 0, I32)]))
    assert not ok and "RJ_NODE_GROUP" in why
    q = pl.Plan()  # ... under a join
    a = q.new_scan_node(0, [(0, I32), (1, I32)])
    g = q.new_group_node(a, [(0, DESC)], [(KEY, 0, I32)])
    b = q.new_scan_node(0, [(0, I32)])
    q.root = q.new_join_node(True, g, b, 0, 0, [(0, I32)])
    q.new_input(pl.make_table(cols))
    ok, why = capi.plan_shardable(q)
    assert not ok and "RJ_NODE_GROUP" in why


def test_library_holds_the_group_kernels_and_documents_its_switch():
    import _elfsyms
    names = {_elfsyms.short_name(n) for n in _elfsyms.kernel_handles(km.LIB)}
    assert {"k_group_heads<4>", "k_group_heads<8>", "k_group_scan", "k_group_keys<4>", "k_group_keys<8>", "k_group_init",
            "k_group_reduce<0,true>", "k_group_reduce<4,true>", "k_group_reduce<8,true>", "k_group_reduce<0,false>", "k_group_reduce<4,false>",
            "k_group_reduce<8,false>", "k_group_column"} == {n for n in names if n.startswith("k_group_")}
    hpp = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
    assert "constexpr int GROUP_TILE = " in hpp
    doc = open(os.path.join(os.path.dirname(km.LIB), "..", "INTEGRATION.md")).read()
    assert "RJ_TUNE_GROUP_GRID" in doc


# ------------------------------------------------------------------ the key decoding on the host
@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_host_key_decoding_round_trips_the_edge_values(dt, flags):
    for v, bits in EDGES[dt]:
        if v is None:
            continue
        _, key = capi.sort_key(dt, flags, bits)
        back = capi.sort_key_value(dt, flags, key)
        if dt == F64 and math.isnan(v):
            assert back == CANON_NAN, (hex(bits), hex(back))
        elif dt == F64 and v == 0:
            assert back == 0, (hex(bits), hex(back))          # -0.0 decodes to +0.0
        else:
            assert back == bits, (dt, flags, hex(bits), hex(back))
        assert capi.sort_key(dt, flags, back)[1] == key        # the canonical value has the same key


def test_host_key_decoding_is_the_documented_mapping_and_its_error_contract():
    assert capi.sort_key_value(I32, 0, 5 ^ 0x80000000) == 5
    assert capi.sort_key_value(I32, DESC, ~(5 ^ 0x80000000) & 0xFFFFFFFF) == 5
    assert capi.sort_key_value(I32, 0, 0) == 0x80000000                       # INT32_MIN, in the low word
    assert capi.sort_key_value(I64, NF, ((-7) & (2**64 - 1)) ^ (1 << 63)) == (-7) & (2**64 - 1)
    assert capi.sort_key_value(F64, 0, bits_of(1.0) | (1 << 63)) == bits_of(1.0)
    assert capi.sort_key_value(F64, 0, ~bits_of(-1.0) & (2**64 - 1)) == bits_of(-1.0)
    assert capi.sort_key_value(F64, DESC | NF, ~(bits_of(2.5) | (1 << 63)) & (2**64 - 1)) == bits_of(2.5)
    for b in (sp.QNAN, sp.SNAN, sp.NEG_NAN, sp.PAYLOAD_NAN):
        assert capi.sort_key_value(F64, 0, capi.sort_key(F64, 0, b)[1]) == CANON_NAN
    assert capi.sort_key_value(F64, 0, capi.sort_key(F64, 0, bits_of(-0.0))[1]) == 0
    for dt, flags in ((VC, 0), (7, 0), (I32, 4), (I32, -1)):
        with pytest.raises(capi.RjError) as e:
            capi.sort_key_value(dt, flags, 0)
        assert e.value.code == 1
    assert capi.load().rj_debug_sort_key_value(I32, 0, 0, None) == 1


@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_numpy_decoding_is_the_librarys(dt):
    cols = sp.key_table(rng_for("dec", dt), 200, [dt], null_p=0)
    _, key = _groupref._sortref.encode(dt, cols[0][1], cols[0][2], 0)
    back = np.ascontiguousarray(_groupref.decode(dt, key)).view(np.uint32 if dt == I32 else np.uint64)
    for r in range(200):
        assert int(back[r]) == capi.sort_key_value(dt, 0, int(key[r])), r
