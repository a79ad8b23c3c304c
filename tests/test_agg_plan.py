"""Aggregation nodes (RJ_NODE_AGG) without a GPU: marshalling, the sharding refusal, the compiled
kernel families, and the numpy reference tests/_aggref.py against a brute-force Python dict and
against the pinned C oracle (its inner join distinct_keys(T) x T, grouped in Python)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import _aggref
import _elfsyms
import _oracle
from pyrj import capi
from pyrj import plan as pl
from test_gpu_kernel_matrix import LIB

I32, I64 = pl.INT32, pl.INT64
ALL = [(pl.AGG_KEY, 0, None), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_COUNT, 1, I64), (pl.AGG_SUM, 1, I64),
       (pl.AGG_MIN, 1, None), (pl.AGG_MAX, 1, None)]


def rng_for(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def agg_plan(cols, outputs, key_attr=0):
    """Scan(cols) -> GROUP BY key_attr; a result type of None is filled in from the column."""
    p = pl.Plan()
    sc = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(cols)])
    outs = [(f, c, t if t is not None else _aggref.result_type(f, cols[c][0], cols[key_attr][0])) for f, c, t in outputs]
    p.root = p.new_agg_node(sc, key_attr, outs)
    p.new_input(pl.make_table(cols))
    return p


def small_table(rng, n, kt=I32, vt=I64, groups=7, key_nulls=True, val_nulls=True):
    k = rng.integers(-3, groups - 3, n).astype(_aggref.NP_OF[kt])
    lim = 2**62 if vt == I64 else 2**31 - 1
    v = rng.integers(-lim, lim, n, dtype=np.int64).astype(_aggref.NP_OF[vt])
    kv = rng.random(n) >= (0.15 if key_nulls else 0.0)
    vv = rng.random(n) >= (0.3 if val_nulls else 0.0)
    return [(kt, k, kv), (vt, v, vv)]


def test_marshalling_round_trips_kind_outputs_and_types():
    p = agg_plan(small_table(rng_for("m"), 10), ALL)
    cp, keep = pl.plan_to_c(p)
    nd = cp.nodes[p.root]
    assert nd.kind == pl.NODE_AGG == 6 and nd.left == 0 and nd.left_attr == 0 and nd.n_out == len(ALL)
    want_t = [I32, I64, I64, I64, I64, I64]
    for k, (f, c, _) in enumerate(ALL):
        assert nd.out_idx[k] == (f << 56) | c
        assert (pl.agg_func(nd.out_idx[k]), pl.agg_col(nd.out_idx[k])) == (f, c)
        assert nd.out_type[k] == want_t[k]
    assert (pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX) == (0, 1, 2, 3, 4, 5)
    del keep


def test_header_declares_the_kind_and_the_encoding():
    import os
    h = open(os.path.join(os.path.dirname(LIB), "..", "include", "rj.h")).read()
    for text in ("RJ_NODE_AGG = 6", "RJ_AGG_KEY        = 0", "RJ_AGG_MAX        = 5", "#define RJ_AGG_OUT(func, col)",
                 "#define RJ_AGG_FUNC(x)", "#define RJ_AGG_COL(x)"):
        assert text in h, text


def test_plan_shardable_refuses_aggregations():
    cols = small_table(rng_for("s"), 50, val_nulls=False, key_nulls=False)
    p = agg_plan(cols, ALL)
    ok, why = capi.plan_shardable(p)
    assert not ok and "RJ_NODE_AGG" in why
    # ... under a join
    q = pl.Plan()
    a = q.new_scan_node(0, [(0, I32), (1, I64)])
    g = q.new_agg_node(a, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64)])
    b = q.new_scan_node(0, [(0, I32)])
    q.root = q.new_join_node(True, g, b, 0, 0, [(0, I32), (1, I64)])
    q.new_input(pl.make_table(cols))
    ok, why = capi.plan_shardable(q)
    assert not ok and "RJ_NODE_AGG" in why
    # a plain join plan stays shardable
    j = pl.Plan()
    a = j.new_scan_node(0, [(0, I32)])
    b = j.new_scan_node(0, [(0, I32)])
    j.root = j.new_join_node(True, a, b, 0, 0, [(0, I32)])
    j.new_input(pl.make_table(cols))
    assert capi.plan_shardable(j)[0]


def test_library_holds_the_aggregation_kernels():
    names = {_elfsyms.short_name(n) for n in _elfsyms.kernel_handles(LIB)}
    fams = {n.split("<")[0] for n in names}
    assert {"k_agg_parts", "k_agg_nullkey", "k_agg_emit", "k_agg_merge_init", "k_agg_column"} <= fams
    assert {f"k_agg_parts<{kw},{cw}>" for kw, cws in ((1, range(4)), (2, range(3))) for cw in cws} <= names
    assert {f"k_agg_nullkey<{cw}>" for cw in range(4)} <= names


def brute(cols, outputs, key_attr=0):
    groups = {}
    n = cols[0][1].shape[0]
    for r in range(n):
        k = cols[key_attr][1][r].item() if cols[key_attr][2][r] else None
        groups.setdefault(k, []).append(r)
    rows = []
    for k, rs in groups.items():
        row = []
        for f, c, _ in outputs:
            vals = [cols[c][1][r].item() for r in rs if cols[c][2][r]] if f >= pl.AGG_COUNT else []
            if f == pl.AGG_KEY:
                row.append(k)
            elif f == pl.AGG_COUNT_STAR:
                row.append(len(rs))
            elif f == pl.AGG_COUNT:
                row.append(len(vals))
            elif not vals:
                row.append(None)
            elif f == pl.AGG_SUM:
                row.append((sum(vals) + 2**63) % 2**64 - 2**63)
            else:
                row.append(min(vals) if f == pl.AGG_MIN else max(vals))
        rows.append(tuple(row))
    return sorted(rows, key=pl._sort_key)


@pytest.mark.parametrize("kt,vt", [(I32, I64), (I64, I32), (I32, I32), (I64, I64)])
@pytest.mark.parametrize("seed", range(4))
def test_reference_agrees_with_a_python_dict(kt, vt, seed):
    rng = rng_for("dict", kt, vt, seed)
    cols = small_table(rng, int(rng.integers(1, 400)), kt, vt, groups=int(rng.integers(1, 40)), key_nulls=seed % 2 == 0)
    if seed == 3:  # a group whose values are all NULL
        cols[1] = (vt, cols[1][1], cols[1][2] & (cols[0][1] != 0))
    p = agg_plan(cols, ALL)
    assert pl.sorted_rows(_aggref.execute(p)) == brute(cols, ALL)


def test_reference_sum_wraps_and_empty_child():
    cols = [(I32, np.zeros(3, np.int32)), (I64, np.full(3, 2**62, np.int64))]
    t = _aggref.execute(agg_plan(cols, [(pl.AGG_SUM, 1, I64)]))
    assert pl.table_rows(t) == [((3 * 2**62 + 2**63) % 2**64 - 2**63,)]
    t = _aggref.execute(agg_plan([(I32, np.zeros(0, np.int32)), (I64, np.zeros(0, np.int64))], ALL))
    assert t.num_rows == 0 and [c.type for c in t.columns] == [I32, I64, I64, I64, I64, I64]


@pytest.mark.parametrize("kt", [I32, I64])
@pytest.mark.parametrize("seed", range(3))
def test_reference_is_tied_to_the_oracles_inner_join(kt, seed):
    """distinct_keys(T) JOIN T through the pinned C oracle, grouped in Python, gives the same COUNT /
    SUM / MIN / MAX per key as _aggref (NULL keys drop out of a join: the NULL group is left out)."""
    rng = rng_for("oracle", kt, seed)
    cols = small_table(rng, 500, kt, I64, groups=60, key_nulls=True, val_nulls=False)
    keys = np.unique(cols[0][1][cols[0][2]])
    p = pl.Plan()
    d = p.new_scan_node(0, [(0, kt)])
    t = p.new_scan_node(1, [(0, kt), (1, I64)])
    p.root = p.new_join_node(True, d, t, 0, 0, [(0, kt), (2, I64)])
    p.new_input(pl.make_table([(kt, keys)]))
    p.new_input(pl.make_table(cols))
    by_key = {}
    for k, v in pl.table_rows(_oracle.execute(p)):
        by_key.setdefault(k, []).append(v)
    want = sorted((k, len(v), len(v), (sum(v) + 2**63) % 2**64 - 2**63, min(v), max(v)) for k, v in by_key.items())
    got = [r for r in pl.sorted_rows(_aggref.execute(agg_plan(cols, ALL))) if r[0] is not None]
    assert got == want and len(want) == keys.shape[0]


def test_reference_evaluates_nested_plans():
    """AGG over a join and a join over an AGG go through evaluate()."""
    rng = rng_for("nest")
    cols = small_table(rng, 300, key_nulls=True, val_nulls=True)
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    g = p.new_agg_node(a, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64)])
    b = p.new_scan_node(0, [(0, I32)])
    j = p.new_join_node(True, g, b, 0, 0, [(0, I32), (1, I64)])
    p.root = p.new_agg_node(j, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_SUM, 1, I64)])
    p.new_input(pl.make_table(cols))
    k, kv = cols[0][1], cols[0][2]
    want = sorted((int(x), int((k[kv] == x).sum()) ** 2) for x in np.unique(k[kv]))
    assert pl.sorted_rows(_aggref.execute(p)) == want
