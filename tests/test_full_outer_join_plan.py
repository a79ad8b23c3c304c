"""Full outer join nodes (RJ_NODE_FULL) without a GPU: plan marshalling, rj_plan_shardable, the
kernel handles librj.so compiles for them (tests/_elfsyms.py), and the numpy reference the GPU tests
compare against (tests/_fullref.py) tied to the pinned references:
  rows valid on both sides              ==  the C oracle's inner join of the plan,
  pairs + rows NULL on the built side   ==  _outerref.execute of the plan as an outer join,
  rows NULL on the built side           ==  _filterref's ANTI (probed side preserved),
  rows NULL on the probed side          ==  _filterref's ANTI the other way,
  the row count is the sum of the three, and swapping build_left changes nothing."""
import os
from collections import Counter

import numpy as np
import pytest

import _elfsyms
import _filterref
import _fullref
import _oracle
import _outerref
from pyrj import capi
from pyrj import hashing as hs
from pyrj import plan as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "radix-join_amd", "librj.so")
I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
NP_OF = {I32: np.int32, I64: np.int64, F64: np.float64}

# (KW, CWB, CWP) of k_full_bcast / k_full_join: KW = key words (1: INT32, 2: INT64 / FP64); CWB /
# CWP = carry words of the built / probed side, both under the optional rules: 0 nothing, 1 a row
# index, 2 / 3 a wide carry that ends with a validity word.  Each is bounded by 4 - KW.
FULL_SHAPES = [(kw, b, p) for kw in (1, 2) for b in range(5 - kw) for p in range(5 - kw)]
BUILD_SHAPES = [(kw, b) for kw in (1, 2) for b in range(5 - kw)]


@pytest.fixture(scope="module")
def handles():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    return _elfsyms.kernel_handles(LIB)


def _plan(build_left=True, under_join=False):
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I32)])
    b = p.new_scan_node(1, [(0, I32), (1, I64)])
    outs = [(2, I32), (3, I64), (1, I32)]
    f = p.new_full_outer_join_node(build_left, a, b, 0, 1 if build_left else 0, outs)
    p.root = f
    if under_join:
        c = p.new_scan_node(2, [(0, I32)])
        p.root = p.new_join_node(True, c, f, 0, 0, [(0, I32), (2, I64)])
    for _ in range(3):
        p.new_input(pl.make_table([(I32, [1, 2, 3]), (I32, [4, 5, 6])]))
    return p


@pytest.mark.parametrize("build_left", [True, False])
@pytest.mark.parametrize("under_join", [False, True])
def test_marshalling_round_trips_kind(build_left, under_join):
    assert pl.NODE_FULL == 5
    p = _plan(build_left, under_join)
    cp, keep = pl.plan_to_c(p, with_inputs=False)
    nodes = [cp.nodes[i] for i in range(cp.n_nodes)]
    assert [n.kind for n in nodes] == ([0, 0, 5, 0, 1] if under_join else [0, 0, 5])
    f = nodes[2]
    assert (f.build_left, f.left, f.right, f.left_attr, f.right_attr) == (int(build_left), 0, 1, 0, 1 if build_left else 0)
    assert [f.out_idx[i] for i in range(f.n_out)] == [2, 3, 1]
    assert [f.out_type[i] for i in range(f.n_out)] == [I32, I64, I32]
    assert p.nodes[2].data == pl.FullOuterJoinNode(build_left, 0, 1, 0, 1 if build_left else 0)
    del keep


def test_older_constructors_keep_their_kinds():
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32)])
    b = p.new_scan_node(1, [(0, I32)])
    j = p.new_join_node(True, a, b, 0, 0, [(0, I32)])
    s = p.new_semi_join_node(True, a, b, 0, 0, [(1, I32)])
    t = p.new_anti_join_node(True, a, b, 0, 0, [(1, I32)])
    o = p.new_outer_join_node(True, a, b, 0, 0, [(1, I32)])
    p.root = j
    cp, keep = pl.plan_to_c(p, with_inputs=False)
    assert [cp.nodes[i].kind for i in (j, s, t, o)] == [1, 2, 3, 4]
    assert isinstance(p.nodes[o].data, pl.OuterJoinNode) and isinstance(p.nodes[j].data, pl.JoinNode)
    del keep


@pytest.mark.parametrize("under_join", [False, True])
def test_plans_with_full_nodes_are_not_shardable(under_join):
    ok, why = capi.plan_shardable(_plan(under_join=under_join))
    assert not ok
    assert "RJ_NODE_FULL" in why


def test_plain_join_plan_stays_shardable():
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I32)])
    b = p.new_scan_node(1, [(0, I32), (1, I32)])
    p.root = p.new_join_node(True, a, b, 0, 0, [(0, I32), (1, I32), (3, I32)])
    assert capi.plan_shardable(p) == (True, "")


def test_abi_version_is_unchanged():
    assert capi.load().rj_abi_version() == 3


def test_library_holds_the_full_kernel_families(handles):
    names = {_elfsyms.short_name(h) for h in handles}
    want = {f"{fam}<{kw},{b},{p}>" for fam in ("k_full_bcast", "k_full_join") for kw, b, p in FULL_SHAPES}
    want |= {f"{fam}<{kw},{b}>" for fam in ("k_full_unmatched", "k_full_buildrows") for kw, b in BUILD_SHAPES}
    assert {n for n in names if n.startswith("k_full_")} == want
    by = Counter(_elfsyms.family(h) for h in handles)
    assert (by["k_full_bcast"], by["k_full_join"], by["k_full_unmatched"], by["k_full_buildrows"]) == (25, 25, 7, 7)


def test_pinned_families_are_unchanged(handles):
    """The full outer join partitions with the inner join's shapes only, reuses k_outer_nullkeys and
    k_outer_gather as they are, and brings its own kernels under its own names."""
    by = Counter(_elfsyms.family(h) for h in handles)
    pinned = {"k_join": 83, "k_join_bcast": 25, "k_pass_hist": 7, "k_fine_hist": 4, "k_pass_scatter": 19,
              "k_pass_scatter_packed": 5, "k_filter_bcast": 7, "k_filter_join": 7, "k_filter_nullkeys": 7,
              "k_outer_bcast": 25, "k_outer_join": 25, "k_outer_nullkeys": 7, "k_outer_gather": 2}
    assert {f: by[f] for f in pinned} == pinned


# ------------------------------------------------------------ _fullref against the pinned references
def _fp64_specials():
    bits = [0x7FF0000000000001, 0x7FF8000000000000, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF,  # NaNs
            0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x800000000000000F,  # +-inf, subnormals
            0x8000000000000000]                                                              # -0.0 only
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _plans(bcols, pcols, build_left, outs):
    """The same inputs and output list under a full outer, an outer and an inner join, and (one
    side's columns only) the two anti joins.  bcols / pcols: built / probed columns, the key first."""
    lcols, rcols = (bcols, pcols) if build_left else (pcols, bcols)
    both = [c[0] for c in lcols] + [c[0] for c in rcols]
    lw = len(lcols)
    plans = {}
    for kind in ("full", "outer", "inner", "anti_p", "anti_b"):
        p = pl.Plan()
        p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
        p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])
        o = [(i, both[i]) for i in outs]
        bl = build_left
        if kind == "anti_p":  # the probed rows without a partner: the built side filters
            o = [(i, t) for i, t in o if (i >= lw) == build_left]
        if kind == "anti_b":  # the built rows without a partner: the probed side filters
            o = [(i, t) for i, t in o if (i < lw) == build_left]
            bl = not build_left
        mk = {"full": p.new_full_outer_join_node, "outer": p.new_outer_join_node, "inner": p.new_join_node,
              "anti_p": p.new_anti_join_node, "anti_b": p.new_anti_join_node}[kind]
        p.root = mk(bl, 0, 1, 0, 0, o)
        p.new_input(pl.make_table(lcols))
        p.new_input(pl.make_table(rcols))
        plans[kind] = p
    built_pos = [k for k, i in enumerate(outs) if (i < lw) == build_left]
    return plans, built_pos


def _check_identities(bcols, pcols, build_left, outs):
    plans, built_pos = _plans(bcols, pcols, build_left, outs)
    (m, pairs), (u, pad_b), (v, pad_p) = _fullref.split_full(plans["full"])
    n, cols = _fullref.evaluate(plans["full"])
    want_inner = _oracle.execute(plans["inner"])
    want_outer = _outerref.execute(plans["outer"])
    want_anti_p = _filterref.execute(plans["anti_p"])
    want_anti_b = _filterref.execute(plans["anti_b"])
    assert (m, u, v) == (want_inner.num_rows, want_anti_p.num_rows, want_anti_b.num_rows)
    assert n == m + u + v
    _fullref.same(_fullref.to_table(m, pairs), want_inner, "pairs vs the oracle's inner join")
    head = [_filterref._take(c, np.arange(m + u)) for c in cols]
    _fullref.same(_fullref.to_table(m + u, head), want_outer, "pairs + rows padded on the built side vs OUTER")
    probed_pos = [k for k in range(len(outs)) if k not in built_pos]
    for k in built_pos:
        assert not pad_b[k][2].any()
    for k in probed_pos:
        assert not pad_p[k][2].any()
    _fullref.same(_fullref.to_table(u, [pad_b[k] for k in probed_pos]), want_anti_p, "built-side NULL rows vs ANTI")
    _fullref.same(_fullref.to_table(v, [pad_p[k] for k in built_pos]), want_anti_b, "probed-side NULL rows vs ANTI")
    # build_left is a hint: the same children and outputs built the other way give the same multiset
    swapped, _ = _plans(pcols, bcols, not build_left, outs)
    _fullref.same(_fullref.execute(swapped["full"]), _fullref.execute(plans["full"]), "build_left swapped")
    return m, u, v


@pytest.mark.parametrize("seed", range(9))
def test_fullref_identities_random(seed):
    rng = np.random.default_rng(500 + seed)
    kt = [I32, I64, F64][seed % 3]
    nb, npr = int(rng.integers(1, 2500)), int(rng.integers(1, 4000))
    dom = max(1, int(nb * rng.uniform(0.6, 2.5)))

    def keys(n):
        k = rng.integers(-dom // 2, dom - dom // 2, n)
        if kt == F64:
            k = k * 0.25 + 0.125
            put = rng.random(n) < 0.05
            sp = _fp64_specials()
            k[put] = sp[rng.integers(0, len(sp), int(put.sum()))]
        elif kt == I64:
            k = k * 3_000_000_019
        return k.astype(NP_OF[kt])

    bcols = [(kt, keys(nb), rng.random(nb) >= 0.1), (I64, rng.integers(-2**40, 2**40, nb)),
             (F64, rng.standard_normal(nb), rng.random(nb) >= 0.2)]
    pcols = [(kt, keys(npr), rng.random(npr) >= 0.1), (I32, rng.integers(-9, 9, npr).astype(np.int32))]
    build_left = seed % 4 < 2
    nl = len(bcols) if build_left else len(pcols)
    outs = list(range(len(bcols) + len(pcols))) if seed % 2 else [nl + 1, 0, 2, nl, 1]
    m, u, v = _check_identities(bcols, pcols, build_left, outs)
    assert m > 0 and u > 0 and v > 0


@pytest.mark.parametrize("kt", [I32, I64, F64])
def test_fullref_identities_adversarial(kt):
    """Keys sharing their low hash bits, duplicates on both sides, NULL keys, NaNs."""
    rng = np.random.default_rng(23 + kt)
    mask = 0xFFFFFFFF if kt != I32 else 0xFFF
    distinct = hs.keys_with_hash_bits(600, NP_OF[kt], 0x2A5, mask, rng=rng)
    if kt == F64:
        distinct = np.concatenate([distinct, _fp64_specials()])
    bk = np.concatenate([distinct[:400], distinct[:50], distinct[:5]])
    pk = np.concatenate([rng.choice(distinct[200:], 1500), distinct[200:220]])
    bcols = [(kt, bk, rng.random(bk.shape[0]) >= 0.05), (I32, np.arange(bk.shape[0], dtype=np.int32))]
    pcols = [(kt, pk, rng.random(pk.shape[0]) >= 0.05), (I64, np.arange(pk.shape[0], dtype=np.int64))]
    for build_left in (True, False):
        m, u, v = _check_identities(bcols, pcols, build_left, [0, 1, 2, 3])
        assert m > 0 and u > 0 and v > 0


def test_fullref_edges():
    k = np.arange(5, dtype=np.int32)
    pay = (I32, np.arange(5, dtype=np.int32) + 10)
    e = np.zeros(0, dtype=np.int32)
    # key types differ: every row of both children is unmatched
    assert _check_identities([(I64, k.astype(np.int64)), pay], [(I32, k), pay], True, [0, 1, 2, 3]) == (0, 5, 5)
    # either child empty: every row of the other one, padded
    for build_left in (True, False):
        assert _check_identities([(I32, e), (I32, e)], [(I32, k), pay], build_left, [0, 1, 2, 3]) == (0, 5, 0)
        assert _check_identities([(I32, k), pay], [(I32, e), (I32, e)], build_left, [0, 1, 2, 3]) == (0, 0, 5)
    # both empty
    plans, _ = _plans([(I32, e), (I32, e)], [(I32, e), (I32, e)], True, [0, 1, 2, 3])
    n, cols = _fullref.evaluate(plans["full"])
    assert n == 0 and [c[0] for c in cols] == [I32] * 4
