"""Outer join nodes (RJ_NODE_OUTER) without a GPU: plan marshalling, rj_plan_shardable, the kernel
handles librj.so compiles for them (tests/_elfsyms.py), and the numpy reference the GPU tests
compare against (tests/_outerref.py) tied to the pinned C oracle, which knows inner joins only:
  rows of the reference whose optional columns are valid  ==  the oracle's inner join of the plan,
  its padded rows                                          ==  _filterref's ANTI of the plan,
  and its row count is the sum of the two."""
import os
from collections import Counter

import numpy as np
import pytest

import _elfsyms
import _filterref
import _oracle
import _outerref
from pyrj import capi
from pyrj import hashing as hs
from pyrj import plan as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "radix-join_amd", "librj.so")
I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
NP_OF = {I32: np.int32, I64: np.int64, F64: np.float64}

# (KW, CWB, CWP) of k_outer_bcast / k_outer_join: KW = key words (1: INT32, 2: INT64 / FP64);
# CWB = carry words of the optional side: 0 nothing, 1 a row index, 2 / 3 a wide carry, which
# always ends with a validity word; CWP = carry words of the preserved side, as for any join.
# Each is bounded by MAX_WORDS - KW = 4 - KW.
OUTER_SHAPES = [(kw, b, p) for kw in (1, 2) for b in range(5 - kw) for p in range(5 - kw)]
NULLKEY_SHAPES = [(kw, p) for kw in (1, 2) for p in range(5 - kw)]


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
    f = p.new_outer_join_node(build_left, a, b, 0, 1 if build_left else 0, outs)
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
    assert pl.NODE_OUTER == 4
    p = _plan(build_left, under_join)
    cp, keep = pl.plan_to_c(p, with_inputs=False)
    nodes = [cp.nodes[i] for i in range(cp.n_nodes)]
    assert [n.kind for n in nodes] == ([0, 0, 4, 0, 1] if under_join else [0, 0, 4])
    f = nodes[2]
    assert (f.build_left, f.left, f.right, f.left_attr, f.right_attr) == (int(build_left), 0, 1, 0, 1 if build_left else 0)
    assert [f.out_idx[i] for i in range(f.n_out)] == [2, 3, 1]
    assert [f.out_type[i] for i in range(f.n_out)] == [I32, I64, I32]
    assert p.nodes[2].data == pl.OuterJoinNode(build_left, 0, 1, 0, 1 if build_left else 0)
    del keep


def test_older_constructors_keep_their_kinds():
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32)])
    b = p.new_scan_node(1, [(0, I32)])
    j = p.new_join_node(True, a, b, 0, 0, [(0, I32)])
    s = p.new_semi_join_node(True, a, b, 0, 0, [(1, I32)])
    t = p.new_anti_join_node(True, a, b, 0, 0, [(1, I32)])
    p.root = j
    cp, keep = pl.plan_to_c(p, with_inputs=False)
    assert [cp.nodes[i].kind for i in (j, s, t)] == [1, 2, 3]
    assert isinstance(p.nodes[j].data, pl.JoinNode) and isinstance(p.nodes[s].data, pl.FilterJoinNode)
    del keep


@pytest.mark.parametrize("under_join", [False, True])
def test_plans_with_outer_nodes_are_not_shardable(under_join):
    ok, why = capi.plan_shardable(_plan(under_join=under_join))
    assert not ok
    assert "outer" in why and "RJ_NODE_OUTER" in why


def test_plain_join_plan_stays_shardable():
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I32)])
    b = p.new_scan_node(1, [(0, I32), (1, I32)])
    p.root = p.new_join_node(True, a, b, 0, 0, [(0, I32), (1, I32), (3, I32)])
    assert capi.plan_shardable(p) == (True, "")


def test_abi_version_is_unchanged():
    assert capi.load().rj_abi_version() == 3


def test_library_holds_the_outer_kernel_families(handles):
    names = {_elfsyms.short_name(h) for h in handles}
    want = {f"{fam}<{kw},{b},{p}>" for fam in ("k_outer_bcast", "k_outer_join") for kw, b, p in OUTER_SHAPES}
    want |= {f"k_outer_nullkeys<{kw},{p}>" for kw, p in NULLKEY_SHAPES}
    want |= {"k_outer_gather<4>", "k_outer_gather<8>"}
    assert {n for n in names if n.startswith("k_outer_")} == want
    by = Counter(_elfsyms.family(h) for h in handles)
    assert (by["k_outer_bcast"], by["k_outer_join"], by["k_outer_nullkeys"], by["k_outer_gather"]) == (25, 25, 7, 2)


def test_pinned_families_are_unchanged(handles):
    """The outer join partitions with the inner join's shapes only and brings its own kernels."""
    by = Counter(_elfsyms.family(h) for h in handles)
    pinned = {"k_join": 83, "k_join_bcast": 25, "k_pass_hist": 7, "k_fine_hist": 4, "k_pass_scatter": 19,
              "k_pass_scatter_packed": 5, "k_filter_bcast": 7, "k_filter_join": 7, "k_filter_nullkeys": 7}
    assert {f: by[f] for f in pinned} == pinned


# ------------------------------------------------------- _outerref against the oracle + _filterref
def _fp64_specials():
    bits = [0x7FF0000000000001, 0x7FF8000000000000, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF,  # NaNs
            0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x800000000000000F,  # +-inf, subnormals
            0x8000000000000000]                                                              # -0.0 only
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _three_plans(ocols, pcols, build_left, outs):
    """The same inputs and output list under an outer join, an inner join and (preserved columns
    only) an anti join.  ocols / pcols: optional / preserved columns, the key first."""
    lcols, rcols = (ocols, pcols) if build_left else (pcols, ocols)
    both = [c[0] for c in lcols] + [c[0] for c in rcols]
    lw = len(lcols)
    plans = []
    for kind in ("outer", "inner", "anti"):
        p = pl.Plan()
        p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
        p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])
        o = [(i, both[i]) for i in outs]
        if kind == "anti":
            o = [(i, t) for i, t in o if (i >= lw) == build_left]
        mk = {"outer": p.new_outer_join_node, "inner": p.new_join_node, "anti": p.new_anti_join_node}[kind]
        p.root = mk(build_left, 0, 1, 0, 0, o)
        p.new_input(pl.make_table(lcols))
        p.new_input(pl.make_table(rcols))
        plans.append(p)
    return plans, [k for k, i in enumerate(outs) if (i < lw) == build_left]


def _check_identities(ocols, pcols, build_left, outs):
    (outer, inner, anti), opt_pos = _three_plans(ocols, pcols, build_left, outs)
    (m, matched), (u, padded) = _outerref.split_outer(outer)
    want_inner = _oracle.execute(inner)
    want_anti = _filterref.execute(anti)
    n, _ = _outerref.evaluate(outer)
    assert (m, u, n) == (want_inner.num_rows, want_anti.num_rows, want_inner.num_rows + want_anti.num_rows)
    _outerref.same(_outerref.to_table(m, matched), want_inner, "matched half vs the oracle's inner join")
    # the padded half: optional columns all NULL, the preserved ones are ANTI's rows
    for k in opt_pos:
        assert not padded[k][2].any()
    pres = [c for k, c in enumerate(padded) if k not in opt_pos]
    _outerref.same(_outerref.to_table(u, pres), want_anti, "padded half vs ANTI")
    return m, u


@pytest.mark.parametrize("seed", range(9))
def test_outerref_equals_oracle_plus_anti_random(seed):
    rng = np.random.default_rng(300 + seed)
    kt = [I32, I64, F64][seed % 3]
    no, npr = int(rng.integers(1, 2500)), int(rng.integers(1, 4000))
    dom = max(1, int(no * rng.uniform(0.3, 2.0)))

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

    ocols = [(kt, keys(no), rng.random(no) >= 0.1), (I64, rng.integers(-2**40, 2**40, no)),
             (F64, rng.standard_normal(no), rng.random(no) >= 0.2)]
    pcols = [(kt, keys(npr), rng.random(npr) >= 0.1), (I32, rng.integers(-9, 9, npr).astype(np.int32))]
    build_left = seed % 4 < 2
    nl = len(ocols) if build_left else len(pcols)
    outs = list(range(len(ocols) + len(pcols))) if seed % 2 else [nl + 1, 0, 2, nl, 1]
    m, u = _check_identities(ocols, pcols, build_left, outs)
    assert m > 0 and u > 0


@pytest.mark.parametrize("kt", [I32, I64, F64])
def test_outerref_equals_oracle_plus_anti_adversarial(kt):
    """Keys sharing their low hash bits, duplicates on both sides, NULL keys, NaNs."""
    rng = np.random.default_rng(17 + kt)
    mask = 0xFFFFFFFF if kt != I32 else 0xFFF
    distinct = hs.keys_with_hash_bits(600, NP_OF[kt], 0x2A5, mask, rng=rng)
    if kt == F64:
        distinct = np.concatenate([distinct, _fp64_specials()])
    ok = np.concatenate([distinct[:400], distinct[:50], distinct[:5]])
    pk = np.concatenate([rng.choice(distinct, 1500), distinct[:20]])
    ocols = [(kt, ok, rng.random(ok.shape[0]) >= 0.05), (I32, np.arange(ok.shape[0], dtype=np.int32))]
    pcols = [(kt, pk, rng.random(pk.shape[0]) >= 0.05), (I64, np.arange(pk.shape[0], dtype=np.int64))]
    for build_left in (True, False):
        m, u = _check_identities(ocols, pcols, build_left, [0, 1, 2, 3])
        assert m > 0 and u > 0


def test_outerref_edges():
    k = np.arange(5, dtype=np.int32)
    pay = (I32, np.arange(5, dtype=np.int32) + 10)
    # key types differ: every preserved row padded
    m, u = _check_identities([(I64, k.astype(np.int64)), pay], [(I32, k), pay], True, [0, 1, 2, 3])
    assert (m, u) == (0, 5)
    # an empty optional side
    e = np.zeros(0, dtype=np.int32)
    (outer, _, _), _ = _three_plans([(I32, e), (I32, e)], [(I32, k), pay], False, [0, 1, 2, 3])
    n, cols = _outerref.evaluate(outer)
    assert n == 5 and not cols[2][2].any() and not cols[3][2].any() and cols[0][2].all()
    # an empty preserved side
    (outer, _, _), _ = _three_plans([(I32, k), pay], [(I32, e), (I32, e)], True, [0, 1, 2, 3])
    assert _outerref.evaluate(outer)[0] == 0
