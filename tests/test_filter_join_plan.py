"""Semi and anti join nodes without a GPU: plan marshalling, rj_plan_shardable, and the kernel
handles librj.so compiles for them (tests/_elfsyms.py)."""
import ctypes as C
import os
from collections import Counter

import pytest

import _elfsyms
from pyrj import capi
from pyrj import plan as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "radix-join_amd", "librj.so")
I32, I64 = pl.INT32, pl.INT64


@pytest.fixture(scope="module")
def handles():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    return _elfsyms.kernel_handles(LIB)


def _plan(kind, build_left=True, under_join=False):
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I32)])
    b = p.new_scan_node(1, [(0, I32), (1, I64)])
    mk = p.new_semi_join_node if kind == pl.NODE_SEMI else p.new_anti_join_node
    outs = [(2, I32), (3, I64)] if build_left else [(0, I32), (1, I32)]
    f = mk(build_left, a, b, 0, 1 if build_left else 0, outs)
    p.root = f
    if under_join:
        c = p.new_scan_node(2, [(0, I32)])
        p.root = p.new_join_node(True, c, f, 0, 0, [(0, I32), (2, outs[1][1])])
    for _ in range(3):
        p.new_input(pl.make_table([(I32, [1, 2, 3]), (I32, [4, 5, 6])]))
    return p


@pytest.mark.parametrize("kind", [pl.NODE_SEMI, pl.NODE_ANTI], ids=["semi", "anti"])
@pytest.mark.parametrize("build_left", [True, False])
def test_marshalling_round_trips_kind(kind, build_left):
    p = _plan(kind, build_left, under_join=True)
    cp, keep = pl.plan_to_c(p, with_inputs=False)
    nodes = [cp.nodes[i] for i in range(cp.n_nodes)]
    assert [n.kind for n in nodes] == [0, 0, kind, 0, 1]
    f = nodes[2]
    assert (f.build_left, f.left, f.right, f.left_attr, f.right_attr) == (int(build_left), 0, 1, 0, 1 if build_left else 0)
    assert [f.out_idx[i] for i in range(f.n_out)] == [a for a, _ in p.nodes[2].output_attrs]
    assert p.nodes[2].data == pl.FilterJoinNode(kind, build_left, 0, 1, 0, 1 if build_left else 0)
    del keep


def test_new_join_node_keeps_its_kind():
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32)])
    b = p.new_scan_node(1, [(0, I32)])
    p.root = p.new_join_node(True, a, b, 0, 0, [(0, I32)])
    cp, keep = pl.plan_to_c(p, with_inputs=False)
    assert cp.nodes[2].kind == 1 and isinstance(p.nodes[2].data, pl.JoinNode)


@pytest.mark.parametrize("kind,name", [(pl.NODE_SEMI, "semi"), (pl.NODE_ANTI, "anti")])
@pytest.mark.parametrize("under_join", [False, True])
def test_plans_with_filter_nodes_are_not_shardable(kind, name, under_join):
    ok, why = capi.plan_shardable(_plan(kind, under_join=under_join))
    assert not ok
    assert name in why and ("RJ_NODE_SEMI" if kind == pl.NODE_SEMI else "RJ_NODE_ANTI") in why


def test_plain_join_plan_stays_shardable():
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, I32), (1, I32)])
    b = p.new_scan_node(1, [(0, I32), (1, I32)])
    p.root = p.new_join_node(True, a, b, 0, 0, [(0, I32), (1, I32), (3, I32)])
    assert capi.plan_shardable(p) == (True, "")


def test_abi_version_is_unchanged():
    assert capi.load().rj_abi_version() == 3


def test_library_holds_the_filter_kernel_families(handles):
    by = Counter(_elfsyms.family(h) for h in handles)
    # KW 1 with 0..3 preserved carry words, KW 2 with 0..2
    assert by["k_filter_bcast"] == 7 and by["k_filter_join"] == 7 and by["k_filter_nullkeys"] == 7
    names = {_elfsyms.short_name(h) for h in handles}
    for fam in ("k_filter_bcast", "k_filter_join", "k_filter_nullkeys"):
        for kw, cws in [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2)]:
            assert f"{fam}<{kw},{cws}>" in names


def test_pinned_join_families_are_unchanged(handles):
    """The semi / anti path partitions with the inner join's shapes only: no new instantiation of
    the six families the kernel matrix (test_gpu_kernel_matrix.py) pins."""
    by = Counter(_elfsyms.family(h) for h in handles)
    assert {f: by[f] for f in ("k_join", "k_join_bcast", "k_pass_hist", "k_fine_hist", "k_pass_scatter",
                               "k_pass_scatter_packed")} == {
        "k_join": 83, "k_join_bcast": 25, "k_pass_hist": 7, "k_fine_hist": 4, "k_pass_scatter": 19,
        "k_pass_scatter_packed": 5}
