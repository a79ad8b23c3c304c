"""A context built with prewarm=True (RJ_CTX_PREWARM, what bench.py and Contest::build_context() use) loads
the code object of every kernel file of the join path (csrc/rj_pages.hip, rj_partition.hip, rj_join.hip, rj_bcast.hip,
rj_filter.hip, rj_outer.hip, rj_full.hip, rj_agg.hip, rj_select.hip), and rj_varchar_dev.hip's, before its first execute.
What is checked here is narrow: after those loads everything still computes correctly.  One plan per
kernel family on ONE such context, 12 000 probe rows with NULL keys on both sides against 5 000 build rows
— more than one LDS table holds (JN_RMAX), so the joins take the partition passes and the partitioned
kernels — and against 3 000, where they take the broadcast kernels; the launch log says which family
ran.  The inner join also runs on a prewarmed context with forced radix bits (the way
tests/test_gpu_kernel_matrix.py forces the partitioned path at small sizes).  Inner joins against the C
oracle, the other node kinds against tests/_selectref.py, by pl.table_digest."""
import numpy as np
import pytest

import _oracle
import _selectref
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, VC = pl.INT32, pl.INT64, pl.VARCHAR
NB, NB_BCAST, NP = 5_000, 3_000, 12_000


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = capi.Context(prewarm=True, **kw)
        return made[key]

    yield get
    for c in made.values():
        c.destroy()


def _tables(nb):
    rng = np.random.default_rng(1907)
    bk = rng.integers(0, 4_000, nb).astype(np.int32)        # duplicates on the build side
    pk = rng.integers(0, 5_000, NP).astype(np.int32)        # a fifth of the probe keys miss
    b = [(I32, bk, rng.random(nb) >= 0.03), (I64, rng.integers(-2**62, 2**62, nb))]
    p = [(I32, pk, rng.random(NP) >= 0.03), (I32, np.arange(NP, dtype=np.int32))]
    return b, p


def _plan(kind, nb=NB):
    """b (nb rows: INT32 key, INT64 payload) is the built / filter / optional side, p (INT32 key, INT32 payload) the other"""
    b, p = _tables(nb)
    q = pl.Plan()
    sb = q.new_scan_node(0, [(0, I32), (1, I64)])
    sp = q.new_scan_node(1, [(0, I32), (1, I32)])
    q.new_input(pl.make_table(b))
    q.new_input(pl.make_table(p))
    both = [(0, I32), (1, I64), (2, I32), (3, I32)]
    if kind == "inner":
        q.root = q.new_join_node(True, sb, sp, 0, 0, [(0, I32), (1, I64), (3, I32)])
    elif kind == "semi":
        q.root = q.new_semi_join_node(True, sb, sp, 0, 0, both[2:])
    elif kind == "anti":
        q.root = q.new_anti_join_node(True, sb, sp, 0, 0, both[2:])
    elif kind == "left outer":  # p LEFT JOIN b
        q.root = q.new_outer_join_node(False, sp, sb, 0, 0, [(0, I32), (1, I32), (2, I32), (3, I64)])
    elif kind == "full outer":
        q.root = q.new_full_outer_join_node(True, sb, sp, 0, 0, both)
    elif kind == "agg":
        q.root = q.new_agg_node(sp, 0, [(pl.AGG_KEY, 0, I32), (pl.AGG_COUNT_STAR, 0, I64), (pl.AGG_SUM, 1, I64)])
    else:
        assert kind == "select over join"
        j = q.new_join_node(True, sb, sp, 0, 0, [(0, I32), (1, I64), (3, I32)])
        q.root = q.new_select_node(j, [("GT", 1, 0), ("LT", 2, NP // 2), ("AND",)], [(0, I32), (1, I64), (2, I32)])
    return q


def _check(ctx, plan, want, family):
    ctx.launch_log(True)
    try:
        got = capi.execute(plan, ctx)
        ran = km.launched(ctx)
    finally:
        ctx.launch_log(False)
    assert got.num_rows == want.num_rows > 0
    assert [c.type for c in got.columns] == [c.type for c in want.columns]
    assert pl.table_digest(got) == pl.table_digest(want)
    assert any(name.split("<")[0] == family for name in ran), (family, sorted(ran))


@pytest.mark.parametrize("kind, nb, family", [
    ("inner", NB, "k_join"), ("semi", NB, "k_filter_join"), ("anti", NB, "k_filter_join"), ("left outer", NB, "k_outer_join"),
    ("full outer", NB, "k_full_join"), ("agg", NB, "k_agg_parts"), ("select over join", NB, "k_select"),
    ("inner", NB_BCAST, "k_join_bcast"), ("semi", NB_BCAST, "k_filter_bcast"), ("anti", NB_BCAST, "k_filter_bcast"),
    ("left outer", NB_BCAST, "k_outer_bcast"), ("full outer", NB_BCAST, "k_full_bcast"),
    ("inner", NB, "k_pass_scatter"), ("inner", NB, "k_finish_streams")])
def test_prewarmed_context_computes_every_family(contexts, kind, nb, family):
    plan = _plan(kind, nb)
    want = _oracle.execute(plan) if kind == "inner" else _selectref.execute(plan)
    _check(contexts(), plan, want, family)


def test_prewarmed_context_partitioned_inner_join(contexts):
    plan = _plan("inner")
    _check(contexts(radix_bits=8), plan, _oracle.execute(plan), "k_join")


def test_prewarmed_context_varchar_key_join(contexts):
    rng = np.random.default_rng(1908)
    word = lambda k: None if rng.random() < 0.03 else b"w%d" % k
    bt = pl.make_table([(VC, [word(int(k)) for k in rng.integers(0, 4_000, NB)]), (I64, rng.integers(-2**62, 2**62, NB))])
    pt = pl.make_table([(VC, [word(int(k)) for k in rng.integers(0, 5_000, NP)]), (I32, np.arange(NP, dtype=np.int32))])
    q = pl.Plan()
    sb = q.new_scan_node(0, [(0, VC), (1, I64)])
    sp = q.new_scan_node(1, [(0, VC), (1, I32)])
    q.new_input(bt)
    q.new_input(pt)
    q.root = q.new_join_node(True, sb, sp, 0, 0, [(1, I64), (3, I32)])
    _check(contexts(), q, _oracle.execute(q), "k_vc_hash")
