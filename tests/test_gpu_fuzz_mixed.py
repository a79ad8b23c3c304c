"""Differential fuzzing of plans that mix all six node kinds: tests/_plangen.mixed_plan(seed) through
the C-ABI against the numpy reference tests/_aggref.py (tests/test_mixed_plan_ref.py pins that
reference, on the same seeds, against an independent row-at-a-time one and against the C oracle, and
proves on the CPU that no seed is too large: nothing here skips).

Row count, column types and the sorted row multiset (pl.canonical_rows) are compared; mid plans above
50 000 result rows go by pl.table_digest, as tests/test_gpu_agg.py's check does.  The small plans run
through ONE context, so hundreds of nodes of every kind share its buffer pool; the same plans run
under forced radix bits (the only way small inputs leave the broadcast kernels), with the XCD-aware
placement forced on, and with RJ_TUNE_WIDE_CARRY=0 (OUTER / FULL optional sides then travel as row
indices padded with OUTER_NO_ROW; AGG ignores the switch).  The mid plans reach the partitioned
kernels and both sides of the JN_RMAX cut by their sizes alone; the launch log proves it.

RJ_MIXED_SEEDS="first:count" widens the sweep of the small plans for soak runs."""
import functools
import os

import pytest

import _aggref
import _pagecheck
import _plangen
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

_FIRST, _COUNT = (int(x) for x in os.environ.get("RJ_MIXED_SEEDS", "0:300").split(":"))
BITS = [3, 11, 17, 20]  # one pass; two with the fine histogram; two above its LDS limit; three passes
MID = range(20)
# kind -> (partitioned kernel family, broadcast kernel family): tests/test_gpu_kernel_matrix.py,
# test_gpu_filter_join.py, test_gpu_outer_join.py, test_gpu_full_outer_join.py (FAMILIES)
PROBE_FAMILY = {"join": ("k_join", "k_join_bcast"), "semi": ("k_filter_join", "k_filter_bcast"),
                "anti": ("k_filter_join", "k_filter_bcast"), "outer": ("k_outer_join", "k_outer_bcast"),
                "full": ("k_full_join", "k_full_bcast")}
MID_FAMILIES = ("k_filter_join", "k_outer_join", "k_full_join", "k_full_unmatched", "k_agg_parts", "k_agg_emit", "k_join",
                "k_join_bcast", "k_filter_bcast", "k_outer_bcast", "k_full_bcast")
mid_launched = {}  # seed -> families, filled by test_mixed_plan_mid


@pytest.fixture(scope="module")
def ctx():
    c = capi.build_context()
    yield c
    capi.destroy_context(c)


@functools.lru_cache(maxsize=None)
def case(seed, size="small"):
    """-> (plan, reference result): computed once, shared by the tests, never changed."""
    p = _plangen.mixed_plan(seed, size=size)
    return p, _aggref.execute(p)


@functools.lru_cache(maxsize=None)
def want_rows(seed, size="small"):
    return pl.canonical_rows(case(seed, size)[1])


def same(got, seed, size="small", what=""):
    want = case(seed, size)[1]
    assert got.num_rows == want.num_rows, (seed, what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], (seed, what)
    # every result column by the strict reader (tests/_pagecheck.py), which must decode what pyrj.pages decodes
    assert _pagecheck.same_as(_pagecheck.check_table(got), pl.decode_table(got)), (seed, what)
    if want.num_rows <= 50_000 or any(c.type == pl.VARCHAR for c in want.columns):
        assert pl.canonical_rows(got) == want_rows(seed, size), (seed, what)
    else:
        assert pl.table_digest(got) == pl.table_digest(want), (seed, what)


def tuned_context(env, **kw):
    """A context created under tuning variables (read once, when the context is created)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.Context(**kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run_on(c, seed):
    try:
        return capi.execute(case(seed)[0], c)
    finally:
        c.destroy()


@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + _COUNT))
def test_mixed_plan(ctx, seed):
    same(capi.execute(case(seed)[0], ctx), seed)


# AGG clamps the forced bits to 1 ... 21 as the joins do (agg_bits in rj_exec.hip)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + min(_COUNT, 60)))
def test_mixed_plan_forced_radix(seed, bits):
    same(run_on(capi.Context(radix_bits=bits), seed), seed, what=bits)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + min(_COUNT, 25)))
def test_mixed_plan_forced_radix_xcd_placement(seed, bits):
    same(run_on(tuned_context({"RJ_TUNE_XCD_MIN_ROWS": "0"}, radix_bits=bits), seed), seed, what=bits)


@pytest.mark.parametrize("bits", [0, 11])
@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + min(_COUNT, 60)))
def test_mixed_plan_row_index_carries(seed, bits):
    same(run_on(tuned_context({"RJ_TUNE_WIDE_CARRY": "0"}, radix_bits=bits), seed), seed, what=bits)


@pytest.mark.parametrize("seed", MID)
def test_mixed_plan_mid(seed):
    p, _ = case(seed, "mid")
    c = capi.Context()
    try:
        c.launch_log(True)
        got = capi.execute(p, c)
        ran = {n.split("<")[0] for n in km.launched(c)}
    finally:
        c.destroy()
    same(got, seed, "mid")
    mid_launched[seed] = ran
    # every binary node whose build side is above JN_RMAX rows left the broadcast kernels — unless it
    # has nothing to probe or its keys are of two types, which needs no table at all
    # (_plangen.probe_forms); every other node that probes took the broadcast kernel; an aggregation
    # over a child with rows partitions it
    for kind, form in _plangen.probe_forms(p):
        if form != "none":
            assert PROBE_FAMILY[kind][form == "bcast"] in ran, (seed, kind, form, sorted(ran))
    rows = _plangen.relation_rows(p)
    for i in _plangen.reachable(p):
        if _plangen.kind_of(p.nodes[i]) == "agg" and rows[p.nodes[i].data.child]:
            assert "k_agg_parts" in ran, (seed, sorted(ran))


def test_mid_plans_launched_every_family():
    assert sorted(mid_launched) == list(MID), "runs after test_mixed_plan_mid, in one process"
    ran = set().union(*mid_launched.values())
    assert not [f for f in MID_FAMILIES if f not in ran], sorted(ran)


def test_same_plan_twice_on_one_context(ctx):
    """State the first run leaves in pooled buffers (FULL's matched bits, the zeroed counters, AGG's
    merge table) must not reach the second, nor a run over resident tables that keeps its result on
    the device."""
    seeds = []
    for seed in range(300):
        if {"full", "agg"} & {_plangen.kind_of(n) for n in case(seed)[0].nodes}:
            seeds.append(seed)
        if len(seeds) == 10:
            break
    assert len(seeds) == 10
    for seed in seeds:
        p = case(seed)[0]
        same(capi.execute(p, ctx), seed, what="first")
        same(capi.execute(p, ctx), seed, what="second")
        tables = [ctx.upload(t) for t in p.inputs]
        try:
            r = ctx.execute_resident(p, tables, keep_on_device=True)
            try:
                same(r.to_table(), seed, what="resident")
            finally:
                r.free()
        finally:
            for t in tables:
                t.release()
