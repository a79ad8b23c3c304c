"""The first radix pass without its histogram (csrc/rj_partition.hip: k_pass_sample, k_spec_caps, k_spec_scatter*,
k_spec_close; csrc/rj_radix_plan.cpp: `spec`, csrc/rj_radix.hip: sample_first; csrc/rj_exec.hip: repartition_exact).

A join's big two-pass plans size the 4096 output sub-ranges of the first pass from a 1/32 sample of the keys plus a
safety margin, check the room in the scatter's reservation, and fall back to the exact histogram path when a
sub-range turns out too small.  Every case here is a plan through the public API on a fresh context with 18 radix
bits forced (two passes of 9), XCD placement and the speculative path forced on for inputs of any size and the
launch log on — the pattern, the sizes and the data makers of test_gpu_scatter_rank.py.  The result is compared
with the reference's as a multiset, its row count with the count worked out here from the keys.

  taken            random keys: the log names k_pass_sample, the speculative scatter and both second-pass kernels
                   (which read the sub-ranges as segments with gaps between them) and no histogram over the source;
                   at 3 tiles + 1029 rows, and at about 20 tiles per side so that every one of the eight sub-ranges
                   of a digit receives several tiles
  forced_overflow  RJ_TUNE_SPEC_Z=0 leaves no margin at all (capacity = 32 x the sample count), so about half of
                   the sub-ranges are too small: the runs that find no room go to the spare tile behind the
                   arrays, the flag comes back with the row count, and the log shows k_pass_sample followed by the
                   exact k_pass_hist<SrcLoader...>
  clustered        the probe side sorted by key, one key owning more than 5 whole tiles, at the default margin:
                   either path is right, only the result is asserted
  nulls ... all_digits   test_gpu_scatter_rank's data (its cases themselves, not copies): a sample slice that sees
                   nothing (null_tile), a sub-range that holds one tuple (tail_one), one digit owning the tile
  join_kinds       semi, anti, left outer and full outer joins, each taken and with the forced overflow
  poison           RJ_DEBUG_POISON: the room a sub-range does not use holds the fill pattern, which a second pass
                   that read beyond a sub-range's end would carry into the result
  reuse            one context: an execute that overflows at the default margin (one key owns 2500 rows of the probe
                   side's first tile, all outside that tile's sample slice, rows [0, 512): its sub-range gets room
                   for about 900) and then two that do not — no flag, cursor or capacity of the first may reach
                   the others (the block cache hands the same memory out again); and two executes on one context
                   that both overflow"""
import os

import numpy as np
import pytest

import _filterref
import _fullref
import _oracle
import _outerref
import test_gpu_filter_join as fj
import test_gpu_full_outer_join as fo
import test_gpu_outer_join as og
import test_gpu_scatter_rank as sr
from pyrj import capi
from pyrj import plan as pl
from test_gpu_kernel_matrix import S, SP, launched

pytestmark = pytest.mark.gpu

PT_TILE = sr.PT_TILE
I32, I64 = pl.INT32, pl.INT64
RADIX_BITS = sr.RADIX_BITS
TAKEN = dict(sr.KNOBS, RJ_TUNE_SPEC_MIN_ROWS="1")
OVERFLOW = dict(TAKEN, RJ_TUNE_SPEC_Z="0")
SIZES = {"3t": (sr.N_BUILD, sr.N_PROBE), "20t": (19 * PT_TILE + 4 * 1029 + 3, 20 * PT_TILE + 1029)}

SAMPLE = "k_pass_sample<1>"
# shape id -> (key type, payload type, the speculative scatter, the exact one, the second pass' histogram and scatter)
SHAPES = {
    "i32_i64": (I32, I64, "k_spec_scatter<3,SrcLoader<1,2,0>,1>", S(3, "SrcLoader<1,2,0>", 1, 0),
                ("k_pass_hist<DenseLoaderT<-1>>", S(3, "DenseLoaderT<1>", 1, 1))),
    "i32_i32": (I32, I32, "k_spec_scatter_packed<SrcLoader<1,1,0>,true>", SP("SrcLoader<1,1,0>", 1),
                ("k_pass_hist<BlockedLoader>", SP("BlockedLoader", 0))),
}
EXACT_HIST = "k_pass_hist<SrcLoader<1,0,0>>"


def context(env, radix_bits=RADIX_BITS):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # read once, when the context is created
    try:
        return capi.Context(radix_bits=radix_bits)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run(p, env, ctx=None):
    """-> (result, {instantiation: launches})"""
    c = ctx or context(env)
    try:
        c.launch_log(True)
        got = capi.execute(p, c)
        ran = launched(c)
        c.launch_log(False)
    finally:
        if ctx is None:
            c.destroy()
    return got, ran


def took_the_path(ran, shape):
    _, _, spec, exact, second = SHAPES[shape]
    missing = [k for k in (SAMPLE, spec) + second if k not in ran]
    assert not missing, f"expected {missing} to run; the launch log holds {sorted(ran)}"
    assert EXACT_HIST not in ran and exact not in ran, sorted(ran)
    assert ran[SAMPLE] == ran[spec] == 2  # once per side


def fell_back(ran, shape):
    _, _, spec, exact, second = SHAPES[shape]
    missing = [k for k in (SAMPLE, spec, EXACT_HIST, exact) + second if k not in ran]
    assert not missing, f"expected {missing} to run; the launch log holds {sorted(ran)}"


# ------------------------------------------------------------------ inner joins of the two shapes
def join_plan(kt, ct, bk, bv, pk, pv, rng):
    nb, npr = bk.shape[0], pk.shape[0]
    p = pl.Plan()
    ls = p.new_scan_node(0, [(0, kt), (1, ct)])
    rs = p.new_scan_node(1, [(0, kt), (1, ct)])
    p.root = p.new_join_node(True, ls, rs, 0, 0, [(0, kt), (1, ct), (3, ct)])
    p.new_input(pl.make_table([(kt, bk, bv), sr.payload(rng, ct, nb)]))
    p.new_input(pl.make_table([(kt, pk, pv), sr.payload(rng, ct, npr)]))
    return p


def random_sides(kt, size, rng):
    """Random keys with duplicates on both sides, a fifth of the probe keys without a partner, 2 % NULL keys."""
    nb, npr = SIZES[size]
    dom = nb * 3 // 4
    bk = np.concatenate([np.arange(dom), rng.integers(0, dom, nb - dom)])
    pk = rng.integers(0, int(dom * 1.25), npr)
    return sr.keys_of(kt, rng.permutation(bk)), rng.random(nb) >= 0.02, sr.keys_of(kt, pk), rng.random(npr) >= 0.02


def clustered_sides(kt, rng):
    """The probe side sorted by key, one key owning 5 tiles + 77 rows of it; the build side random."""
    nb, npr = SIZES["20t"]
    dom = nb * 3 // 4
    bk = rng.permutation(np.concatenate([np.arange(dom), rng.integers(0, dom, nb - dom)]))
    hot = 5 * PT_TILE + 77
    k = sr.keys_of(kt, np.concatenate([np.full(hot, dom // 2), rng.integers(0, int(dom * 1.25), npr - hot)]))
    return sr.keys_of(kt, bk), np.ones(nb, bool), np.sort(k), np.ones(npr, bool)


def hidden_sides(kt, rng):
    """Random sides, but rows [1000, 3500) of the probe side hold one key: the sample of that tile, rows [0, 512),
    does not see it."""
    bk, bv, pk, pv = random_sides(kt, "20t", rng)
    pk[1000:3500] = bk[5]
    pv[1000:3500] = True
    return bk, bv, pk, pv


_CASES = {}


def case(shape, data, size="3t"):
    """(plan, reference result, expected row count): built once and left unchanged."""
    key = (shape, data, size)
    if key not in _CASES:
        kt, ct = SHAPES[shape][:2]
        rng = np.random.default_rng(4421 + 97 * sorted(SHAPES).index(shape) + 7 * len(data) + len(size))
        if data == "random":
            bk, bv, pk, pv = random_sides(kt, size, rng)
        else:
            bk, bv, pk, pv = {"clustered": clustered_sides, "hidden": hidden_sides}[data](kt, rng)
        p = join_plan(kt, ct, bk, bv, pk, pv, rng)
        _CASES[key] = (p, _oracle.execute(p), sr.expected_rows(bk, bv, pk, pv))
    return _CASES[key]


def same_join(got, want, rows):
    assert want.num_rows == rows, (want.num_rows, rows)  # the reference itself
    assert got.num_rows == rows, (got.num_rows, rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns]
    assert pl.table_digest(got) == pl.table_digest(want)


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_taken(shape, size):
    p, want, rows = case(shape, "random", size)
    got, ran = run(p, TAKEN)
    took_the_path(ran, shape)
    same_join(got, want, rows)


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_forced_overflow(shape, size):
    p, want, rows = case(shape, "random", size)
    got, ran = run(p, OVERFLOW)
    fell_back(ran, shape)
    same_join(got, want, rows)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_clustered(shape):
    p, want, rows = case(shape, "clustered", "20t")
    got, ran = run(p, TAKEN)
    assert SAMPLE in ran, sorted(ran)
    same_join(got, want, rows)


@pytest.mark.parametrize("data", sr.DATA)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_scatter_rank_data(shape, data):
    p, want, rows = sr.case(shape, data)
    got, ran = run(p, TAKEN)
    assert SAMPLE in ran and SHAPES[shape][2] in ran, sorted(ran)
    same_join(got, want, rows)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_poison(shape):
    p, want, rows = case(shape, "random", "20t")
    got, ran = run(p, dict(TAKEN, RJ_DEBUG_POISON="0x15A"))
    took_the_path(ran, shape)
    same_join(got, want, rows)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_reuse(shape):
    hidden_rows = case(shape, "hidden", "20t")
    random_rows = case(shape, "random", "20t")
    ctx = context(TAKEN)
    try:
        got, ran = run(hidden_rows[0], None, ctx)
        fell_back(ran, shape)
        assert ran[EXACT_HIST] == 1, ran  # the probe side alone is partitioned again
        same_join(got, *hidden_rows[1:])
        for _ in range(2):
            got, ran = run(random_rows[0], None, ctx)
            took_the_path(ran, shape)
            same_join(got, *random_rows[1:])
    finally:
        ctx.destroy()
    ctx = context(OVERFLOW)
    try:
        for _ in range(2):
            got, ran = run(random_rows[0], None, ctx)
            fell_back(ran, shape)
            same_join(got, *random_rows[1:])
    finally:
        ctx.destroy()


# ------------------------------------------------------------------ the other join kinds
def kind_plan(kind):
    """-> (plan, its reference module): INT32 keys with NULLs on both sides, the preserved / probed side carries an
    INT64 payload (two carry words), sizes as above."""
    rng = np.random.default_rng(90210 + len(kind))
    bk, bv, pk, pv = random_sides(I32, "3t", rng)
    nb, npr = bk.shape[0], pk.shape[0]
    if kind in ("semi", "anti"):
        ppay = [sr.payload(rng, I64, npr)]
        return fj.filter_plan(fj.SEMI if kind == "semi" else fj.ANTI, I32, bk, bv, pk, pv, ppay), _filterref
    bcols = [(I32, bk, bv), sr.payload(rng, I32, nb)]
    pcols = [(I32, pk, pv), sr.payload(rng, I64, npr)]
    if kind == "outer":
        return og.outer_plan(bcols, pcols, build_left=False), _outerref  # probe LEFT JOIN build
    return fo.full_plan(bcols, pcols), _fullref


_KINDS = {}
KIND_KERNELS = {"semi": "k_filter_join", "anti": "k_filter_join", "outer": "k_outer_join", "full": "k_full_join"}


@pytest.mark.parametrize("env", ["taken", "forced_overflow"])
@pytest.mark.parametrize("kind", sorted(KIND_KERNELS))
def test_join_kinds(kind, env):
    if kind not in _KINDS:
        p, ref = kind_plan(kind)
        _KINDS[kind] = (p, ref, ref.execute(p))
    p, ref, want = _KINDS[kind]
    got, ran = run(p, TAKEN if env == "taken" else OVERFLOW)
    assert any(k.startswith(KIND_KERNELS[kind] + "<") for k in ran), sorted(ran)
    assert ran.get(SAMPLE) == 2 and sum(n for k, n in ran.items() if k.startswith("k_spec_scatter")) == 2, sorted(ran)
    assert (EXACT_HIST in ran) == (env == "forced_overflow"), sorted(ran)
    (fj.same if ref is _filterref else ref.same)(got, want, (kind, env))
