"""The last radix pass of a big inner join without its histogram (csrc/rj_partition.hip: k_last_sample, k_last_caps,
k_last_scatter*, k_last_close; csrc/rj_radix_plan.cpp: `spec2`, csrc/rj_radix.hip: sample_last; csrc/rj_exec.hip: repartition_exact; csrc/rj_join.hip and
k_heavy_tasks: a partition is [begin[q], end[q])).

Behind a speculative first pass, an inner join's last pass sizes the final partitions from a sample of the first
pass' output (1/4 by default; every case here sets RJ_TUNE_SPEC2_SAMPLE=3, 1/8, whose slices of 2048 rows the
constructed cases are built around) plus a margin of z = 7, checks the room in the scatter's reservation, and sends the side back to the
exact path (both passes) when a partition turns out too small.  The join then reads partitions with unused room
behind them.  The pattern is test_gpu_spec_pass1's: a plan through the public API on a fresh context, knobs in the
environment around its creation, XCD placement and BOTH speculative passes forced on for inputs of any size, the
launch log on, the result compared with the reference's as a multiset and its row count with the count worked out
from the keys.  Sizes are test_gpu_spec_pass1.SIZES (3t, 20t) with one exception (forced_overflow below).  Radix bits
are 5 + 5 (with RJ_TUNE_FINE=0: 10 bits would otherwise take the fine histogram) and 9 + 8; 9 + 9, the benchmark's
split, in one case per shape only: with 2^18 bins the z^2 / 2 term of the host's bound allocates some hundred MB per
relation whatever the input size.

  taken            random keys: the log names the new sample kernel and the new scatter once per side, the
                   speculative first pass, and no exact histogram or scatter of either pass
  forced_overflow  RJ_TUNE_SPEC2_Z=0.  No margin overflows only where the sample is a FAIR 1/8: a tile of at most a
                   slice (2048 rows) is read whole and a partial tile's slice is more than 1/8 of it, yet either
                   count is multiplied by 8 — so at SIZES, where no input segment of the second pass reaches two
                   whole tiles under any bit split, a capacity of 8 x the count exceeds every partition and nothing
                   overflows.  The case therefore runs 32 tiles + 1029 rows per side without NULL keys with the bits
                   split 1 + 9 (RJ_TUNE_P1_BITS=1): 16 input segments of two whole tiles and a few rows each, 1024
                   final partitions of about 512 tuples whose capacity 8 c (c: binomial, mean 64, deviation 7.5)
                   is too small for about half of them.  The log shows the new sample kernel and the exact
                   histograms of both passes
  first_pass_overflow / both   RJ_TUNE_SPEC_Z=0 with the last pass' margin at its default, and both at 0
  hidden (must fall back at the default margin)   see hidden_sides(): 6000 rows of one key that the first pass'
                   sample sees in proportion and the last pass' sample cannot see at all
  must not fall back   test_taken at 20t: random keys, every partition's count is binomial and the margin is 7
                   deviations plus z^2 / 2, so the room is short with probability < 2^18 Phi(-7) ~ 3e-7 per side
  skew             gaps seen by the join: one key owning 70 000 probe rows (above JN_HEAVY = 65536: k_heavy_tasks cuts
                   a partition with room behind it) and one owning 4500 build rows (above 4096: the chunked build),
                   in random order.  Empty final partitions, partitions of one tuple and NULL keys are in every
                   case: 3t puts 50 000 rows, 2 % of them NULL, into 2^17 or 2^18 partitions
  poison           RJ_DEBUG_POISON with a taken run of each shape: the unused room holds the fill pattern, which a
                   join that read past end[q] would carry into the result
  reuse            one context: the hidden case (overflows in the last pass), then two executes that do not; and
                   two executes on one context that both overflow
  join_kinds       semi, anti, left outer and full outer joins under the same knobs: the exact second pass and none
                   of the new kernels
  default_thresholds   RJ_TUNE_SPEC2_MIN_ROWS unset: the log is what test_gpu_spec_pass1 expects"""
import numpy as np
import pytest

import test_gpu_scatter_rank as sr
import test_gpu_spec_pass1 as sp1
from pyrj import hashing
from test_gpu_kernel_matrix import launched
from pyrj import capi

pytestmark = pytest.mark.gpu

PT_TILE = sr.PT_TILE
I32, I64 = sp1.I32, sp1.I64
S2 = 3  # RJ_TUNE_SPEC2_SAMPLE, set explicitly: the cases below are built around slices of PT_TILE >> 3 = 2048 rows
BOTH = dict(sp1.TAKEN, RJ_TUNE_SPEC2_MIN_ROWS="1", RJ_TUNE_SPEC2_SAMPLE=str(S2), RJ_TUNE_FINE="0")
SIZES = dict(sp1.SIZES, **{"32t": (32 * PT_TILE + 1029, 32 * PT_TILE + 1029)})

# the new families and, per shape, the instantiations a taken run launches once per side
FAMILIES = ("k_last_sample", "k_last_caps", "k_last_scatter", "k_last_scatter_packed", "k_last_close")
NEW = {
    "i32_i64": ("k_last_sample<DenseLoaderT<-1>>", "k_last_scatter<3,DenseLoaderT<1>,1>"),
    "i32_i32": ("k_last_sample<BlockedLoader>", "k_last_scatter_packed<BlockedLoader>"),
}
AUX = ("k_last_caps<0>", "k_last_caps<1>", "k_last_close")  # every taken run, once per side
EXACT_HIST = sp1.EXACT_HIST


def expected_instantiations():
    return {k for pair in NEW.values() for k in pair} | set(AUX)


def run(p, env, bits, ctx=None):
    c = ctx or sp1.context(env, radix_bits=bits)
    try:
        c.launch_log(True)
        got = capi.execute(p, c)
        ran = launched(c)
        c.launch_log(False)
    finally:
        if ctx is None:
            c.destroy()
    return got, ran


def new_kernels(ran):
    return sorted(k for k in ran if k.split("<")[0] in FAMILIES)


def took_both(ran, shape):
    _, _, spec1, exact1, second = sp1.SHAPES[shape]
    for k in (sp1.SAMPLE, spec1) + NEW[shape] + AUX:
        assert ran.get(k) == 2, (k, sorted(ran.items()))  # once per side
    unwanted = [k for k in (EXACT_HIST, exact1) + second if k in ran]
    assert not unwanted, (unwanted, sorted(ran))


def fell_back(ran, shape, sides=None):
    """The last pass was tried and the exact histograms of both passes ran (`sides`: for how many sides).  The launch
    log is a count per kernel handle (LaunchLog: a map, rj_internal.hpp), so the ORDER of launches cannot be
    observed from a test.  That the sample came first follows from the counts: the exact histograms run only in
    repartition_exact, which nothing reaches before an attempt — sample, scatter, join — has raised the flag; a
    side that went straight to the exact path would show no k_last_sample launch for it, and the callers assert
    two."""
    _, _, spec1, exact1, second = sp1.SHAPES[shape]
    missing = [k for k in (sp1.SAMPLE, spec1, NEW[shape][0], EXACT_HIST, exact1) + second if k not in ran]
    assert not missing, f"expected {missing} to run; the launch log holds {sorted(ran)}"
    if sides is not None:
        assert ran[EXACT_HIST] == ran[second[0]] == sides, sorted(ran.items())
    assert ran[NEW[shape][0]] == 2, sorted(ran.items())  # the speculative attempt ran on both sides


def hot_sides(kt, rng):
    """Random sides at 20t, but 70 000 probe rows in random places hold one build key and 4500 build rows in random
    places hold another, which three probe rows have."""
    bk, bv, pk, pv = sp1.random_sides(kt, "20t", rng)
    at = rng.permutation(pk.shape[0])
    pk[at[:70_000]] = bk[11]
    pv[at[:70_000]] = True
    bt = rng.permutation(bk.shape[0])
    bt = bt[(bt != 11)][:4500]
    heavy_build = sr.keys_of(kt, [10**6 + 1])[0]
    bk[bt] = heavy_build
    bv[bt] = True
    pk[at[70_000:70_003]] = heavy_build
    pv[at[70_000:70_003]] = True
    return bk, bv, pk, pv


HIDDEN_ENV = dict(BOTH, RJ_TUNE_TPG1="8")
HIDDEN_BITS = 10


def hidden_sides(kt, rng):
    """The definite overflow of the LAST pass at the default margins, bits 5 + 5, RJ_TUNE_TPG1=8.

    With eight tiles per workgroup the probe side's first pass has three workgroups; workgroup 0 walks tiles 0..7 one
    after the other and appends each tile's run of first digit 0 to sub-range (digit 0, x = 0), which nobody else
    writes: that sub-range is the runs of tiles 0..7 IN TILE ORDER (the order inside a run is not fixed).  It is the
    first input segment of the last pass, so it starts at tuple 0, holds one partial tile (about 10 000 tuples), and
    the slice of that tile is at rot = 0: tuples [0, 2048).  Tiles 0..4 bring at least 2300 valid rows of digit 0
    (asserted below from the device hash), so the slice sees only them.  One key of first digit 0 owns every second
    row of [0, 12000) of tile 5: 6000 rows.
      * The first pass' sample reads rows [1536, 2048) of tile 5 and sees 256 of them, in proportion: its sub-range
        gets room for about 16 000 tuples and holds about 10 000.  The control run (RJ_TUNE_SPEC_P2=0) shows no
        fallback.
      * The last pass' sample cannot see one of the 6000.  The key's final partition is sampled only from other
        rows of the same partition, of which the whole side has n_f (about 340, computed below): its capacity is at
        most 8 (n_f + 7 sqrt(n_f + 1) + 24.5) + 32 < 4100 whatever the sample holds, and it receives 6000 + n_f
        tuples.  The decision has more than 2000 tuples, over 60 rounding steps of 32, to spare (asserted below)."""
    bk, bv, pk, pv = sp1.random_sides(kt, "20t", rng)
    assert kt == I32

    def digit(k):  # the final partition: first digit in the low 5 bits of the device hash, second digit above it
        return hashing.key_hash(np.asarray(k, np.int32), False).astype(np.int64) & 1023

    hot = bk[np.flatnonzero((digit(bk) & 31) == 0)[0]]
    rows = 5 * PT_TILE + 2 * np.arange(6000)
    pk[rows] = hot
    pv[rows] = True
    d = digit(pk)
    mine = pv.copy()  # every other valid row (a stray row of the same key elsewhere counts as one of them)
    mine[rows] = False
    assert int((mine[: 5 * PT_TILE] & ((d[: 5 * PT_TILE] & 31) == 0)).sum()) >= 2300
    n_f = int((mine & (d == digit([hot])[0])).sum())
    cap_max = 8 * (n_f + 7 * np.sqrt(n_f + 1) + 24.5) + 32
    assert 6000 + n_f > cap_max + 2000, (n_f, cap_max)
    return bk, bv, pk, pv


_CASES = {}


def case(shape, data, size="3t"):
    """(plan, reference result, expected row count): built once and left unchanged."""
    if data == "random" and size in sp1.SIZES:
        return sp1.case(shape, data, size)
    key = (shape, data, size)
    if key not in _CASES:
        kt, ct = sp1.SHAPES[shape][:2]
        rng = np.random.default_rng(8803 + 97 * sorted(NEW).index(shape) + 7 * len(data) + len(size))
        if data == "random":  # 32t: no NULL keys (see forced_overflow above)
            nb, npr = SIZES[size]
            dom = nb * 3 // 4
            bk = sr.keys_of(kt, rng.permutation(np.concatenate([np.arange(dom), rng.integers(0, dom, nb - dom)])))
            pk = sr.keys_of(kt, rng.integers(0, int(dom * 1.25), npr))
            bv, pv = np.ones(nb, bool), np.ones(npr, bool)
        else:
            bk, bv, pk, pv = {"skew": hot_sides, "hidden": hidden_sides}[data](kt, rng)
        p = sp1.join_plan(kt, ct, bk, bv, pk, pv, rng)
        _CASES[key] = (p, sp1._oracle.execute(p), sr.expected_rows(bk, bv, pk, pv))
    return _CASES[key]


@pytest.mark.parametrize("size,bits", [("3t", 10), ("3t", 17), ("3t", 18), ("20t", 10), ("20t", 17)])
@pytest.mark.parametrize("shape", sorted(NEW))
def test_taken(shape, size, bits):
    p, want, rows = case(shape, "random", size)
    got, ran = run(p, BOTH, bits)
    took_both(ran, shape)
    sp1.same_join(got, want, rows)


OVERFLOW2 = dict(BOTH, RJ_TUNE_SPEC2_Z="0", RJ_TUNE_P1_BITS="1")


@pytest.mark.parametrize("shape", sorted(NEW))
def test_forced_overflow(shape):
    p, want, rows = case(shape, "random", "32t")
    got, ran = run(p, OVERFLOW2, 10)
    fell_back(ran, shape, sides=2)
    sp1.same_join(got, want, rows)


@pytest.mark.parametrize("env", ["first", "both"])
@pytest.mark.parametrize("shape", sorted(NEW))
def test_first_pass_overflow(shape, env):
    p, want, rows = case(shape, "random", "20t")
    knobs = dict(BOTH, RJ_TUNE_SPEC_Z="0", **({"RJ_TUNE_SPEC2_Z": "0"} if env == "both" else {}))
    got, ran = run(p, knobs, 17)
    fell_back(ran, shape, sides=2)
    sp1.same_join(got, want, rows)


@pytest.mark.parametrize("shape", sorted(NEW))
def test_hidden_rows_fall_back(shape):
    p, want, rows = case(shape, "hidden", "20t")
    got, ran = run(p, dict(HIDDEN_ENV, RJ_TUNE_SPEC_P2="0"), HIDDEN_BITS)  # the control: the first pass is clean
    assert EXACT_HIST not in ran and not new_kernels(ran), sorted(ran)
    sp1.same_join(got, want, rows)
    got, ran = run(p, HIDDEN_ENV, HIDDEN_BITS)
    fell_back(ran, shape, sides=1)  # the probe side alone is partitioned again
    assert ran[NEW[shape][0]] == 2, ran
    sp1.same_join(got, want, rows)


@pytest.mark.parametrize("shape", sorted(NEW))
def test_skew_gaps_seen_by_the_join(shape):
    p, want, rows = case(shape, "skew", "20t")
    got, ran = run(p, BOTH, 17)
    took_both(ran, shape)  # (random order: both samples see the heavy keys in proportion)
    assert ran.get("k_heavy_tasks", 0) >= 1, sorted(ran)
    sp1.same_join(got, want, rows)


@pytest.mark.parametrize("shape", sorted(NEW))
def test_poison(shape):
    p, want, rows = case(shape, "random", "20t")
    got, ran = run(p, dict(BOTH, RJ_DEBUG_POISON="0x15A"), 17)
    took_both(ran, shape)
    sp1.same_join(got, want, rows)


@pytest.mark.parametrize("shape", sorted(NEW))
def test_reuse(shape):
    hidden_rows = case(shape, "hidden", "20t")
    random_rows = case(shape, "random", "20t")
    ctx = sp1.context(HIDDEN_ENV, radix_bits=HIDDEN_BITS)
    try:
        got, ran = run(hidden_rows[0], None, None, ctx)
        fell_back(ran, shape, sides=1)
        sp1.same_join(got, *hidden_rows[1:])
        for _ in range(2):
            got, ran = run(random_rows[0], None, None, ctx)
            took_both(ran, shape)
            sp1.same_join(got, *random_rows[1:])
    finally:
        ctx.destroy()
    big = case(shape, "random", "32t")
    ctx = sp1.context(OVERFLOW2, radix_bits=10)
    try:
        for _ in range(2):
            got, ran = run(big[0], None, None, ctx)
            fell_back(ran, shape, sides=2)
            sp1.same_join(got, *big[1:])
    finally:
        ctx.destroy()


@pytest.mark.parametrize("kind", sorted(sp1.KIND_KERNELS))
def test_other_join_kinds_keep_the_exact_last_pass(kind):
    if kind not in sp1._KINDS:
        p, ref = sp1.kind_plan(kind)
        sp1._KINDS[kind] = (p, ref, ref.execute(p))
    p, ref, want = sp1._KINDS[kind]
    got, ran = run(p, dict(sp1.TAKEN, RJ_TUNE_SPEC2_MIN_ROWS="1"), sp1.RADIX_BITS)
    assert any(k.startswith(sp1.KIND_KERNELS[kind] + "<") for k in ran), sorted(ran)
    assert not new_kernels(ran), new_kernels(ran)
    assert ran.get(sp1.SAMPLE) == 2 and EXACT_HIST not in ran, sorted(ran)
    assert sum(n for k, n in ran.items() if k.startswith("k_pass_hist<")) == 2, sorted(ran)  # the exact second pass
    (sp1.fj.same if ref is sp1._filterref else ref.same)(got, want, kind)


@pytest.mark.parametrize("shape", sorted(NEW))
def test_default_thresholds(shape):
    p, want, rows = case(shape, "random", "20t")
    got, ran = sp1.run(p, sp1.TAKEN)  # RJ_TUNE_SPEC2_MIN_ROWS unset
    sp1.took_the_path(ran, shape)
    assert not new_kernels(ran), new_kernels(ran)
    sp1.same_join(got, want, rows)
