"""Every compiled instantiation of the speculative first pass (k_pass_sample, k_spec_scatter, k_spec_scatter_packed:
csrc/rj_partition.hip), driven against the oracle — the table of test_gpu_kernel_matrix.py for the three families it
does not know.

A row is a test_gpu_kernel_matrix.Case (its data: NULL keys on both sides, type extremes, NaN / +-inf / subnormal
FP64 keys, a 70 000-row hot probe key and a 4 500-row build key in random order, row counts that are multiples of
nothing) as a root join with forced radix bits (two passes), XCD placement and the speculative path on for inputs
of any size.  One plan partitions two sides, so a row names up to two speculative scatters and the sample kernel.
Every row runs twice:

  taken     default margin (z = 6).  The result equals the oracle's, the named instantiations ran, k_pass_sample<KW>
            ran twice (once per side), and NO exact first-pass kernel ran: no k_pass_hist<SrcLoader...>, no
            k_pass_scatter<..SrcLoader..>, no k_pass_scatter_packed<SrcLoader..>.  That is the point of the row: a
            speculative kernel that is subtly wrong still gives the right result, through the fallback.  The rows'
            data is in random order, so the binomial bound of k_spec_caps holds with overwhelming probability;
            tests/test_spec_model.py confirms per row with the host model (tests/_specref.py) that no sub-range
            comes near its capacity
  overflow  RJ_TUNE_SPEC_Z=0: no margin at all, the model predicts an overflow on both sides of every row.  The
            speculative scatter ran and so did the exact histogram and the exact scatter of the same shape, once per
            side.  Only here do the spare-tile writes of the nine unbatched shapes and of the unblocked packed kernel
            run (the four NW == 4 kernels send a run to the spare tile in three arrays, one of them of pairs)

  poison    RJ_DEBUG_POISON=0x15A, taken, for an NW == 4 shape and the unblocked packed one: a second pass that read
            past a sub-range's end in any of its arrays would carry the fill pattern into the result

VARCHAR keys.  A join on a VARCHAR key IS eligible: hash_varchar_keys (rj_exec.hip) replaces each side's key by a
dense INT64 column of FNV-1a hashes and join_core then partitions both sides like any INT64 key, with the flag
words — radix_plan's `spec` condition (rj_radix_plan.cpp) asks nothing about the key's origin.  The keys are not `prehashed`
(fmix64 is applied on top); both sides carry their row index (one carry word), so the row reaches k_pass_sample<2>
and k_spec_scatter<3,SrcLoader<2,1,0>,-1> twice.  The model has no FNV-1a, so that row's no-fallback assertion rests
on the random order of its rows alone.  `s.prehashed` in k_pass_sample is only ever set by rj_join_tuples (the
sharded join's stage B hands in hashed tuples: JoinSpec::prehashed in Exec::run_tuples); that entry point reaches the
speculative path as a packed INT32 shape, k_spec_scatter_packed<SrcLoader<1,1,0>,true>, which the rows here and
test_gpu_spec_pass1.py cover with unhashed keys; no plan through rj_execute sets it.

test_every_speculative_instantiation_is_driven checks the rows' launch logs against the kernel handles compiled into
librj.so: 14 of 14, none unreachable."""
import dataclasses

import numpy as np
import pytest

import _elfsyms
import _oracle
import test_gpu_kernel_matrix as km
import test_gpu_spec_pass1 as sp1
import test_gpu_varchar_keys as vk
from pyrj import plan as pl
from test_gpu_kernel_matrix import C1, C2, C2W, C2WW, C3, C3S, C3SS, F64, I32, I64, NP0, Case

FAMILIES = ("k_pass_sample", "k_spec_scatter", "k_spec_scatter_packed")
KN = dict(RJ_TUNE_XCD_SPLIT="1", RJ_TUNE_XCD_MIN_ROWS="1", RJ_TUNE_SPEC_MIN_ROWS="1")
Z0 = dict(RJ_TUNE_SPEC_Z="0")
POISON = dict(RJ_DEBUG_POISON="0x15A")
SAMPLE1, SAMPLE2 = "k_pass_sample<1>", "k_pass_sample<2>"


def SS(nw, loader, pw):
    return f"k_spec_scatter<{nw},{loader},{pw}>"


def SSP(blocked):
    return f"k_spec_scatter_packed<SrcLoader<1,1,0>,{'true' if blocked else 'false'}>"


def exact_of(name):
    """The exact first-pass kernel of the same shape."""
    if name.startswith("k_spec_scatter_packed<"):
        return name.replace("k_spec_scatter_packed<", "k_pass_scatter_packed<")
    assert name.startswith("k_spec_scatter<"), name
    return name.replace("k_spec_scatter<", "k_pass_scatter<")[:-1] + ",false>"


def R(expect, kt, bp, pp, path=18, knobs=None, **kw):
    return Case(expect, kt, bp, pp, root=True, path=path, knobs=dict(KN, **(knobs or {})), **kw)


# expect: the speculative scatter(s), then the sample kernel
CASES = [
    R((SS(1, "SrcLoader<1,0,0>", -1), SS(2, "SrcLoader<1,1,0>", -1), SAMPLE1), I32, [], C1, path=16, knobs=NP0),
    R((SS(2, "SrcLoader<2,0,0>", -1), SS(3, "SrcLoader<2,1,0>", -1), SAMPLE2), F64, [], C1),
    R((SS(3, "SrcLoader<1,2,0>", 1), SS(3, "SrcLoader<1,2,1>", 1), SAMPLE1), I32, C2, C2W),
    R((SS(3, "SrcLoader<1,2,1>", 1), SAMPLE1), I32, C2WW, C2WW, build_left=False, seed=1),
    R((SS(4, "SrcLoader<1,3,1>", 2), SS(4, "SrcLoader<1,3,2>", 2), SAMPLE1), I32, C3S, C3),
    R((SS(4, "SrcLoader<1,3,2>", 2), SS(4, "SrcLoader<1,3,1>", 2), SAMPLE1), I32, C3, C3SS, path=16, build_left=False, seed=2),
    R((SS(4, "SrcLoader<2,2,0>", 2), SS(4, "SrcLoader<2,2,1>", 2), SAMPLE2), I64, C2, C2W, path=17),
    R((SS(4, "SrcLoader<2,2,1>", 2), SS(4, "SrcLoader<2,2,0>", 2), SAMPLE2), F64, C2WW, C2, seed=3),
    R((SSP(True), SAMPLE1), I32, C1, C1),
    R((SSP(False), SAMPLE1), I32, C1, C1, path=17, knobs=dict(RJ_TUNE_BLOCKED_MID="0")),
]
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)
VARCHAR_EXPECT = (SS(3, "SrcLoader<2,1,0>", -1), SAMPLE2)
POISONED = [c for c in CASES if c.id in (SS(4, "SrcLoader<1,3,1>", 2), SSP(False))]
assert len(POISONED) == 2


def named():
    """Every instantiation some row expects."""
    return {e for c in CASES for e in c.expect} | set(VARCHAR_EXPECT)


def compiled_in_scope():
    return sorted(n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(km.LIB)) if n.split("<")[0] in FAMILIES)


def with_knobs(c: Case, extra):
    return dataclasses.replace(c, knobs=dict(c.knobs, **extra))  # (same id and seed: the same data)


def exact_first_pass(ran):
    """The exact first-pass kernels in a launch log: the histogram over the source and the scatters out of it."""
    return sorted(k for k in ran if k.startswith("k_pass_hist<SrcLoader") or k.startswith("k_pass_scatter_packed<SrcLoader")
                  or (k.startswith("k_pass_scatter<") and "SrcLoader" in k))


def took_the_path(c_expect, ran):
    *scatters, sample = c_expect
    assert ran.get(sample) == 2, (sample, sorted(ran))  # once per side
    assert sum(ran.get(k, 0) for k in scatters) == 2 and all(k in ran for k in scatters), sorted(ran)
    assert not exact_first_pass(ran), exact_first_pass(ran)


def fell_back(c_expect, ran):
    *scatters, sample = c_expect
    hist = f"k_pass_hist<SrcLoader<{sample[-2]},0,0>>"
    missing = [k for k in [sample, hist] + scatters + [exact_of(k) for k in scatters] if k not in ran]
    assert not missing, f"expected {missing} to run; the launch log holds {sorted(ran)}"
    assert ran[sample] == 2 and ran[hist] == 2, ran  # the model: both sides overflow (tests/test_spec_model.py)
    assert sum(ran[k] for k in scatters) == sum(ran[exact_of(k)] for k in scatters) == 2, ran


_TAKEN = {}  # row id -> launch log of its taken run


def run_taken(c: Case):
    if c.id not in _TAKEN:
        _TAKEN[c.id] = km.check_case(c)  # the result equals the oracle's, the named instantiations ran
    return _TAKEN[c.id]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_taken(case):
    took_the_path(case.expect, run_taken(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forced_overflow(case):
    fell_back(case.expect, km.check_case(with_knobs(case, Z0)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", POISONED, ids=[c.id for c in POISONED])
def test_poison(case):
    took_the_path(case.expect, km.check_case(with_knobs(case, POISON)))


# ------------------------------------------------------------------ a VARCHAR key
_VARCHAR = {}


def varchar_keys(rng, n, vocab, empty):
    """n strings out of `vocab` in random order, 3 % NULL, the empty string in `empty` rows."""
    out = [b"w%d" % v for v in rng.integers(0, vocab, n)]
    for i in np.flatnonzero(rng.random(n) < 0.03):
        out[i] = None
    for i in rng.choice(n, empty, replace=False):
        out[i] = b""
    return out


def varchar_plan():
    """(plan, oracle result): VARCHAR keys with NULLs in random order; the empty string is a hot probe key (a fifth
    of the rows: about 3 200 per tile, three times the room a sub-range gets whose sample does not show them — a
    sample that hashed the key otherwise than the scatter would fall back)."""
    if not _VARCHAR:
        rng = np.random.default_rng(6161)
        nb, npr = 2 * km.PT_TILE + 1029, 5 * km.PT_TILE + 333
        bt = pl.make_table([(pl.VARCHAR, varchar_keys(rng, nb, 30_000, 3)), (I32, np.arange(nb, dtype=np.int32))])
        pt = pl.make_table([(pl.VARCHAR, varchar_keys(rng, npr, 33_000, 16_000)), (I64, rng.integers(-2**62, 2**62, npr))])
        p = vk.two(bt, pt, True, [(0, pl.VARCHAR), (1, I32)], [(0, pl.VARCHAR), (1, I64)], [(0, pl.VARCHAR), (1, I32), (3, I64)])
        _VARCHAR["p"] = (p, _oracle.execute(p))
    return _VARCHAR["p"]


def run_varchar():
    if "ran" not in _VARCHAR:
        p, want = varchar_plan()
        got, ran = sp1.run(p, KN)
        assert got.num_rows == want.num_rows and [c.type for c in got.columns] == [c.type for c in want.columns]
        assert pl.canonical_rows(got) == pl.canonical_rows(want)
        _VARCHAR["ran"] = ran
    return _VARCHAR["ran"]


@pytest.mark.gpu
def test_varchar_key_taken():
    took_the_path(VARCHAR_EXPECT, run_varchar())


@pytest.mark.gpu
def test_every_speculative_instantiation_is_driven():
    compiled = set(compiled_in_scope())
    reached = set(run_varchar())
    for c in CASES:
        reached |= set(run_taken(c))
    reached &= compiled
    print(f"reached {len(reached)} of {len(compiled)} compiled")
    assert not compiled - reached, sorted(compiled - reached)
    assert len(reached) == len(compiled) == 14
