"""The speculative first pass against its host model (tests/_specref.py): a side falls back to the exact histogram
path exactly when the model says one of its sub-ranges is too small.

A speculative pass that goes wrong still gives the right answer — a sample that hashes differently from the
scatter, drops other rows or reads the wrong slice of a tile only makes sub-ranges too small, and the exact path
repairs that at two and a half times the cost.  So every case here asserts, next to the result, HOW OFTEN the exact
source histogram ran: once per side the model predicts to overflow, read from the launch log.  Each case is an
INT32 or INT64 inner join through capi.execute on a fresh context, XCD placement and the speculative path forced
on for inputs of any size, at about 20 tiles per side (the `20t` sizes and the data of test_gpu_spec_pass1.py), so
that the slice rotation takes twenty distinct values.

  phase_in / phase_out    a hot key owns 2500 rows of the probe side in every whole tile, placed with the model's own
                          slice function: around that tile's sample slice (the slice sees 512 of them: room for
                          everything) or wholly outside it (the slice sees none: overflow).  A kernel whose rotation
                          differs from the model's gets at least one of the two wrong.  *_tail: the hot rows lie in the
                          partial last tile only (4000 rows: more than a slice, so the slice's place is clamped to the
                          tile's end)
  fixed_period            the hot key in rows [0, 512) of every tile, what the rotation exists for: only tile 0 (and
                          with 25 tiles nothing else) samples it, sub-ranges 1 .. 7 of its digit overflow
  s1 / s3 / s5            RJ_TUNE_SPEC_SAMPLE on random keys (no overflow) and on phase_out data placed for that
                          slice width
  b16 / b17 / b10         forced radix bits 16 (8 + 8: 2048 sub-ranges, k_spec_caps' threads take two each, F = 256 in
                          k_spec_close), 17 (9 + 8) and, with RJ_TUNE_FINE=0, 10 (5 + 5: 256 sub-ranges, fewer than
                          k_spec_caps has threads, F = 32); each taken and with z = 0.  All three leave `spec` true in
                          radix_plan (rj_radix_plan.cpp): two passes, no fine histogram (16 and 17 are above its 15 bits, RJ_TUNE_FINE=0
                          takes it from the 10-bit plan), nothing else of the condition depends on the bits
  tpg3                    RJ_TUNE_TPG1=3: groups of three tiles, sub-range x = (tile // 3) & 7
  i64                     INT64 keys, random, phase_in and phase_out: with the INT64 / FP64 rows of
                          test_gpu_spec_matrix.py the only cases that tell a k_pass_sample<2> that hashes differently
                          from SrcLoader<2,...>.  (phase_in is the one that tells: a sample that puts the hot key's 512
                          rows into another bin leaves its sub-range too small.  Uniform keys fit under any hash, and
                          phase_out overflows under any.)
  three_digits            the probe side's keys all hash to 3 of the 512 first-pass digits: 4072 of the 4096
                          sub-ranges get the minimum capacity and hold nothing, the second pass reads thousands of
                          empty input segments with gaps between them

Plans, reference results and predictions are made once per module and left unchanged.  tests/test_spec_model.py
checks without a GPU that every case gets a definite prediction, and which."""
from dataclasses import dataclass

import numpy as np
import pytest

import _oracle
import _specref
import test_gpu_scatter_rank as sr
import test_gpu_spec_pass1 as sp1
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

PT_TILE = sr.PT_TILE
I32, I64 = pl.INT32, pl.INT64
HOT = 2500
EXACT_HIST = {I32: "k_pass_hist<SrcLoader<1,0,0>>", I64: "k_pass_hist<SrcLoader<2,0,0>>"}
SAMPLE = {I32: "k_pass_sample<1>", I64: "k_pass_sample<2>"}
SPEC_SCATTER = {(I32, I64): "k_spec_scatter<3,SrcLoader<1,2,0>,1>",
                (I32, I32): "k_spec_scatter_packed<SrcLoader<1,1,0>,true>",
                (I64, I64): "k_spec_scatter<4,SrcLoader<2,2,0>,2>"}


@dataclass(frozen=True)
class Spec:
    data: str
    kt: int = I32
    ct: int = I64
    bits: int = 18
    s: int = 5          # RJ_TUNE_SPEC_SAMPLE
    z: int = 60         # RJ_TUNE_SPEC_Z
    tpg: int = 0        # RJ_TUNE_TPG1
    fine: bool = True   # RJ_TUNE_FINE

    @property
    def env(self):
        e = dict(sp1.TAKEN, RJ_TUNE_SPEC_SAMPLE=str(self.s), RJ_TUNE_SPEC_Z=str(self.z))
        if self.tpg:
            e["RJ_TUNE_TPG1"] = str(self.tpg)
        if not self.fine:
            e["RJ_TUNE_FINE"] = "0"
        return e


CASES = {
    "phase_in": Spec("phase_in"),
    "phase_out": Spec("phase_out"),
    "phase_in_tail": Spec("phase_in_tail", ct=I32),
    "phase_out_tail": Spec("phase_out_tail", ct=I32),
    "fixed_period": Spec("fixed_period"),
    "random_s1": Spec("random", ct=I32, s=1),
    "random_s3": Spec("random", s=3),
    "random_s5": Spec("random", ct=I32),
    "phase_out_s1": Spec("phase_out", s=1),
    "phase_out_s3": Spec("phase_out", ct=I32, s=3),
    "b16": Spec("random", bits=16),
    "b16_z0": Spec("random", bits=16, z=0),
    "b17": Spec("random", ct=I32, bits=17),
    "b17_z0": Spec("random", ct=I32, bits=17, z=0),
    "b10": Spec("random", bits=10, fine=False),
    "b10_z0": Spec("random", bits=10, fine=False, z=0),
    "tpg3_random": Spec("random", tpg=3),
    "tpg3_phase_out": Spec("phase_out", ct=I32, tpg=3),
    "i64_random": Spec("random", kt=I64),
    "i64_phase_in": Spec("phase_in", kt=I64),
    "i64_phase_out": Spec("phase_out", kt=I64),
    "three_digits": Spec("three_digits"),
}


# ------------------------------------------------------------------ data
def hot_block(tile, rows, s, inside):
    """Where HOT consecutive rows go in a tile of `rows` rows: around the tile's sample slice (the slice and the rows
    behind it, moved down where the tile ends first), or wholly outside it (behind it, or in front where there is no
    room behind).  None: the tile has no room for them."""
    at, cnt = _specref.slice_of(tile, s, rows)
    if inside:
        lo = min(at, rows - max(HOT, cnt))
        return (lo, lo + max(HOT, cnt)) if lo >= 0 else None
    if at + cnt + HOT <= rows:
        return at + cnt, at + cnt + HOT
    return (at - HOT, at) if at >= HOT else None


def grown(rng, pk, pv, n):
    """The probe side with n rows: more rows drawn from its own."""
    more = rng.integers(0, pk.shape[0], n - pk.shape[0])
    return np.concatenate([pk, pk[more]]), np.concatenate([pv, pv[more]])


def make_sides(c: Spec, rng):
    """-> build keys, build validity, probe keys, probe validity"""
    bk, bv, pk, pv = sp1.random_sides(c.kt, "20t", rng)
    hot = bk[5]
    bv[5] = True

    def own(lo, hi):
        pk[lo:hi] = hot
        pv[lo:hi] = True

    if c.data in ("phase_in", "phase_out"):
        placed = 0
        for t in range(-(-pk.shape[0] // PT_TILE)):
            blk = hot_block(t, min(PT_TILE, pk.shape[0] - t * PT_TILE), c.s, c.data == "phase_in")
            if blk:
                own(t * PT_TILE + blk[0], t * PT_TILE + blk[1])
                placed += 1
        assert placed == 20  # every whole tile
    elif c.data in ("phase_in_tail", "phase_out_tail"):
        pk, pv = grown(rng, pk, pv, 20 * PT_TILE + 4000)
        at, cnt = _specref.slice_of(20, c.s, 4000)
        assert (at, cnt) == (4000 - 512, 512)  # clamped: the unclamped place is 7 * 20 * 512 % 16384 = 6144
        lo, hi = hot_block(20, 4000, c.s, c.data == "phase_in_tail")
        own(20 * PT_TILE + lo, 20 * PT_TILE + hi)
    elif c.data == "fixed_period":
        pk, pv = grown(rng, pk, pv, 24 * PT_TILE + 1029)
        for t in range(25):
            own(t * PT_TILE, t * PT_TILE + 512)
    elif c.data == "three_digits":
        cand = np.arange(400_000)
        dg = sr.low_digit(c.kt, sr.keys_of(c.kt, cand))
        pool = sr.keys_of(c.kt, cand[np.isin(dg, (0, 257, 511))])
        assert pool.shape[0] > 2000
        pk = pool[rng.integers(0, pool.shape[0], pk.shape[0])]
    else:
        assert c.data == "random", c.data
    return bk, bv, pk, pv


_SIDES, _PLANS, _PRED = {}, {}, {}


def _data_key(c: Spec):
    return (c.data, c.kt, c.s if c.data.startswith("phase") else 0)


def sides(c: Spec):
    k = _data_key(c)
    if k not in _SIDES:
        rng = np.random.default_rng(7103 + 13 * sorted({s.data for s in CASES.values()}).index(c.data) + c.kt + c.s)
        _SIDES[k] = make_sides(c, rng)
    return _SIDES[k]


def prediction(name):
    """-> (build side's, probe side's) _specref.Prediction"""
    if name not in _PRED:
        c = CASES[name]
        bk, bv, pk, pv = sides(c)
        _PRED[name] = tuple(_specref.predict(k, v, c.kt, c.bits, c.s, c.z, c.tpg) for k, v in ((bk, bv), (pk, pv)))
    return _PRED[name]


def plan_of(c: Spec):
    """(plan, reference result, expected row count), once per data set and payload type."""
    k = _data_key(c) + (c.ct,)
    if k not in _PLANS:
        bk, bv, pk, pv = sides(c)
        p = sp1.join_plan(c.kt, c.ct, bk, bv, pk, pv, np.random.default_rng(len(_PLANS)))
        _PLANS[k] = (p, _oracle.execute(p), sr.expected_rows(bk, bv, pk, pv))
    return _PLANS[k]


@pytest.mark.parametrize("name", list(CASES))
def test_falls_back_exactly_when_the_model_says(name):
    c = CASES[name]
    pred = prediction(name)
    assert all(q.overflows is not None for q in pred), "the model gives no definite prediction: pick other data"
    want_exact = sum(bool(q.overflows) for q in pred)
    p, want, rows = plan_of(c)
    ctx = sp1.context(c.env, c.bits)
    try:
        got, ran = sp1.run(p, None, ctx)
    finally:
        ctx.destroy()
    spec = SPEC_SCATTER[c.kt, c.ct]
    print(f"{name}: predicted overflow (build, probe) = {[q.overflows for q in pred]}, fullest sub-range "
          f"{[round(q.fullest, 3) for q in pred]} of its capacity; exact histograms {ran.get(EXACT_HIST[c.kt], 0)}")
    assert ran.get(SAMPLE[c.kt]) == 2 and ran.get(spec) == 2, sorted(ran)  # once per side
    assert ran.get(EXACT_HIST[c.kt], 0) == want_exact, (name, want_exact, ran)
    sp1.same_join(got, want, rows)
