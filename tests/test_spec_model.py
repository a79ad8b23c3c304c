"""The host model of the speculative first pass (tests/_specref.py) checked against itself and against the host's
own bound, and its predictions for every committed GPU case — no GPU.

The GPU tests (test_gpu_spec_matrix.py, test_gpu_spec_model.py, test_gpu_spec_pass1.py) assert that a side falls
back, or does not; this file makes sure each of those assertions rests on a definite prediction of the model and
says which one."""
import numpy as np
import pytest

import _specref
import test_gpu_kernel_matrix as km
import test_gpu_spec_matrix as sm
import test_gpu_spec_model as gm
import test_gpu_spec_pass1 as sp1
from pyrj import plan as pl

PT_TILE = _specref.PT_TILE


# ------------------------------------------------------------------ the model itself
def test_pass_bits():
    assert [_specref.pass_bits(b) for b in (18, 17, 16, 10)] == [[9, 9], [9, 8], [8, 8], [5, 5]]


def test_slice_places():
    for s in range(1, 6):
        width = PT_TILE >> s
        starts = [_specref.slice_of(t, s)[0] for t in range(33)]
        assert all(st % width == 0 and st + width <= PT_TILE for st in starts)
        assert len(set(starts[:1 << s])) == 1 << s  # every place comes up before one repeats
        assert starts[1 << s] == starts[0] == 0
    starts = [_specref.slice_of(t, 5)[0] for t in range(33)]
    assert len(set(starts[:32])) == 32 and starts[32] == starts[0]
    assert _specref.slice_of(1, 5) == (7 * 512, 512)
    # a partial last tile: clamped to its end while it holds more than a slice, read whole otherwise
    assert _specref.slice_of(20, 5, 4000) == (4000 - 512, 512)
    assert _specref.slice_of(20, 5, 6144 + 512) == (6144, 512) and _specref.slice_of(20, 5, 6144 + 511) == (6143, 512)
    assert _specref.slice_of(20, 5, 513) == (1, 512)
    assert _specref.slice_of(20, 5, 512) == (0, 512) and _specref.slice_of(20, 5, 77) == (0, 77)
    m = _specref.sampled(20 * PT_TILE + 1029, 5)
    assert m.sum() == 21 * 512 and m[20 * PT_TILE + 517:].all() and not m[20 * PT_TILE:20 * PT_TILE + 517].any()


def test_no_margin_is_the_scaled_sample_count():
    c = np.arange(0, 3000)
    for s in range(1, 6):
        want = ((c << s) + 31) // 32 * 32
        assert (_specref.capacity(c, s, 0) == want).all()
    assert (_specref.capacity(c, 5, 0) == 32 * c).all()


def test_capacity_formula():
    # c = 0, s = 5, z = 6: 32 (0 + 6 + 18) = 768; c = 3: 32 (3 + 12 + 18) = 1056; both multiples of 32 already
    assert list(_specref.capacity([0, 3], 5, 60)) == [768, 1056]
    # c = 8, s = 1, z = 6: 2 (8 + 18 + 18) = 88 -> 96
    assert list(_specref.capacity([8], 1, 60)) == [96]
    assert (np.diff(_specref.capacity(np.arange(5000), 5, 60)) >= 0).all() and (_specref.capacity(np.arange(5000), 3, 25) % 32 == 0).all()


def _keys(kind, n, rng):
    if kind == "one_key":
        return np.full(n, 123457, np.int32)
    return rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)


@pytest.mark.parametrize("kind", ["random", "one_key"])
@pytest.mark.parametrize("bits", [18, 16, 10])  # first pass of 9, 8 and 5 bits
def test_capacities_stay_below_the_hosts_bound(kind, bits):
    rng = np.random.default_rng(bits)
    bits0 = _specref.pass_bits(bits)[0]
    for n in (1029, 3 * PT_TILE + 1029, 20 * PT_TILE + 1029):
        keys = _keys(kind, n, rng)
        d, ok = _specref.digits(keys, None, pl.INT32, bits0)
        for s in range(1, 6):
            sub = (d << 3) | ((np.arange(n) // PT_TILE) & 7)
            sample = np.bincount(sub[_specref.sampled(n, s)], minlength=8 << bits0)
            assert sample.sum() <= -(-n // PT_TILE) * (PT_TILE >> s)
            for z in (0, 25, 60):
                total = int(_specref.capacity(sample, s, z).sum())
                assert total <= _specref.cap_max(n, bits0, s, z), (kind, bits, n, s, z)
                p = _specref.predict(keys, None, pl.INT32, bits, s, z)
                assert (p.cap == _specref.capacity(sample, s, z)).all()  # so nothing is ever cut at cap_max
                assert (p.sample == sample).all() and p.count.sum() == n


def test_flag_rule():
    """z > 0: a definite answer only away from the boundary; z = 0: exact."""
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 2**31 - 1, 20 * PT_TILE).astype(np.int32)
    p = _specref.predict(keys, None, pl.INT32, 18)
    assert p.overflows is False and (p.count <= p.cap - 32).all()
    p0 = _specref.predict(keys, None, pl.INT32, 18, z_tenths=0)
    assert p0.overflows is True and (p0.count > p0.cap).any()
    # NULL and NaN keys are no tuples
    f = np.array([np.nan, 1.5, -0.0, np.inf] * 100)
    v = np.ones(400, bool)
    v[1::4] = False
    q = _specref.predict(f, v, pl.FP64, 18)
    assert q.count.sum() == 200


# ------------------------------------------------------------------ the committed GPU cases
@pytest.mark.parametrize("name", list(gm.CASES))
def test_model_cases_get_a_definite_prediction(name):
    pred = gm.prediction(name)
    assert all(q.overflows is not None for q in pred), name
    c = gm.CASES[name]
    if c.z == 0:
        want = (True, True)
    elif c.data == "fixed_period" or c.data.startswith("phase_out"):
        want = (False, True)
    else:
        want = (False, False)
    assert tuple(q.overflows for q in pred) == want, (name, [q.fullest for q in pred])


def test_three_digits_leaves_nearly_every_sub_range_empty():
    _, probe = gm.prediction("three_digits")
    assert (probe.count > 0).sum() == 24 and (probe.cap[probe.count == 0] == 768).all()


@pytest.mark.parametrize("shape", sorted(sp1.SHAPES))
def test_spec_pass1_cases_get_a_definite_prediction(shape):
    """random: no side overflows (at the default margin; both do without one); hidden: the probe side alone;
    clustered: whatever the model says, but it says something."""
    kt = sp1.SHAPES[shape][0]
    for data, size, want in (("random", "3t", (False, False)), ("random", "20t", (False, False)),
                             ("hidden", "20t", (False, True)), ("clustered", "20t", None)):
        rng = np.random.default_rng(4421 + 97 * sorted(sp1.SHAPES).index(shape) + 7 * len(data) + len(size))  # sp1.case's
        if data == "random":
            bk, bv, pk, pv = sp1.random_sides(kt, size, rng)
        else:
            bk, bv, pk, pv = {"clustered": sp1.clustered_sides, "hidden": sp1.hidden_sides}[data](kt, rng)
        got = tuple(_specref.predict(k, v, kt, sp1.RADIX_BITS).overflows for k, v in ((bk, bv), (pk, pv)))
        assert None not in got, (shape, data, got)
        if want:
            assert got == want, (shape, data, got)
        if data == "random":
            z0 = tuple(_specref.predict(k, v, kt, sp1.RADIX_BITS, z_tenths=0).overflows for k, v in ((bk, bv), (pk, pv)))
            assert z0 == (True, True)


@pytest.mark.parametrize("case", sm.CASES, ids=sm.IDS)
def test_matrix_rows_get_a_definite_prediction(case):
    """taken: no side comes near its capacity; z = 0: both sides overflow; the poisoned rows are taken rows."""
    assert case.root and isinstance(case.path, int) and len(_specref.pass_bits(case.path)) == 2
    p = km.make_case(case)
    assert [q.overflows for q in _specref.predict_plan(p, case.path)] == [False, False]
    assert [q.overflows for q in _specref.predict_plan(p, case.path, z_tenths=0)] == [True, True]
    keys = _specref.plan_sides(p)
    if case.kt == pl.FP64:
        assert all(np.isnan(k[v]).any() for k, v, _ in keys)  # k_pass_sample<2> sees NaN keys that are not NULL
    assert all((~v).any() for _, v, _ in keys)
