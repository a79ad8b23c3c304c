"""CPU tier of the hash-adversarial tests: the numpy mixers restate the device's and the oracle's
hash, the key builder really produces keys with the asked-for hash bits, and the numpy reference
join (tests/_refjoin.py, used where the oracle is too slow) agrees with the oracle."""
import numpy as np
import pytest

import _oracle
import _refjoin
from pyrj import hashing as hs
from pyrj import plan as pl

I32MIN, I32MAX = -(2**31), 2**31 - 1
I64MIN, I64MAX = -(2**63), 2**63 - 1


def test_fmix64_equals_the_oracle_hash():
    rng = np.random.default_rng(1)
    vals = [0, -1, 1, I64MIN, I64MAX, I32MIN, I32MAX, I32MIN - 1, I32MAX + 1, 0x7FF8000000000000]
    vals += [int(x) for x in rng.integers(I64MIN, I64MAX, 500, dtype=np.int64)]
    vals += [int(x) for x in rng.integers(I32MIN, I32MAX, 500, dtype=np.int64)]
    L = _oracle.lib()
    want = np.array([L.rjo_hash_int(v) for v in vals], dtype=np.uint64)
    got = hs.fmix64(np.array(vals, dtype=np.int64).view(np.uint64))
    assert np.array_equal(got, want)
    # INT32 keys reach the oracle sign-extended: INT32_MIN/MAX and -1 as 64-bit values
    i32 = np.array([I32MIN, I32MAX, -1, 0], dtype=np.int32)
    assert np.array_equal(hs.fmix64(i32.astype(np.int64).view(np.uint64)),
                          np.array([L.rjo_hash_int(int(v)) for v in i32], dtype=np.uint64))


def test_unmixers_invert_the_mixers():
    rng = np.random.default_rng(2)
    h32 = np.concatenate([rng.integers(0, 2**32, 100_000, dtype=np.uint64).astype(np.uint32),
                          np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)])
    assert np.array_equal(hs.fmix32(hs.unfmix32(h32)), h32)
    assert np.array_equal(hs.unfmix32(hs.fmix32(h32)), h32)
    h64 = np.concatenate([rng.integers(0, 2**63, 100_000, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                          np.array([0, 1, 2**63, 2**64 - 1, 2**32 - 1, 2**32], dtype=np.uint64)])
    assert np.array_equal(hs.fmix64(hs.unfmix64(h64)), h64)
    assert np.array_equal(hs.unfmix64(hs.fmix64(h64)), h64)
    # fmix32 of 0 is 0 and fmix64 of 0 is 0: the keys whose hash is 0 are 0
    assert hs.fmix32(np.uint32(0)) == 0 and hs.fmix64(np.uint64(0)) == 0


@pytest.mark.parametrize("dtype,value,mask", [
    (np.int32, 0x1FFF, 0x1FFF),                 # one partition at <= 13 radix bits (the last one)
    (np.int32, 0, 0x1FFF),
    (np.int32, 0x7FF << 14 | 0x155, 0x1FFFFFF),  # partition + home bucket 2047 at 14 radix bits
    (np.int64, 0xDEADBEEF, 0xFFFFFFFF),         # the whole low word shared
    (np.float64, 0x7FF << 8 | 0x3C, 0x7FFFF),
    (np.float64, 0xFFFFFFFF, 0xFFFFFFFF),
])
def test_key_builder_carries_the_bits(dtype, value, mask):
    rng = np.random.default_rng(3)
    n = 128 if mask == 0x1FFFFFF else 20_000
    k = hs.keys_with_hash_bits(n, dtype, value, mask, rng=rng)
    assert k.dtype == np.dtype(dtype) and k.shape == (n,)
    wide = dtype != np.int32
    h = hs.key_hash(k, wide).astype(np.uint64)
    assert np.all(h & np.uint64(mask) == np.uint64(value & mask))
    assert np.unique(h).shape[0] == n  # distinct keys
    if dtype == np.float64:
        assert not hs.is_nan_bits(k.view(np.uint64)).any()
    if wide:  # the high hash words still differ: only they separate the keys
        assert np.unique(h >> np.uint64(32)).shape[0] > n * 0.99


def test_key_builder_owner_and_exhaustion():
    rng = np.random.default_rng(4)
    for n_ranks in (2, 4, 8):
        for owner in range(n_ranks):
            k = hs.keys_with_hash_bits(1000, np.int32, 0x5, 0xF, owner=owner, n_ranks=n_ranks, rng=rng)
            assert np.all(hs.owner_rank(k, n_ranks) == owner)
            assert np.all(hs.key_hash(k, False) & 0xF == 5)
    # 14 radix bits + 11 bucket bits fixed leave 7 bits: exactly 128 keys, then no more
    k = hs.keys_with_hash_bits(128, np.int32, 0x3FF, 0x1FFFFFF, rng=rng)
    assert np.unique(k).shape[0] == 128
    with pytest.raises(ValueError):
        hs.keys_with_hash_bits(129, np.int32, 0x3FF, 0x1FFFFFF, rng=rng)


# ------------------------------------------------------------------ _refjoin against the oracle

def _plan(bcols, pcols, build_left, outs=None):
    p = pl.Plan()
    bt, pt = pl.make_table(bcols), pl.make_table(pcols)
    if build_left:
        p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(bcols)])
        p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(pcols)])
        both = [c[0] for c in bcols] + [c[0] for c in pcols]
    else:
        p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(pcols)])
        p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(bcols)])
        both = [c[0] for c in pcols] + [c[0] for c in bcols]
    outs = outs if outs is not None else list(range(len(both)))
    p.new_join_node(build_left, 0, 1, 0, 0, [(i, both[i]) for i in outs])
    p.new_input(bt if build_left else pt)
    p.new_input(pt if build_left else bt)
    p.root = 2
    return p


def _same(p):
    want = _oracle.execute(p)
    got = _refjoin.execute(p)
    assert got.num_rows == want.num_rows
    assert [c.type for c in got.columns] == [c.type for c in want.columns]
    assert pl.table_digest(got) == pl.table_digest(want)
    if want.num_rows <= 2000:
        assert pl.canonical_rows(got) == pl.canonical_rows(want)
    return want.num_rows


def _fp64_specials():
    bits = [0x7FF0000000000001, 0x7FF4000000000000, 0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF,  # sNaN, qNaN
            0xFFF0000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF,                      # negative NaNs
            0x7FF0000000000000, 0xFFF0000000000000,                                          # +-inf
            0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x800000000000000F,                      # subnormals
            0x8000000000000000]                                                              # -0.0 only
    return np.array(bits, dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("seed", range(12))
def test_refjoin_equals_oracle_random(seed):
    rng = np.random.default_rng(100 + seed)
    kt = [pl.INT32, pl.INT64, pl.FP64][seed % 3]
    nb, npr = int(rng.integers(1, 3000)), int(rng.integers(1, 5000))
    dom = max(1, int(nb * rng.uniform(0.3, 2.0)))
    npt = {pl.INT32: np.int32, pl.INT64: np.int64, pl.FP64: np.float64}[kt]

    def keys(n):
        k = rng.integers(-dom // 2, dom - dom // 2, n)
        if kt == pl.FP64:
            k = k * 0.25
            sp = _fp64_specials()
            put = rng.random(n) < 0.05
            k[put] = sp[rng.integers(0, len(sp), int(put.sum()))]
        elif kt == pl.INT64:
            k = k * 3_000_000_019
        return k.astype(npt)

    bcols = [(kt, keys(nb), rng.random(nb) >= 0.1), (pl.INT64, rng.integers(-2**40, 2**40, nb)),
             (pl.FP64, rng.standard_normal(nb), rng.random(nb) >= 0.2)]
    pcols = [(kt, keys(npr), rng.random(npr) >= 0.1), (pl.INT32, rng.integers(-9, 9, npr).astype(np.int32))]
    outs = None if seed % 2 else [4, 0, 2, 3]
    assert _same(_plan(bcols, pcols, build_left=bool(seed % 4 < 2), outs=outs)) > 0


@pytest.mark.parametrize("kt", [pl.INT32, pl.INT64, pl.FP64])
def test_refjoin_equals_oracle_adversarial(kt):
    """Keys sharing their low hash bits (the 64-bit ones their whole low fmix64 word), duplicates
    on both sides, NULL keys, and for FP64 every NaN class (never matches), +-inf and subnormals
    (match themselves) and a -0.0-only key."""
    rng = np.random.default_rng(7 + kt)
    npt = {pl.INT32: np.int32, pl.INT64: np.int64, pl.FP64: np.float64}[kt]
    mask = 0xFFFFFFFF if kt != pl.INT32 else 0xFFF
    distinct = hs.keys_with_hash_bits(600, npt, 0x2A5, mask, rng=rng)
    if kt == pl.FP64:
        distinct = np.concatenate([distinct, _fp64_specials()])
    bk = np.concatenate([distinct[:400], distinct[:50], distinct[:5]])  # up to 3 copies
    pk = np.concatenate([rng.choice(distinct, 1500), distinct[:20]])
    bcols = [(kt, bk, rng.random(bk.shape[0]) >= 0.05), (pl.INT32, np.arange(bk.shape[0], dtype=np.int32))]
    pcols = [(kt, pk, rng.random(pk.shape[0]) >= 0.05), (pl.INT64, np.arange(pk.shape[0], dtype=np.int64))]
    for build_left in (True, False):
        assert _same(_plan(bcols, pcols, build_left)) > 0
    if kt == pl.FP64:  # NaN keys never match, even their own bit pattern
        sp = _fp64_specials()
        nan = sp[hs.is_nan_bits(sp.view(np.uint64))]
        p = _plan([(kt, nan), (pl.INT32, np.arange(len(nan), dtype=np.int32))], [(kt, nan), (pl.INT32, np.zeros(len(nan), np.int32))], True)
        assert _oracle.execute(p).num_rows == 0 == _refjoin.execute(p).num_rows
