"""Hash-adversarial joins: keys chosen against the device hash, not drawn from a random domain.

The kernels lay out their work by the HASHED key (csrc/rj_partition.hip, rj_join.hip, rj_bcast.hip): the low radix_bits bits pick
the partition, the next 11 bits the home bucket of the LDS table (a full bucket spills into the next,
bucket 2047 wraps to 0), the broadcast table takes its home bucket from the lowest 11 bits, the
tagged table stores h >> radix_bits as tag, a 64-bit key's high hash word separates keys whose low
words match, and the top bits pick the owner rank of a sharded join.  Random keys spread evenly
over all of these; here every construction is computed through the inverse mixers
(pyrj/hashing.keys_with_hash_bits), so the tests reach on purpose:
  a. one partition (or one pass-1 / pass-2 digit) holding every tuple: chunked build, heavy tasks;
  b. bucket chains of ~750 buckets wrapping 2047 -> 0 in the generic table, 64-bit keys that only
     the high-word compare separates;
  c. the tagged table: chains of 128 keys with duplicates (the re-walk crosses the wrap), the
     largest tag and tag 0;
  d. the broadcast table with 4096 / 4095 build keys in one home bucket;
  e. the heavy-task table near its bound (partitions of JN_HEAVY, JN_HEAVY+1, 2*JN_HEAVY+1);
  f. key and hash extremes (hash 0, all-ones, the EMPTY word of a neighbouring partition, NaN,
     +-inf, subnormals) through the broadcast join, one pass and two passes;
  g. a sharded join in which one rank owns every key.
Each case asserts its construction on the host (and for INT32 keys on the device, through the
hashed keys stage A returns) and a non-empty result equal to the oracle's — or, where the oracle's
hash table turns quadratic on 64-bit keys sharing low fmix64 bits, to tests/_refjoin.py.

Measured on an MI355X: 78 tests in 18 s, 12 s of which is the first test's device start-up; every
chain case takes under 0.3 s."""
import os

import numpy as np
import pytest

import _oracle
import _refjoin
from pyrj import capi
from pyrj import dist
from pyrj import hashing as hs
from pyrj import plan as pl
from test_gpu_midscale import _KNOBS
from test_gpu_sharded import combine, run_sharded

pytestmark = pytest.mark.gpu

JN_RMAX, JN_HEAVY = 4096, 65536
NP_OF = {pl.INT32: np.int32, pl.INT64: np.int64, pl.FP64: np.float64}


def make_ctx(env=None, **kw):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # read once, when the context is created
    try:
        return capi.Context(**kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx0():
    c = capi.Context()
    yield c
    capi.destroy_context(c)


@pytest.fixture(scope="module", params=list(_KNOBS) + ["bits=11", "bits=16", "bits=20"])
def a_ctx(request):
    """The midscale knob matrix (default / xcd / side / mid3 / chunks / pairs) and forced radix bits."""
    if request.param in _KNOBS:
        env, kw = _KNOBS[request.param]
        c = make_ctx(env, **kw)
    else:
        c = make_ctx(radix_bits=int(request.param.split("=")[1]))
    c.knob = request.param
    yield c
    capi.destroy_context(c)


def join_plan(bcols, pcols, build_left=True, outs=None):
    """Scan(build) JOIN Scan(probe) on column 0; outs index left outputs ++ right outputs."""
    p = pl.Plan()
    lcols, rcols = (bcols, pcols) if build_left else (pcols, bcols)
    p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
    p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])
    both = [c[0] for c in lcols] + [c[0] for c in rcols]
    outs = outs if outs is not None else range(len(both))
    p.new_join_node(build_left, 0, 1, 0, 0, [(i, both[i]) for i in outs])
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(rcols))
    p.root = 2
    return p


def expect(p, ref="oracle"):
    want = (_oracle if ref == "oracle" else _refjoin).execute(p)
    assert want.num_rows > 0
    return want.num_rows, pl.table_digest(want)


def check(p, ctx, want):
    got = capi.execute(p, ctx)
    assert got.num_rows == want[0]
    assert pl.table_digest(got) == want[1]


def device_hashes_match(ctx, keys, valid=None):
    """Stage A (one rank) returns the device's hashed INT32 keys: they must be fmix32 of the keys."""
    import torch

    keys = np.asarray(keys, dtype=np.int32)
    valid = np.ones(keys.shape[0], bool) if valid is None else valid
    t = ctx.upload(pl.make_table([(pl.INT32, keys, valid), (pl.INT32, np.arange(keys.shape[0], dtype=np.int32))]))
    try:
        hk, carry, counts = dist.GpuOps(ctx).partition(t, keys.shape[0], 1)
        torch.cuda.synchronize()
        got = np.sort(hk.cpu().numpy().view(np.uint32))
    finally:
        t.release()
    assert counts == [int(valid.sum())]
    assert np.array_equal(got, np.sort(hs.fmix32(keys[valid].view(np.uint32))))


def assert_bits(keys, wide, value, mask):
    h = hs.key_hash(keys, wide).astype(np.uint64)
    assert np.all(h & np.uint64(mask) == np.uint64(value & mask))


def hits_and_misses(rng, distinct, n_build, n_probe, miss_frac):
    """build = distinct[:n_build]; probe = hits drawn from the build keys + misses drawn from the
    rest of `distinct` (which share the same hash bits)."""
    bk = distinct[:n_build]
    nm = int(n_probe * miss_frac)
    pk = np.concatenate([rng.choice(bk, n_probe - nm), rng.choice(distinct[n_build:], nm)])
    return bk, pk[rng.permutation(pk.shape[0])]


# ----------------------------------------------------------------- a. one partition holds everything
# value/mask over the low hash bits every key shares; at the default 7-9 radix bits "first"/"last"
# put every tuple into partition 0 / the last partition, "p1" fixes the low 8 bits (the pass-1 digit
# of the 16-bit plans) with the pass-2 digit spread, "p2" the reverse
_A_VARIANTS = {"first": (0, 0x1FFF), "last": (0x1FFF, 0x1FFF), "p1": (0xA5, 0xFF), "p2": (0x5A00, 0xFF00)}
_A_DATA = {}


def a_data(variant):
    if variant not in _A_DATA:
        value, mask = _A_VARIANTS[variant]
        rng = np.random.default_rng(11 + list(_A_VARIANTS).index(variant))
        nb, npr = 400_000, 800_000
        distinct = hs.keys_with_hash_bits(nb + 120_000, np.int32, value, mask, rng=rng)
        bk, pk = hits_and_misses(rng, distinct, nb, npr, 0.3)
        pvalid = rng.random(npr) >= 0.01
        assert_bits(bk, False, value, mask)
        assert_bits(pk, False, value, mask)
        p = join_plan([(pl.INT32, bk), (pl.INT32, np.arange(nb, dtype=np.int32))],
                      [(pl.INT32, pk, pvalid), (pl.INT32, rng.integers(-9, 9, npr).astype(np.int32))],
                      outs=[0, 1, 3])
        _A_DATA[variant] = (p, expect(p), bk, pk, pvalid)
    return _A_DATA[variant]


@pytest.mark.parametrize("variant", list(_A_VARIANTS))
def test_a_one_partition_holds_everything(a_ctx, variant):
    p, want, bk, pk, pvalid = a_data(variant)
    ctx = a_ctx
    if ctx.knob == "default":
        device_hashes_match(ctx, bk)
        device_hashes_match(ctx, pk, pvalid)
    check(p, ctx, want)


def test_a_int64_one_partition(ctx0):
    rng = np.random.default_rng(31)
    nb, npr = 300_000, 600_000
    distinct = hs.keys_with_hash_bits(nb + 100_000, np.int64, 0x0ABC, 0x1FFF, rng=rng)
    bk, pk = hits_and_misses(rng, distinct, nb, npr, 0.3)
    assert_bits(bk, True, 0x0ABC, 0x1FFF)
    p = join_plan([(pl.INT64, bk), (pl.INT64, rng.integers(-2**40, 2**40, nb))],
                  [(pl.INT64, pk, rng.random(npr) >= 0.02), (pl.INT32, np.arange(npr, dtype=np.int32))])
    check(p, ctx0, expect(p, ref="refjoin"))


# ------------------------------------------------------------------------------ b. bucket chains
B_BITS = 8  # forced: k_join (not the broadcast join); 8 + 11 fixed bits leave 13 free for 3000 keys
B_PART = 0x3C


def chain_keys(rng, dtype, n, bits, part):
    """n distinct keys of partition `part` with home bucket 2047 (the chain wraps to bucket 0).
    64-bit keys share the WHOLE low hash word: only the high word separates them."""
    if dtype == np.int32:
        value, mask = part | (2047 << bits), (1 << (bits + 11)) - 1
    else:
        value, mask = part | (2047 << bits) | (0x1234 << (bits + 11)), 0xFFFFFFFF
    k = hs.keys_with_hash_bits(n, dtype, value, mask, rng=rng)
    assert_bits(k, dtype != np.int32, value, mask)
    return k


def background(rng, dtype, n):
    if dtype == np.int32:
        return rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    if dtype == np.int64:
        return rng.integers(-2**62, 2**62, n)
    return rng.standard_normal(n) * 1e6


def payload(rng, dt, n):
    return (dt, background(rng, NP_OF[dt], n))


# build carries: one word (INT32), two words (INT64), wide (INT32 + INT64 columns)
_B_CARRIES = {"cw1": [pl.INT32], "cw2": [pl.INT64], "wide": [pl.INT32, pl.INT64]}


@pytest.fixture(scope="module")
def ctx_b():
    c = make_ctx(radix_bits=B_BITS)
    yield c
    capi.destroy_context(c)


def chain_join(rng, kt, bpay, build_left, bits, part, n_chain=3000):
    dtype = NP_OF[kt]
    chain = chain_keys(rng, dtype, n_chain + 1000, bits, part)
    bg = background(rng, dtype, 200_000)
    bk = np.concatenate([bg, chain[:n_chain]])
    # probe: background, every chain key twice, chain keys that miss (they walk the whole chain)
    pk = np.concatenate([rng.choice(bg, 300_000), chain[:n_chain], chain[:n_chain], chain[n_chain:]])
    pk = pk[rng.permutation(pk.shape[0])]
    bcols = [(kt, bk)] + [payload(rng, t, bk.shape[0]) for t in bpay]
    pcols = [(kt, pk), (pl.INT32, np.arange(pk.shape[0], dtype=np.int32))]
    return join_plan(bcols, pcols, build_left), chain


@pytest.mark.parametrize("build_left", [True, False])
@pytest.mark.parametrize("carry", list(_B_CARRIES))
def test_b_int32_bucket_chain(ctx_b, carry, build_left):
    rng = np.random.default_rng(41 + len(carry) + build_left)
    p, chain = chain_join(rng, pl.INT32, _B_CARRIES[carry], build_left, B_BITS, B_PART)
    device_hashes_match(ctx_b, chain)
    check(p, ctx_b, expect(p))


@pytest.mark.parametrize("build_left", [True, False])
@pytest.mark.parametrize("kt", [pl.INT64, pl.FP64])
def test_b_64_bit_keys_sharing_the_low_word(ctx_b, kt, build_left):
    rng = np.random.default_rng(51 + kt + build_left)
    p, chain = chain_join(rng, kt, [pl.INT32], build_left, B_BITS, B_PART)
    # the chain keys' hashes differ in the high word only
    h = hs.key_hash(chain, True)
    assert np.unique(h & np.uint64(0xFFFFFFFF)).shape[0] == 1 and np.unique(h).shape[0] == chain.shape[0]
    check(p, ctx_b, expect(p))


# ------------------------------------------------------------------------------ c. tagged table
@pytest.mark.parametrize("build_left", [True, False])
@pytest.mark.parametrize("bits", [14, 16])
def test_c_tagged_table_chains(bits, build_left):
    """INT32 key + INT64 build payload at >= 14 radix bits: the tagged table.  The last partition's
    home bucket 2047 holds every key its 32 - bits - 11 free bits allow (128 at 14 bits), each 1-30
    times, so the duplicate re-walk runs across the wrap; the largest tag (hash 0xFFFFFFFF) is one
    of them, and tag 0 of the same partition (hash = its radix bits) has home bucket 0, where the
    wrapped chain already sits."""
    rng = np.random.default_rng(61 + bits + build_left)
    top = (1 << bits) - 1
    chain = hs.keys_with_hash_bits(1 << (32 - bits - 11), np.int32, (1 << (bits + 11)) - 1, (1 << (bits + 11)) - 1, rng=rng)
    hmax, htag0 = np.uint32(0xFFFFFFFF), np.uint32(top)
    tag_max_key, tag0_key = hs.unfmix32(hmax).view(np.int32), hs.unfmix32(htag0).view(np.int32)
    assert tag_max_key in chain
    assert int(hs.fmix32(tag_max_key.view(np.uint32))) >> bits == (1 << (32 - bits)) - 1
    tag0_other = hs.unfmix32(np.uint32(0x155)).view(np.int32)  # tag 0 of partition 0x155
    copies = rng.integers(1, 31, chain.shape[0])
    copies[chain == tag_max_key] = 30
    bg = background(rng, np.int32, 300_000)
    special = np.array([tag0_key, tag0_key, tag0_other], dtype=np.int32)
    bk = np.concatenate([bg, np.repeat(chain, copies), special])
    pk = np.concatenate([rng.choice(bg, 400_000), chain, chain[: chain.shape[0] // 2], special,
                         np.full(5, tag_max_key, np.int32)])
    pk = pk[rng.permutation(pk.shape[0])]
    c = make_ctx(radix_bits=bits)
    try:
        device_hashes_match(c, np.concatenate([chain, special]))
        p = join_plan([(pl.INT32, bk), (pl.INT64, background(rng, np.int64, bk.shape[0]))],
                      [(pl.INT32, pk), (pl.INT32, np.arange(pk.shape[0], dtype=np.int32))], build_left)
        check(p, c, expect(p))
    finally:
        capi.destroy_context(c)


# -------------------------------------------------------------------------- d. broadcast table
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("nb", [4096, 4095])
@pytest.mark.parametrize("kt", [pl.INT32, pl.INT64])
def test_d_broadcast_one_home_bucket(ctx0, kt, nb, nulls):
    """Build sides of 4096 / 4095 rows (k_join_bcast) whose keys all have low hash bits 2047: one
    chain of ~1024 buckets from bucket 2047 around to ~1023.  64-bit keys share the whole low word."""
    rng = np.random.default_rng(71 + kt + nb + nulls)
    dtype = NP_OF[kt]
    value, mask = (0x7FF, 0x7FF) if kt == pl.INT32 else (0x9ABCD7FF, 0xFFFFFFFF)
    distinct = hs.keys_with_hash_bits(nb + 2000, dtype, value, mask, rng=rng)
    assert_bits(distinct, kt != pl.INT32, value, mask)
    bk, pk = hits_and_misses(rng, distinct, nb, 1_000_000, 0.3)
    bvalid = rng.random(nb) >= 0.1 if nulls else np.ones(nb, bool)
    pvalid = rng.random(pk.shape[0]) >= 0.05 if nulls else np.ones(pk.shape[0], bool)
    if kt == pl.INT32:
        device_hashes_match(ctx0, bk, bvalid)
    p = join_plan([(kt, bk, bvalid), (pl.INT64, background(rng, np.int64, nb))],
                  [(kt, pk, pvalid), (pl.INT32, np.arange(pk.shape[0], dtype=np.int32))], build_left=False, outs=[0, 1, 3])
    # 64-bit keys sharing the low fmix64 word are the oracle's quadratic case (~5 s each here)
    check(p, ctx0, expect(p, ref="oracle" if kt == pl.INT32 else "refjoin"))


# ------------------------------------------------------------------------ e. heavy-task table bound
@pytest.mark.parametrize("big_build", [False, True])
def test_e_heavy_task_bound(big_build):
    """Forced 8 bits: 16 probe partitions of exactly JN_HEAVY+1 tuples (two tasks each), 4 of exactly
    JN_HEAVY (not heavy), 4 of 2*JN_HEAVY+1 (three tasks) and nothing else on the probe side: 44 tasks
    against max_tasks = 2*(|S|/JN_HEAVY)+2 = 58.  Distinct probe keys; build partitions of 1000 keys,
    or of 5000 (above JN_RMAX: every task re-walks two build chunks)."""
    rng = np.random.default_rng(81 + big_build)
    sizes = [JN_HEAVY + 1] * 16 + [JN_HEAVY] * 4 + [2 * JN_HEAVY + 1] * 4
    parts = rng.permutation(256)[: len(sizes)]
    nbp = 5000 if big_build else 1000
    bks, pks = [], []
    for q, s in zip(parts, sizes):
        k = hs.keys_with_hash_bits(s + nbp, np.int32, int(q), 0xFF, rng=rng)
        bks.append(k[:nbp])
        # distinct probe keys: the first half of the build keys hit, the rest miss
        pks.append(np.concatenate([k[: nbp // 2], k[nbp : nbp + s - nbp // 2]]))
    bk, pk = np.concatenate(bks), np.concatenate(pks)
    pk = pk[rng.permutation(pk.shape[0])]
    ph = hs.key_hash(pk, False) & 0xFF
    assert sorted(np.bincount(ph, minlength=256)[parts].tolist()) == sorted(sizes)
    assert np.unique(pk).shape[0] == pk.shape[0]
    c = make_ctx(radix_bits=8)
    try:
        device_hashes_match(c, pk)
        p = join_plan([(pl.INT32, bk), (pl.INT32, np.arange(bk.shape[0], dtype=np.int32))],
                      [(pl.INT32, pk), (pl.INT64, background(rng, np.int64, pk.shape[0]))], outs=[0, 1, 3])
        want = expect(p)
        assert want[0] == len(sizes) * (nbp // 2)
        check(p, c, want)
    finally:
        capi.destroy_context(c)


# ------------------------------------------------------------------------- f. key and hash extremes
def extreme_keys(kt):
    if kt == pl.INT32:
        hashes = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE, 0xFF, 0xFE, 0xFFFF, 0xFFFE] + list(range(2, 16))
        k = hs.unfmix32(np.array(hashes, dtype=np.uint32)).view(np.int32)
        return np.unique(np.concatenate([k, np.array([-(2**31), 2**31 - 1, 0, -1, 1], dtype=np.int32)]))
    low = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE, 0xFF, 0xFE, 0xFFFF, 0xFFFE] + list(range(2, 16))
    hashes = [lo | (hi << 32) for lo in low for hi in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)]
    bits = hs.unfmix64(np.array(hashes, dtype=np.uint64))
    if kt == pl.FP64:
        bits = bits[~hs.is_nan_bits(bits)]
        special = np.array([0x7FF0000000000000, 0xFFF0000000000000,          # +-inf
                            0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x800000000000000F,  # subnormals
                            0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x3FF0000000000000,  # +-DBL_MAX, 1.0
                            0x8000000000000000], dtype=np.uint64)               # -0.0 (no +0.0 anywhere)
        bits = bits[bits != 0]  # keep +0.0 out: only -0.0 appears
        return np.unique(np.concatenate([bits, special])).view(np.float64)
    ext = np.array([-(2**63), 2**63 - 1, 0, -1, -(2**31), 2**31 - 1], dtype=np.int64)
    return np.unique(np.concatenate([bits.view(np.int64), ext]))


_NANS = np.array([0x7FF0000000000001, 0x7FF4000000000000, 0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF,
                  0xFFF0000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("path", ["bcast", "bits=8", "bits=16"])
@pytest.mark.parametrize("kt", [pl.INT32, pl.INT64, pl.FP64])
def test_f_key_and_hash_extremes(kt, path):
    rng = np.random.default_rng(91 + kt)
    ext = extreme_keys(kt)
    bg = background(rng, NP_OF[kt], 3000)
    if kt == pl.FP64:
        bg = bg[bg != 0]
        ext_b = np.concatenate([ext, ext, _NANS])
        ext_p = np.concatenate([ext, _NANS, _NANS])
    else:
        ext_b, ext_p = np.concatenate([ext, ext]), ext
    bk = np.concatenate([bg, ext_b])  # <= 4096 rows: the broadcast join unless bits are forced
    pk = np.concatenate([rng.choice(bg, 200_000), np.repeat(ext_p, 50)])
    pk = pk[rng.permutation(pk.shape[0])]
    assert bk.shape[0] <= JN_RMAX
    p = join_plan([(kt, bk), (pl.INT32, np.arange(bk.shape[0], dtype=np.int32))],
                  [(kt, pk), (pl.INT32, np.arange(pk.shape[0], dtype=np.int32))], build_left=kt != pl.INT64)
    want = expect(p)
    # every extreme key meets its two build copies 50 times; NaN never matches
    n_bg = int(np.isin(pk, bg).sum())
    assert want[0] >= 2 * 50 * ext.shape[0] + n_bg
    c = make_ctx() if path == "bcast" else make_ctx(radix_bits=int(path.split("=")[1]))
    try:
        if kt == pl.INT32:
            device_hashes_match(c, ext)
        check(p, c, want)
    finally:
        capi.destroy_context(c)


# ----------------------------------------------------------------------- g. sharded owner skew
@pytest.fixture(scope="module")
def g_data():
    """Every key (build and probe, hits and misses) owned by rank 5 of 8 — rank 2 of 4."""
    rng = np.random.default_rng(101)
    nb, npr = 300_000, 600_000
    distinct = hs.keys_with_hash_bits(nb + 100_000, np.int32, owner=5, n_ranks=8, rng=rng)
    assert np.all(hs.owner_rank(distinct, 8) == 5) and np.all(hs.owner_rank(distinct, 4) == 2)
    bk, pk = hits_and_misses(rng, distinct, nb, npr, 0.3)
    bt = pl.make_table([(pl.INT32, bk), (pl.INT32, np.arange(nb, dtype=np.int32))])
    pt = pl.make_table([(pl.INT32, pk), (pl.INT32, rng.integers(-2**31, 2**31 - 1, npr).astype(np.int32))])
    p = pl.Plan()
    p.new_scan_node(0, [(0, pl.INT32), (1, pl.INT32)])
    p.new_scan_node(1, [(0, pl.INT32), (1, pl.INT32)])
    p.new_join_node(True, 0, 1, 0, 0, [(0, pl.INT32), (1, pl.INT32), (3, pl.INT32)])
    p.new_input(bt)
    p.new_input(pt)
    p.root = 2
    return p, bt, bk, expect(p)


@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("n_ranks,bits", [(4, 0), (8, 0), (4, 21), (8, 21)])
def test_g_sharded_one_rank_owns_every_key(g_data, ctx0, n_ranks, bits, fold):
    p, bt, bk, want = g_data
    owner = 5 >> (3 - (n_ranks - 1).bit_length())
    if fold == "1" and bits == 0:  # stage A on the device sends every tuple to the owner
        import torch

        t = ctx0.upload(bt)
        try:
            _, _, counts = dist.GpuOps(ctx0).partition(t, bt.num_rows, n_ranks)
            torch.cuda.synchronize()
        finally:
            t.release()
        assert counts == [bt.num_rows if r == owner else 0 for r in range(n_ranks)]
    old = os.environ.get("RJ_TUNE_FOLD_OWNER")
    os.environ["RJ_TUNE_FOLD_OWNER"] = fold  # read once, when run_sharded creates its context
    try:
        parts = run_sharded(p, n_ranks, **({"radix_bits": bits} if bits else {}))
    finally:
        if old is None:
            del os.environ["RJ_TUNE_FOLD_OWNER"]
        else:
            os.environ["RJ_TUNE_FOLD_OWNER"] = old
    assert sorted(q.num_rows > 0 for q in parts) == [False] * (n_ranks - 1) + [True]  # one rank holds it all
    assert sum(q.num_rows for q in parts) == want[0]
    assert combine([pl.table_digest(q) for q in parts if q.num_rows]) == want[1]
