"""The scatter kernels' ranking and loaders, driven where the branch-free ranking can go wrong.

The first pass of a key + two-word-carry plan (k_pass_scatter<3,SrcLoader<1,2,*>,1,*>) ranks a tile
with one LDS atomic per item and no branch: an item that holds no tuple (past the end of a partial
tile, NULL key) adds to one of PT_DUMMY dummy counters behind the real ones, and ranks and LDS
positions travel two per register (14 bits of rank) (csrc/rj_partition.hip: rank_tile, place_tile).
The other shapes here keep a branch per item; they share the kernel template, the loaders and the
counter array with it, so the same data goes through them.  What can break, per plan shape:

  nulls        NULL keys in every one of a thread's 16 item positions, under both row mappings of
               a tile (strided: rows t + 1024 j; vector: rows 4 t .. 4 t + 3 of every 4096), on
               both sides, plus scattered ones — dummy counters next to real ranks in one thread
  null_tile    a whole first tile of NULL keys on both sides: dummy counters only, the tile
               reserves nothing and writes nothing
  tail_one     a single valid tuple in the partial last tile of the probe side
  one_key      the probe side holds one key throughout (>= 3 tiles): one digit owns the tile and
               ranks reach PT_TILE - 1, the last value the packed rank has bits for; the build side
               has that key exactly once
  all_digits   the low 9 bits of the key hash (pyrj.hashing: radix digits come from the low bits)
               take all 512 values on the probe side, value d in at least 1 + d // 4 rows, shuffled:
               every tile sees (nearly) every digit, with runs from a tuple or two up to about a
               hundred.  What the other 9-bit digit looks like is left to the hash

Every case is a join plan through the public API on a fresh context with forced radix bits (two
passes of 9 bits, each with a histogram of its own), XCD placement forced on and the launch log on;
the result is compared with the oracle's as a multiset, its row count with the count worked out
here from the keys (rows with NULL keys never appear, every other probe row once per build match),
and the log must name the instantiations the shape is there for.  Row counts are multiples of
neither PT_TILE nor the 256-key block of the blocked pair layout."""
import os

import numpy as np
import pytest

import _oracle
from pyrj import capi
from pyrj import hashing
from pyrj import plan as pl
from test_gpu_kernel_matrix import S, SP, launched

PT_TILE, PT_THREADS = 16384, 1024
I32, I64 = pl.INT32, pl.INT64
N_PROBE = 3 * PT_TILE + 1029
N_BUILD = PT_TILE + 4 * 1029 + 3
RADIX_BITS = 18  # 9 + 9: 512 digits per pass
KNOBS = dict(RJ_TUNE_XCD_SPLIT="1", RJ_TUNE_XCD_MIN_ROWS="1")  # XCD placement for passes of any size

# shape id -> (key type, payload type, the instantiations it is there for)
SHAPES = {
    "i32_i64": (I32, I64, (S(3, "SrcLoader<1,2,0>", 1, 0), S(3, "DenseLoaderT<1>", 1, 1))),
    "i32_i32": (I32, I32, (SP("SrcLoader<1,1,0>", 1), SP("BlockedLoader", 0))),
    "i64_i64": (I64, I64, (S(4, "SrcLoader<2,2,0>", 2, 0), S(4, "DenseLoaderT<2>", 2, 0))),
}
DATA = ("nulls", "null_tile", "tail_one", "one_key", "all_digits")


def keys_of(kt, k):
    """Distinct integers k >= 0 -> distinct keys of type kt."""
    k = np.asarray(k, dtype=np.int64)
    if kt == I32:
        return (k * 7919 % (2**31 - 1) - 2**30).astype(np.int32)
    return k * 4_000_000_007 - 12345


def low_digit(kt, keys):
    """The low 9 bits of the device hash of the keys."""
    h = hashing.key_hash(keys, kt != I32)
    return (h & type(h.flat[0])(511)).astype(np.int64)


def every_item_position_null(n):
    """Rows that are ALL 16 items of one thread, in the strided and in the vector mapping of a tile."""
    i = np.arange(n)
    return (i % PT_THREADS == 7) | ((i % (4 * PT_THREADS)) // 4 == 5)


def make_sides(kt, data, rng):
    """-> build keys, build validity, probe keys, probe validity"""
    dom = 9000
    bk = np.concatenate([np.arange(dom), rng.integers(0, dom, N_BUILD - dom)])  # every key at least once
    pk = rng.integers(0, int(dom * 1.25), N_PROBE)                              # a fifth of them miss
    bv, pv = np.ones(N_BUILD, bool), np.ones(N_PROBE, bool)
    if data == "nulls":
        bv &= ~every_item_position_null(N_BUILD) & (rng.random(N_BUILD) >= 0.03)
        pv &= ~every_item_position_null(N_PROBE) & (rng.random(N_PROBE) >= 0.03)
    elif data == "null_tile":
        bk = rng.permutation(bk)
        bv[:PT_TILE] = False
        pv[:PT_TILE] = False
    elif data == "tail_one":
        pv[3 * PT_TILE:] = False
        pv[3 * PT_TILE + 517] = True
        pk[3 * PT_TILE + 517] = 11
    elif data == "one_key":
        pk[:] = dom + 5
        bk = rng.permutation(np.concatenate([bk[:-1], [dom + 5]]))
    elif data == "all_digits":
        cand = np.arange(400_000)
        dg = low_digit(kt, keys_of(kt, cand))
        order = np.argsort(dg, kind="stable")
        starts = np.searchsorted(dg[order], np.arange(512))
        runs = [cand[order[starts[d]:starts[d] + 1 + d // 4]] for d in range(512)]  # at least 1 .. 128 rows per digit
        assert all(r.shape[0] == 1 + d // 4 for d, r in enumerate(runs))
        core = np.concatenate(runs)
        pk = rng.permutation(np.concatenate([core, rng.choice(core, N_PROBE - core.shape[0])]))
        bk = rng.permutation(np.concatenate([core[: N_BUILD // 2], rng.integers(0, dom, N_BUILD - N_BUILD // 2)]))
        assert np.unique(low_digit(kt, keys_of(kt, pk[:PT_TILE]))).shape[0] > 500
    assert bk.shape[0] == N_BUILD and pk.shape[0] == N_PROBE
    return keys_of(kt, bk), bv, keys_of(kt, pk), pv


def expected_rows(bk, bv, pk, pv):
    u, cnt = np.unique(bk[bv], return_counts=True)
    q = pk[pv]
    i = np.minimum(np.searchsorted(u, q), u.shape[0] - 1)
    return int(cnt[i][u[i] == q].sum())


def payload(rng, dt, n):
    if dt == I64:
        return (dt, rng.integers(-(2**63), 2**63 - 1, n, dtype=np.int64, endpoint=True))
    return (dt, rng.integers(-(2**31), 2**31 - 1, n, dtype=np.int64, endpoint=True).astype(np.int32))


_CASES = {}


def case(shape, data):
    """(plan, oracle result, expected row count): built once and left unchanged."""
    if (shape, data) not in _CASES:
        kt, ct, _ = SHAPES[shape]
        rng = np.random.default_rng(977 + 31 * sorted(SHAPES).index(shape) + DATA.index(data))
        bk, bv, pk, pv = make_sides(kt, data, rng)
        bcols = [(kt, bk, bv), payload(rng, ct, N_BUILD)]
        pcols = [(kt, pk, pv), payload(rng, ct, N_PROBE)]
        p = pl.Plan()
        ls = p.new_scan_node(0, [(0, kt), (1, ct)])
        rs = p.new_scan_node(1, [(0, kt), (1, ct)])
        p.root = p.new_join_node(True, ls, rs, 0, 0, [(0, kt), (1, ct), (3, ct)])
        p.new_input(pl.make_table(bcols))
        p.new_input(pl.make_table(pcols))
        _CASES[shape, data] = (p, _oracle.execute(p), expected_rows(bk, bv, pk, pv))
    return _CASES[shape, data]


def fresh_context():
    old = {k: os.environ.get(k) for k in KNOBS}
    os.environ.update(KNOBS)  # read once, when the context is created
    try:
        return capi.Context(radix_bits=RADIX_BITS)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_scatter_rank(shape, data):
    p, want, rows = case(shape, data)
    assert want.num_rows == rows, (want.num_rows, rows)  # the reference itself: NULL keys never match
    if data == "one_key":
        assert rows == N_PROBE
    ctx = fresh_context()
    try:
        ctx.launch_log(True)
        got = capi.execute(p, ctx)
        ran = launched(ctx)
        ctx.launch_log(False)
    finally:
        ctx.destroy()
    missing = [e for e in SHAPES[shape][2] if e not in ran]
    assert not missing, f"expected {missing} to run; the launch log holds {sorted(ran)}"
    assert got.num_rows == rows, (got.num_rows, rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns]
    assert pl.table_digest(got) == pl.table_digest(want)
