"""Every compiled join / radix-pass kernel instantiation, driven against the oracle.

The join path is a family of templated kernels (csrc/rj_partition.hip, rj_join.hip, rj_bcast.hip): launch_join picks
k_join<KW, CWR, CWS, OM, PK, TG> from the key width, the carry words per side, the output stream
modes, the tuple layout between the passes and the tagged table; launch_join_bcast picks
k_join_bcast<KW, CWR, CWS>; the pass launchers pick k_pass_hist / k_fine_hist / k_pass_scatter /
k_pass_scatter_packed by loader and layout.  Each instantiation is its own machine code, so each
row of CASES names a plan shape, a path, the RJ_TUNE_* knobs, and the instantiation(s) it must
reach; the library's launch log (rj_debug_launch_log) shows which ones ran.  A row that lands on
another variant fails, and so does a row whose result differs from the oracle's.

What a row's data holds (make_case): duplicate keys on both sides, NULL keys on both sides, NULL
carries wherever the layout has a validity word, INT32 / INT64 extremes and FP64 NaN, +-inf,
subnormals and -0.0 (never +0.0 too: see tests/_refjoin.py) as keys and payloads; for partitioned
rows one probe key with more than JN_HEAVY tuples (heavy-task split) and one build key with more
than JN_RMAX tuples (chunked build); row counts that are multiples of neither PT_TILE nor the
256-key block of the blocked pair layout, and — root joins — a result that spans several output
pages and ends one row past a page boundary.

test_every_compiled_instantiation_is_driven runs the whole table with the log on and checks it
against the kernel handles compiled into librj.so (tests/_elfsyms.py) minus UNREACHABLE."""
import os
import zlib
from dataclasses import dataclass, field

import numpy as np
import pytest

import _elfsyms
import _oracle
from pyrj import capi
from pyrj import plan as pl

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radix-join_amd", "librj.so")

JN_RMAX, JN_HEAVY = 4096, 65536
PT_TILE, BLOCK = 16384, 256
ROWS32, ROWS64 = 1984, 1007
I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR

# the families whose every compiled instantiation must be driven (the helpers — decode, gather,
# scans, encode, VARCHAR — have a single instantiation each or their own suites)
FAMILIES = ("k_join", "k_join_bcast", "k_pass_hist", "k_fine_hist", "k_pass_scatter", "k_pass_scatter_packed")

# Compiled, but no plan can select them.  Both sides of a join are partitioned by the same
# radix_partition() code with the same radix bits, so the packed-pairs flag (PK bit 1 / 2: one key word +
# one carry word, RJ_TUNE_PACK) and the 12-byte-tuple flag (PK bit 4 / 8: one key word + two carry
# words, RJ_TUNE_AOS3) come out equal for two sides of equal carry width (rj_radix_plan.cpp choose_layout():
# P.packed / P.aos3 depend on KW, CW and context knobs only).  join_t compiles every subset of
# CAN, so the one-sided subsets of a same-width pair are dead.
_ONE_SIDED = "both sides have the same carry width, and the radix plan sets the {} flag from KW, CW and the knobs alone: one side cannot have it without the other"
UNREACHABLE = {
    f"k_join<1,1,1,{om},{pk},0>": _ONE_SIDED.format("packed-pairs")
    for om in (0, 1, 2) for pk in (1, 2)
}
UNREACHABLE.update({
    f"k_join<1,2,2,{om},{pk},{tg}>": _ONE_SIDED.format("12-byte-tuple")
    for om in (0, 3) for pk in (4, 8) for tg in (0, 1)
})


@dataclass
class Case:
    """One row of the matrix.  bp / pp: the build / probe payload columns as (type, nullable);
    root=False puts the join under a parent join (dense output streams); path: 'bcast' (build side
    of at most JN_RMAX rows), 'auto' (radix bits from the build size) or forced radix bits;
    knobs: RJ_TUNE_* for a fresh context; key_out: the join outputs its key column;
    ranks: > 1 runs the plan sharded over virtual ranks on one GPU."""
    expect: tuple
    kt: int
    bp: list
    pp: list
    root: bool = True
    build_left: bool = True
    path: object = "auto"
    knobs: dict = field(default_factory=dict)
    key_out: bool = True
    ranks: int = 1
    seed: int = 0

    @property
    def id(self):
        return self.expect[0]


NP0 = dict(RJ_TUNE_PACK="0")
NA0 = dict(RJ_TUNE_AOS3="0")
NPA0 = dict(RJ_TUNE_PACK="0", RJ_TUNE_AOS3="0")
C1 = [(I32, False)]                      # one carry word
C2 = [(I64, False)]                      # two carry words: one 64-bit column (paged at the root)
C2W = [(I32, True)]                      # two carry words: an INT32 column + its validity word
C2WW = [(I32, False), (I32, False)]      # two carry words: two INT32 columns
C3 = [(I64, True)]                       # three carry words: INT64 + validity word (WIDE_64_32)
C3S = [(I32, False), (I32, True)]        # three carry words: two INT32 + validity word (WIDE_32S)
C3SS = [(I32, False), (I32, False), (I32, False)]
CVC = [(VC, False)]                      # a VARCHAR payload: its row index travels, dense stream


def J(*a):
    return "k_join<" + ",".join(map(str, a)) + ">"


def B(*a):
    return "k_join_bcast<" + ",".join(map(str, a)) + ">"


H_SRC1, H_SRC2 = "k_pass_hist<SrcLoader<1,0,0>>", "k_pass_hist<SrcLoader<2,0,0>>"
H_DENSE, H_DIGIT, H_AOS3 = "k_pass_hist<DenseLoaderT<-1>>", "k_pass_hist<DigitLoader>", "k_pass_hist<Aos3KeyLoader>"
H_PACKED, H_BLOCKED = "k_pass_hist<PackedLoader>", "k_pass_hist<BlockedLoader>"
F_SRC1, F_SRC2 = "k_fine_hist<SrcLoader<1,0,0>>", "k_fine_hist<SrcLoader<2,0,0>>"
F_DENSE, F_PACKED = "k_fine_hist<DenseLoaderT<-1>>", "k_fine_hist<PackedLoader>"


def S(nw, loader, pw, aos):
    return f"k_pass_scatter<{nw},{loader},{pw},{'true' if aos else 'false'}>"


def SP(loader, blocked):
    return f"k_pass_scatter_packed<{loader},{'true' if blocked else 'false'}>"


CASES = [
    # ---- one key word, no / one carry word: straight-line emit variants (OM 1 paged, 2 dense)
    Case((J(1, 0, 0, 1, 0, 0), H_SRC1, S(1, "SrcLoader<1,0,0>", -1, 0)), I32, [], []),
    Case((J(1, 0, 0, 2, 0, 0), S(1, "DenseLoaderT<-1>", -1, 0), H_DENSE), I32, [], [], root=False, path=19),
    Case((J(1, 0, 0, 0, 0, 0),), I32, [], [], key_out=False, seed=1),
    Case((J(1, 0, 1, 0, 2, 0), SP("SrcLoader<1,1,0>", 0)), I32, [], C1, key_out=False),
    Case((J(1, 0, 1, 0, 0, 0), S(2, "SrcLoader<1,1,0>", -1, 0)), I32, [], C1, key_out=False, knobs=NP0),
    Case((J(1, 0, 1, 1, 2, 0),), I32, [], C1, build_left=False),
    Case((J(1, 0, 1, 1, 0, 0),), I32, [], C1, knobs=NP0),
    Case((J(1, 0, 1, 2, 2, 0),), I32, [], C1, root=False),
    Case((J(1, 0, 1, 2, 0, 0), S(2, "DenseLoaderT<-1>", -1, 0), H_DENSE), I32, [], C1, root=False, path=16, knobs=NP0),
    Case((J(1, 1, 0, 0, 1, 0),), I32, C1, [], key_out=False),
    Case((J(1, 1, 0, 0, 0, 0),), I32, CVC, [], knobs=NP0),
    Case((J(1, 1, 0, 1, 1, 0), H_BLOCKED, SP("SrcLoader<1,1,0>", 1), SP("BlockedLoader", 0)), I32, C1, [], path=16),
    Case((J(1, 1, 0, 1, 0, 0),), I32, C1, [], knobs=NP0, build_left=False),
    Case((J(1, 1, 0, 2, 1, 0), F_SRC1, SP("SrcLoader<1,1,0>", 0), SP("PackedLoader", 0)), I32, C1, [], root=False, path=12),
    Case((J(1, 1, 0, 2, 0, 0),), I32, CVC, [], root=False, knobs=NP0),
    Case((J(1, 1, 1, 0, 3, 0),), I32, C1, C1, key_out=False),
    Case((J(1, 1, 1, 0, 0, 0),), I32, C1, CVC, knobs=NP0),
    Case((J(1, 1, 1, 1, 3, 0), SP("BlockedLoader", 1), SP("BlockedLoader", 0)), I32, C1, C1, path=19),
    Case((J(1, 1, 1, 1, 0, 0),), I32, C1, C1, knobs=NP0, build_left=False),
    Case((J(1, 1, 1, 2, 3, 0), H_PACKED, SP("PackedLoader", 0)), I32, C1, C1, root=False, path=16,
         knobs=dict(RJ_TUNE_BLOCKED_MID="0")),
    Case((J(1, 1, 1, 2, 0, 0),), I32, CVC, C1, root=False, knobs=NP0),
    # ---- one key word, mixed carry widths: packed / 12-byte layout flags
    Case((J(1, 1, 2, 0, 9, 0), S(3, "SrcLoader<1,2,0>", 1, 1)), I32, C1, C2),
    Case((J(1, 1, 2, 0, 1, 0), S(3, "SrcLoader<1,2,0>", 1, 0)), I32, C1, C2, knobs=NA0, build_left=False),
    Case((J(1, 1, 2, 0, 8, 0), S(3, "SrcLoader<1,2,1>", 1, 0), S(3, "DenseLoaderT<1>", 1, 1)), I32, C1, C2WW, knobs=NP0, path=16),
    Case((J(1, 1, 2, 0, 0, 0),), I32, C1, C2W, knobs=NPA0, path=16),
    # (a two-word build carry at >= 14 radix bits takes the tagged table: the TG=0 rows stay below)
    Case((J(1, 2, 1, 0, 6, 0),), I32, C2, C1),
    Case((J(1, 2, 1, 0, 4, 0),), I32, C2, C1, knobs=NP0, path=13),
    Case((J(1, 2, 1, 0, 2, 0), S(3, "DenseLoaderT<1>", 1, 0)), I32, C2, C1, knobs=NA0, path=12),
    Case((J(1, 2, 1, 0, 0, 0),), I32, C2W, C1, knobs=NPA0, build_left=False),
    Case((J(1, 2, 1, 0, 6, 1), F_SRC1, S(3, "SrcLoader<1,2,0>", 1, 1), S(3, "Aos3Loader", 1, 1)), I32, C2, C1, path=14),
    Case((J(1, 2, 1, 0, 4, 1), H_AOS3), I32, C2, C1, path=16, knobs=dict(RJ_TUNE_PACK="0", RJ_TUNE_AOS_MID="3")),
    Case((J(1, 2, 1, 0, 2, 1),), I32, C2WW, C1, path=14, knobs=NA0, root=False),
    Case((J(1, 2, 1, 0, 0, 1),), I32, C2, C1, path=15, knobs=NPA0),
    Case((J(1, 2, 0, 0, 4, 0), S(3, "SrcLoader<1,2,1>", 1, 1)), I32, C2W, []),
    Case((J(1, 2, 0, 0, 0, 0), S(3, "SrcLoader<1,2,1>", 1, 0)), I32, C2WW, [], knobs=NA0),
    Case((J(1, 2, 0, 0, 4, 1),), I32, C2, [], path=14, build_left=False),
    Case((J(1, 2, 0, 0, 0, 1),), I32, C2, [], path=18, knobs=NA0, root=False),
    Case((J(1, 0, 2, 0, 8, 0), H_DIGIT, S(3, "Aos3Loader", 1, 1)), I32, [], C2, path=16, knobs=dict(RJ_TUNE_AOS_MID="1")),
    Case((J(1, 0, 2, 0, 0, 0),), I32, [], C2W, knobs=NA0, path=16),
    # ---- one key word, two carry words both sides: INT32 key pages + 64-bit carry pages (OM 3)
    Case((J(1, 2, 2, 3, 12, 0), S(3, "SrcLoader<1,2,0>", 1, 1)), I32, C2, C2),
    Case((J(1, 2, 2, 3, 0, 0),), I32, [(F64, False)], C2, knobs=NA0, build_left=False),
    Case((J(1, 2, 2, 3, 12, 1),), I32, C2, [(F64, False)], path=14),
    Case((J(1, 2, 2, 3, 0, 1), S(3, "SrcLoader<1,2,0>", 1, 0), S(3, "DenseLoaderT<1>", 1, 0)), I32, C2, C2,
         path=17, knobs=NA0),
    Case((J(1, 2, 2, 0, 12, 0),), I32, C2, C2, key_out=False),
    Case((J(1, 2, 2, 0, 0, 0),), I32, C2, C2W, knobs=NA0),
    Case((J(1, 2, 2, 0, 12, 1),), I32, C2, C2, path=14, root=False),
    Case((J(1, 2, 2, 0, 0, 1),), I32, C2WW, C2, path=14, knobs=NA0),
    # ---- three carry words (wide carries) on one key word
    Case((J(1, 2, 3, 0, 4, 0), S(4, "SrcLoader<1,3,2>", 2, 0)), I32, C2, C3),
    Case((J(1, 2, 3, 0, 0, 0), S(4, "SrcLoader<1,3,1>", 2, 0)), I32, C2, C3SS, knobs=NA0, build_left=False),
    Case((J(1, 2, 3, 0, 4, 1), S(4, "DenseLoaderT<2>", 2, 0)), I32, C2, C3S, path=14),
    Case((J(1, 2, 3, 0, 0, 1),), I32, C2W, C3, path=14, knobs=NA0, root=False),
    Case((J(1, 3, 2, 0, 8, 0),), I32, C3, C2),
    Case((J(1, 3, 2, 0, 0, 0),), I32, C3S, C2, knobs=NA0, path=16),
    Case((J(1, 1, 3, 0, 1, 0),), I32, C1, C3),
    Case((J(1, 1, 3, 0, 0, 0),), I32, C1, C3SS, knobs=NP0, root=False),
    Case((J(1, 3, 1, 0, 2, 0),), I32, C3, C1, build_left=False),
    Case((J(1, 3, 1, 0, 0, 0),), I32, C3S, C1, knobs=NP0),
    Case((J(1, 0, 3, 0, 0, 0),), I32, [], C3),
    Case((J(1, 3, 0, 0, 0, 0),), I32, C3SS, [], root=False),
    Case((J(1, 3, 3, 0, 0, 0),), I32, C3, C3S, path=19),
    # ---- two key words (INT64 / FP64 keys)
    Case((J(2, 0, 0, 0, 0, 0), H_SRC2, S(2, "SrcLoader<2,0,0>", -1, 0)), I64, [], []),
    Case((J(2, 0, 1, 0, 0, 0), F_SRC2), F64, [], C1, path=12),
    Case((J(2, 0, 2, 0, 0, 0), S(4, "SrcLoader<2,2,0>", 2, 0)), I64, [], C2, build_left=False),
    Case((J(2, 1, 0, 0, 0, 0), S(3, "SrcLoader<2,1,0>", -1, 0), S(3, "DenseLoaderT<-1>", -1, 0)), I64, C1, [], path=16),
    Case((J(2, 1, 1, 0, 0, 0),), F64, C1, C1, root=False),
    Case((J(2, 1, 2, 0, 0, 0), S(4, "SrcLoader<2,2,1>", 2, 0)), I64, C1, C2W),
    Case((J(2, 2, 0, 0, 0, 0), S(4, "DenseLoaderT<2>", 2, 0)), F64, C2, [], path=17),
    Case((J(2, 2, 1, 0, 0, 0),), I64, C2WW, C1, build_left=False),
    Case((J(2, 2, 2, 0, 0, 0),), F64, C2, C2, root=False),
    # ---- sharded stage B over virtual ranks: the fine histogram over tuples that arrived
    Case((J(1, 1, 1, 1, 3, 0), F_PACKED), I32, C1, C1, path=12, ranks=2, knobs=dict(RJ_TUNE_FOLD_OWNER="0")),
    Case((J(2, 1, 1, 0, 0, 0), F_DENSE), I64, C1, C1, path=12, ranks=2, knobs=dict(RJ_TUNE_FOLD_OWNER="0")),
]
# ---- broadcast joins (build side of at most JN_RMAX rows), every carry width pair
_BW = {0: [], 1: C1, 2: C2, 3: C3S}
CASES += [Case((B(1, r, s),), I32, _BW[r], _BW[s], path="bcast", root=(r + s) % 2 == 0, build_left=r != 2, seed=r * 4 + s)
          for r in range(4) for s in range(4)]
_BW2 = {0: [], 1: C1, 2: C2W}
CASES += [Case((B(2, r, s),), (I64, F64)[(r + s) % 2], _BW2[r], _BW2[s], path="bcast", root=r != 1, seed=r * 3 + s)
          for r in range(3) for s in range(3)]


# ------------------------------------------------------------------------------------- data
NP_OF = {I32: np.int32, I64: np.int64, F64: np.float64}
SPECIAL_KEYS = {
    I32: np.array([-2**31, 2**31 - 1, -1, 0], dtype=np.int32),
    I64: np.array([-2**63, 2**63 - 1, -1, 2**32], dtype=np.int64),
    # NaN matches nothing; -0.0 but never +0.0 in one input
    F64: np.array([np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -0.0, 1.7976931348623157e308]),
}


def key_values(kt, k):
    """Distinct integers k >= 0 -> distinct keys of type kt (never +0.0)."""
    if kt == I32:
        return (k.astype(np.int64) * 7919 % (2**31 - 1) - 2**30).astype(np.int32)
    if kt == I64:
        return k.astype(np.int64) * 4_000_000_007 - 12345
    return k.astype(np.float64) * 0.5 + 0.25


def payload(rng, dt, n, nullable):
    if dt == VC:
        return (VC, [b"v%d" % (i % 977) * (1 + i % 3) for i in range(n)])
    if dt == F64:
        v = rng.standard_normal(n)
        sp = np.array([np.nan, np.inf, -np.inf, 5e-324, -0.0, 1e-310])
    elif dt == I64:
        v = rng.integers(-(2**63), 2**63 - 1, n, dtype=np.int64, endpoint=True)
        sp = np.array([-2**63, 2**63 - 1, 0], dtype=np.int64)
    else:
        v = rng.integers(-(2**31), 2**31 - 1, n, dtype=np.int64, endpoint=True).astype(np.int32)
        sp = np.array([-2**31, 2**31 - 1, 0], dtype=np.int32)
    v = v.astype(NP_OF[dt])
    v[rng.choice(n, min(n, 30), replace=False)] = np.resize(sp, min(n, 30))
    if nullable:
        return (dt, v, rng.random(n) >= 0.07)
    return (dt, v)


def _shuffle(rng, keys):
    return keys[rng.permutation(keys.shape[0])]


def _no_tile_multiple(n):
    while n % BLOCK == 0 or n % PT_TILE == 0 or n % ROWS32 == 0 or n % ROWS64 == 0:
        n += 1
    return n


def side_keys(c: Case, rng):
    """-> build keys, probe keys, build-key validity, probe-key validity (numpy)."""
    kt = c.kt
    bcast = c.path == "bcast"
    nb_core = 2_900 if bcast else 24_000
    np_core = 41_000
    dom = int(nb_core * 0.8)
    bk = list(rng.integers(0, dom, nb_core))
    pk = list(rng.integers(0, int(dom * 1.25), np_core))  # a fifth of them miss
    hot, fat, uniq = dom + 1, dom + 2, dom + 3
    bk += [hot, hot, uniq]
    pk += [hot] * (3_000 if bcast else JN_HEAVY + 4_321)  # heavy-task split (partitioned rows)
    if not bcast:
        bk += [fat] * (JN_RMAX + 411)                     # one partition beyond one LDS table
        pk += [fat, fat]
    bkv = key_values(kt, np.array(bk))
    pkv = key_values(kt, np.array(pk))
    sp = SPECIAL_KEYS[kt]
    bkv = np.concatenate([bkv, sp, sp[:2]])
    pkv = np.concatenate([pkv, sp, sp, sp[1:3]])
    uniq_v = key_values(kt, np.array([uniq]))
    # a result of r rows that ends one row past a page boundary of the widest paged stream
    if c.root:
        bvalid = np.ones(bkv.shape[0], bool)
        pvalid = np.ones(pkv.shape[0], bool)
        bvalid[rng.choice(nb_core, nb_core // 50, replace=False)] = False
        pvalid[rng.choice(np_core, np_core // 50, replace=False)] = False
        r = _ref_count(kt, bkv, bvalid, pkv, pvalid)
        rows = ROWS64 if (kt != I32 or any(t in (I64, F64) for t, _ in c.bp + c.pp)) else ROWS32
        extra = (1 - r) % rows
        pkv = np.concatenate([pkv, np.repeat(uniq_v, extra)])
        pvalid = np.concatenate([pvalid, np.ones(extra, bool)])
        assert (r + extra) % rows == 1 and r + extra > 3 * rows
    else:
        bvalid = rng.random(bkv.shape[0]) >= 0.02
        pvalid = rng.random(pkv.shape[0]) >= 0.02
    n_p = _no_tile_multiple(pkv.shape[0])
    pkv = np.concatenate([pkv, np.repeat(key_values(kt, np.array([dom * 3])), n_p - pkv.shape[0])])  # misses
    pvalid = np.concatenate([pvalid, np.ones(n_p - pvalid.shape[0], bool)])
    n_b = _no_tile_multiple(bkv.shape[0])
    bkv = np.concatenate([bkv, np.repeat(key_values(kt, np.array([dom * 4])), n_b - bkv.shape[0])])
    bvalid = np.concatenate([bvalid, np.ones(n_b - bvalid.shape[0], bool)])
    if bcast:
        assert bkv.shape[0] <= JN_RMAX
    pb, pp = rng.permutation(bkv.shape[0]), rng.permutation(pkv.shape[0])
    return bkv[pb], pkv[pp], bvalid[pb], pvalid[pp]


def _ref_count(kt, bk, bv, pk, pv):
    """Result rows of the equi-join: bit-pattern equality, NULL and NaN keys match nothing."""
    def bits(k, v):
        b = k.view(np.int64) if kt == F64 else k.astype(np.int64)
        ok = v & ~(np.isnan(k) if kt == F64 else np.zeros(k.shape[0], bool))
        return b[ok]
    u, cnt = np.unique(bits(bk, bv), return_counts=True)
    q = bits(pk, pv)
    i = np.searchsorted(u, q)
    i = np.minimum(i, u.shape[0] - 1)
    return int(cnt[i][u[i] == q].sum())


def make_case(c: Case):
    """-> plan (Scan JOIN Scan, or that join under a parent join that keeps every row)."""
    rng = np.random.default_rng(4242 + 97 * c.seed + zlib.crc32(c.id.encode()) % 1000)
    bk, pk, bv, pv = side_keys(c, rng)
    bcols = [(c.kt, bk, bv)] + [payload(rng, t, bk.shape[0], nl) for t, nl in c.bp]
    pcols = [(c.kt, pk, pv)] + [payload(rng, t, pk.shape[0], nl) for t, nl in c.pp]
    lcols, rcols = (bcols, pcols) if c.build_left else (pcols, bcols)
    p = pl.Plan()
    ls = p.new_scan_node(0, [(i, col[0]) for i, col in enumerate(lcols)])
    rs = p.new_scan_node(1, [(i, col[0]) for i, col in enumerate(rcols)])
    both = [col[0] for col in lcols] + [col[0] for col in rcols]
    lw = len(lcols)
    outs = ([0] if c.key_out else []) + list(range(1, lw)) + list(range(lw + 1, len(both)))
    j = p.new_join_node(c.build_left, ls, rs, 0, 0, [(i, both[i]) for i in outs])
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(rcols))
    if c.root:
        p.root = j
        return p
    # parent: every distinct usable key once (build) against the child's rows (probe): keeps each row
    assert c.key_out
    kb = bk[bv]
    if c.kt == F64:
        kb = kb[~np.isnan(kb)]
    kb = np.unique(kb.view(np.int64) if c.kt == F64 else kb)
    kb = kb.view(np.float64) if c.kt == F64 else kb
    t3 = p.new_scan_node(2, [(0, c.kt)])
    p.new_input(pl.make_table([(c.kt, kb)]))
    p.root = p.new_join_node(False, j, t3, 0, 0, [(k, both[i]) for k, i in enumerate(outs)])
    return p


# ----------------------------------------------------------------------------------- running
def make_ctx(c: Case):
    env = dict(c.knobs)
    kw = {}
    if isinstance(c.path, int):
        kw["radix_bits"] = c.path
    if c.ranks > 1:
        kw["devices"] = [0] * c.ranks
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


_LIB_SYMS = None


def launched(ctx):
    """{short name: launches} of the context's launch log ("+0x..." entries resolved here)."""
    out = {}
    for name, n in ctx.launches().items():
        if name.startswith("+0x"):
            name = _elfsyms.symbol_at(LIB, int(name[1:], 16)) or name
        if name.startswith("_ZN2rj"):
            name = _elfsyms.short_name(name)
        out[name] = out.get(name, 0) + n
    return out


def run_case(c: Case):
    """-> (device result table(s), {instantiation: launches})"""
    from test_gpu_sharded import shard_table

    p = make_case(c)
    ctx = make_ctx(c)
    try:
        ctx.launch_log(True)
        if c.ranks == 1:
            got = [capi.execute(p, ctx)]
        else:
            shards = [shard_table(t, c.ranks) for t in p.inputs]
            tables = [[ctx.lane(d).upload(shards[i][d]) for i in range(len(p.inputs))] for d in range(c.ranks)]
            try:
                res = ctx.execute_sharded(p, tables)
                got = [r.to_table() for r in res]
                for r in res:
                    r.free()
            finally:
                for row in tables:
                    for t in row:
                        t.release()
        ran = launched(ctx)
        ctx.launch_log(False)
    finally:
        ctx.destroy()
    return p, got, ran


def check_case(c: Case):
    p, got, ran = run_case(c)
    want = _oracle.execute(p)
    assert sum(g.num_rows for g in got) == want.num_rows, (c.id, [g.num_rows for g in got], want.num_rows)
    for g in got:
        assert [col.type for col in g.columns] == [col.type for col in want.columns], c.id
    if any(col.type == VC for col in want.columns):
        assert len(got) == 1 and pl.canonical_rows(got[0]) == pl.canonical_rows(want), c.id
    elif len(got) == 1:
        assert pl.table_digest(got[0]) == pl.table_digest(want), c.id
    else:
        from test_gpu_sharded import combine

        assert combine([pl.table_digest(g) for g in got]) == pl.table_digest(want), c.id
    missing = [e for e in c.expect if e not in ran]
    assert not missing, f"{c.id}: expected {missing} to run; the launch log holds {sorted(ran)}"
    return ran


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id + ("-sharded" if c.ranks > 1 else "") for c in CASES])
def test_kernel_matrix_row(case):
    check_case(case)


def compiled_in_scope():
    return sorted(n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(LIB)) if n.split("<")[0] in FAMILIES)


@pytest.mark.gpu
def test_every_compiled_instantiation_is_driven():
    compiled = set(compiled_in_scope())
    reached = {}
    for c in CASES:
        for name, n in check_case(c).items():
            reached[name] = reached.get(name, 0) + n
    reached_in_scope = compiled & set(reached)
    excused = set(UNREACHABLE) & compiled
    print(f"reached {len(reached_in_scope)} of {len(compiled)} compiled, {len(excused)} excused")
    assert not (compiled - excused) - reached_in_scope, sorted((compiled - excused) - reached_in_scope)
    assert not excused & set(reached), f"UNREACHABLE entries were reached: {sorted(excused & set(reached))}"
    assert len(reached_in_scope) + len(excused) == len(compiled)
