"""Outer joins (RJ_NODE_OUTER) on the device against a numpy reference (tests/_outerref.py: the inner
join's pairs by _refjoin, the padded rows by _filterref's ANTI, with the NULL, NaN and type rules
of include/rj.h; tests/test_outer_join_plan.py ties that reference to the pinned C oracle on the
CPU), and for the matched half also straight against the oracle's inner join of the same plan.

Device paths: broadcast (an optional side of at most JN_RMAX rows, k_outer_bcast), partitioned
(k_outer_join, with a preserved partition above JN_HEAVY tuples that is split into heavy tasks,
and k_outer_nullkeys for the preserved rows the first radix pass drops), and partitioned with
forced radix bits so that a partition's build side needs several table rounds.
test_every_outer_instantiation_is_driven runs MATRIX with the launch log on and checks it against
the compiled kernel handles (tests/_elfsyms.py).

A VARCHAR column of the OPTIONAL side in the output is refused (include/rj.h); a test pins that."""
import zlib

import numpy as np
import pytest

import _elfsyms
import _oracle
import _outerref
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import hashing as hs
from pyrj import pages as pg
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
JN_RMAX, JN_HEAVY = 4096, 65536
FAMILIES = ("k_outer_bcast", "k_outer_join", "k_outer_nullkeys", "k_outer_gather")
LIB = km.LIB

# path -> (optional rows, preserved rows, hot preserved tuples, forced radix bits)
PATHS = {
    "bcast": (3_000, 20_000, 0, 0),
    "part": (24_000, 30_000, JN_HEAVY + 3_210, 0),
    "rounds": (40_000, 30_000, 0, 2),  # 4 partitions of ~10 K build tuples: three table rounds each
}


def keys(kt, k):
    return km.key_values(kt, np.asarray(k))


def rng_for(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def sides(kt, path, rng, onull=True, pnull=True, hot_in_optional=True):
    """-> (optional keys, valid, preserved keys, valid): duplicates on both sides, about half of the
    preserved keys without partner, the type's special keys (NaN, +-inf, extremes) on both sides."""
    no, npr, hot, _ = PATHS[path]
    dom = max(no // 2, 10)
    ok = list(rng.integers(0, dom, no - 40))
    pk = list(rng.integers(0, 2 * dom, npr))
    h = 3 * dom  # a hot preserved key: one partition above JN_HEAVY tuples
    pk += [h] * hot
    if hot_in_optional:
        ok += [h, h]
    okv, pkv = keys(kt, ok), keys(kt, pk)
    sp = km.SPECIAL_KEYS[kt]
    okv = np.concatenate([okv, sp, sp[2:4]])
    pkv = np.concatenate([pkv, sp, sp])
    ov = rng.random(okv.shape[0]) >= (0.03 if onull else 0.0)
    pv = rng.random(pkv.shape[0]) >= (0.03 if pnull else 0.0)
    po, pp = rng.permutation(okv.shape[0]), rng.permutation(pkv.shape[0])
    return okv[po], ov[po], pkv[pp], pv[pp]


def payload(rng, n, spec):
    return [km.payload(rng, t, n, nl) for t, nl in spec]


def outer_plan(ocols, pcols, build_left=True, outs=None, kind="outer"):
    """Scan(optional: key, payloads...) OUTER Scan(preserved: key, payloads...).  outs: list of
    ("o" | "p", column) in output order; default every column, the optional side's first."""
    lcols, rcols = (ocols, pcols) if build_left else (pcols, ocols)
    if outs is None:
        outs = [("o", i) for i in range(len(ocols))] + [("p", i) for i in range(len(pcols))]
    p = pl.Plan()
    ls = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
    rs = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])
    lw = len(lcols)
    oa = []
    for side, i in outs:
        left = (side == "o") == build_left
        oa.append(((i if left else lw + i), (ocols if side == "o" else pcols)[i][0]))
    mk = p.new_outer_join_node if kind == "outer" else p.new_join_node
    p.root = mk(build_left, ls, rs, 0, 0, oa)
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(rcols))
    return p


def run(p, radix_bits=0, devices=None, log=False):
    kw = dict(radix_bits=radix_bits)
    if devices:
        kw["devices"] = devices
    ctx = capi.Context(**kw)
    try:
        if log:
            ctx.launch_log(True)
        got = capi.execute(p, ctx)
        ran = km.launched(ctx) if log else {}
    finally:
        ctx.destroy()
    return got, ran


def check(p, radix_bits=0, log=False, what=""):
    got, ran = run(p, radix_bits, log=log)
    _outerref.same(got, _outerref.execute(p), what)
    return got, ran


def rows_where_valid(t, col):
    """The rows of a fixed-width table whose column `col` is non-NULL, as a table."""
    dec = [pg.unpack_fixed(c.pages, t.num_rows, c.type) for c in t.columns]
    keep = np.asarray(dec[col][1], dtype=bool)
    out = pl.make_table([(c.type, np.asarray(v)[keep], np.asarray(m, dtype=bool)[keep]) for c, (v, m) in zip(t.columns, dec)])
    out.num_rows = int(keep.sum())
    return out


def fam(ran, family):
    return {n: c for n, c in ran.items() if n.split("<")[0] == family}


# ------------------------------------------------------------------ the main grid
O_SPECS = ([(I32, False), (I64, True)],   # row index + gather: nullable source column
           [(I32, False)],                # wide carry of two words
           [(I32, False), (I32, True)])   # wide carry of three words, a nullable source column
P_SPECS = ([(I32, True), (I64, True)], [(I64, False), (I32, False)], [(I32, False)])


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("kt", [I32, I64, F64], ids=["i32", "i64", "f64"])
@pytest.mark.parametrize("build_left", [True, False], ids=["right_outer", "left_outer"])
def test_outer_grid(kt, path, build_left):
    """Both sides' keys with NULLs and specials, every column of both sides out (the optional key
    NULL when padded, the preserved key the row's own), against the reference; the rows whose
    optional row-number column is non-NULL against the oracle's inner join."""
    rng = rng_for("grid", kt, path, build_left)
    ok, ov, pk, pv = sides(kt, path, rng)
    sel = (kt + int(build_left) + list(PATHS).index(path)) % 3
    ocols = [(kt, ok, ov)] + payload(rng, ok.shape[0], O_SPECS[sel])
    pcols = [(kt, pk, pv)] + payload(rng, pk.shape[0], P_SPECS[sel])
    ocols[1] = (I32, np.arange(ok.shape[0], dtype=np.int32))  # never NULL at the source
    p = outer_plan(ocols, pcols, build_left)
    got, ran = check(p, PATHS[path][3], log=True, what=(kt, path, build_left))
    if path == "bcast":
        assert fam(ran, "k_outer_bcast") and not fam(ran, "k_outer_join")
    else:
        assert fam(ran, "k_outer_join") and fam(ran, "k_outer_nullkeys") and not fam(ran, "k_outer_bcast")
    if kt == I32 or path == "bcast":
        want = _oracle.execute(outer_plan(ocols, pcols, build_left, kind="inner"))
        matched = rows_where_valid(got, 1)
        assert 0 < matched.num_rows == want.num_rows < got.num_rows
        assert pl.table_digest(matched) == pl.table_digest(want)


@pytest.mark.gpu
@pytest.mark.parametrize("onull,pnull", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("key_out", ["both", "none", "optional"])
def test_null_keys_and_key_columns(onull, pnull, key_out):
    rng = rng_for("nullkeys", onull, pnull, key_out)
    for path in ("bcast", "part"):
        ok, ov, pk, pv = sides(I32, path, rng, onull=onull, pnull=pnull)
        ocols = [(I32, ok, ov)] + payload(rng, ok.shape[0], [(I32, False)])
        pcols = [(I32, pk, pv)] + payload(rng, pk.shape[0], [(I32, False)])
        outs = {"both": [("p", 0), ("o", 0), ("o", 1), ("p", 1)], "none": [("p", 1), ("o", 1)],
                "optional": [("o", 0), ("p", 1)]}[key_out]
        _, ran = check(outer_plan(ocols, pcols, False, outs), log=True, what=(path, onull, pnull, key_out))
        if path == "part":
            assert bool(fam(ran, "k_outer_nullkeys")) == pnull


@pytest.mark.gpu
def test_heavy_partition_without_optional_keys():
    """The hot preserved partition has no build tuple: k_heavy_tasks leaves it to the main pass,
    which pads it whole."""
    rng = rng_for("heavy-empty")
    ok, ov, pk, pv = sides(I32, "part", rng, hot_in_optional=False)
    p = outer_plan([(I32, ok, ov)] + payload(rng, ok.shape[0], [(I64, True)]),
                   [(I32, pk, pv)] + payload(rng, pk.shape[0], [(I32, False)]))
    check(p)


# ------------------------------------------------------------------ duplicates, re-run, rounds
def _dup_plan(rng, no, npr, okeys, pkeys, kt=I32):
    ok = keys(kt, rng.integers(0, okeys, no))
    pk = keys(kt, rng.integers(0, pkeys, npr))
    return outer_plan([(kt, ok), (I32, np.arange(no, dtype=np.int32))],
                      [(kt, pk), (I64, np.arange(npr, dtype=np.int64))])


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 3])
def test_dup_times_dup_outgrows_the_streams_and_is_rerun(radix_bits):
    """4 000 x 5 000 rows over 50 / 100 keys: ~200 K matched rows + ~2 500 padded ones against
    streams sized for ~6 K rows, so the probe kernel runs twice (count, then exact size)."""
    rng = rng_for("rerun", radix_bits)
    p = _dup_plan(rng, 4_000, 5_000, 50, 100)
    got, ran = check(p, radix_bits, log=True)
    assert got.num_rows > 150_000
    probe = fam(ran, "k_outer_join" if radix_bits else "k_outer_bcast")
    assert list(probe.values()) == [2], ran


@pytest.mark.gpu
def test_result_that_fits_is_not_rerun():
    """Unique optional keys: the result has exactly the preserved side's rows, which the first
    streams hold."""
    rng = rng_for("norerun")
    p = outer_plan([(I32, keys(I32, rng.permutation(3_000))), (I32, np.arange(3_000, dtype=np.int32))],
                   [(I32, keys(I32, rng.integers(0, 6_000, 20_000))), (I64, np.arange(20_000, dtype=np.int64))])
    got, ran = check(p, log=True)
    assert got.num_rows == 20_000
    assert list(fam(ran, "k_outer_bcast").values()) == [1], ran


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64], ids=["i32", "i64"])
def test_several_table_rounds_are_exact(kt):
    """One forced partition pair (radix_bits = 1) of ~10 K distinct build keys each: three table
    rounds.  Every preserved key occurs once, so a tuple that matched only in the last round and
    came out padded as well, or an unmatched one that came out twice, would change the row count."""
    rng = rng_for("rounds", kt)
    ids = rng.permutation(40_000)
    ok = keys(kt, ids[:20_000])
    pk = keys(kt, ids[10_000:35_000])  # 10 000 with a partner, 15 000 without
    p = outer_plan([(kt, ok), (I32, np.arange(20_000, dtype=np.int32))], [(kt, pk), (I32, np.arange(25_000, dtype=np.int32))])
    got, ran = check(p, radix_bits=1, log=True)
    assert got.num_rows == 25_000
    assert rows_where_valid(got, 1).num_rows == 10_000
    assert fam(ran, "k_outer_join")


@pytest.mark.gpu
@pytest.mark.parametrize("n_opt", [JN_RMAX, JN_RMAX + 1])
def test_broadcast_boundary(n_opt):
    rng = rng_for("boundary", n_opt)
    p = _dup_plan(rng, n_opt, 30_000, 6_000, 12_000)
    _, ran = check(p, log=True)
    assert bool(fam(ran, "k_outer_bcast")) == (n_opt == JN_RMAX)
    assert bool(fam(ran, "k_outer_join")) == (n_opt != JN_RMAX)


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_hash_adversarial_keys(kt):
    """Every key's hash shares its low bits (the 64-bit ones their whole low word): one partition
    holds every tuple (several table rounds, heavy tasks) and the buckets chain."""
    rng = rng_for("adversarial", kt)
    npt = km.NP_OF[kt]
    mask = 0xFFFFFFFF if kt != I32 else 0x3FFFF
    distinct = hs.keys_with_hash_bits(12_000, npt, 0x2A5A5, mask, rng=rng)
    ok = np.concatenate([distinct[:9_000], distinct[:500]])
    pk = rng.choice(distinct, 90_000)
    p = outer_plan([(kt, ok, rng.random(ok.shape[0]) >= 0.02), (I32, np.arange(ok.shape[0], dtype=np.int32))],
                   [(kt, pk, rng.random(pk.shape[0]) >= 0.02), (I64, np.arange(pk.shape[0], dtype=np.int64))])
    _, ran = check(p, log=True)
    assert fam(ran, "k_outer_join")


# ------------------------------------------------------------------ edge cases
def _small(kt=I32, no=500, npr=2_000, pkt=None, seed=0, build_left=True):
    rng = rng_for("small", kt, no, npr, pkt, seed)
    ok = keys(kt, rng.integers(0, 300, no))
    pk = keys(kt if pkt is None else pkt, rng.integers(0, 600, npr))
    pv = rng.random(npr) >= 0.05
    return outer_plan([(kt, ok)] + payload(rng, no, [(I64, True)]),
                      [(kt if pkt is None else pkt, pk, pv)] + payload(rng, npr, [(I32, True)]), build_left)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 5])
@pytest.mark.parametrize("opay", [[(I64, True)], [(I64, False), (F64, False)], []])
def test_empty_optional_side(radix_bits, opay):
    """Every preserved row, padded; nothing of the (empty) optional relation is dereferenced."""
    rng = rng_for("empty-opt")
    pk = keys(I32, rng.integers(0, 600, 2_000))
    p = outer_plan([(I32, np.zeros(0, np.int32))] + payload(rng, 0, opay),
                   [(I32, pk, rng.random(2_000) >= 0.05)] + payload(rng, 2_000, [(I32, True)]))
    got, _ = check(p, radix_bits)
    assert got.num_rows == 2_000
    assert not pg.unpack_fixed(got.columns[0].pages, 2_000, I32)[1].any()


@pytest.mark.gpu
def test_empty_preserved_side():
    got, _ = check(_small(npr=0))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [I32, I64, I32, I32]
    assert all(c.pages.shape[0] == 0 for c in got.columns)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 5])
def test_key_type_mismatch_pads_every_row(radix_bits):
    p = _small(kt=I64, pkt=I32, no=6_000)
    got, _ = check(p, radix_bits)
    assert got.num_rows == 2_000
    assert not pg.unpack_fixed(got.columns[1].pages, 2_000, I64)[1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 4])
def test_all_rows_matched_and_no_row_matched(radix_bits):
    rng = rng_for("allnone")
    ok = keys(I32, np.arange(3_000))
    opay = [(I32, np.arange(3_000, dtype=np.int32)), (I64, rng.integers(-5, 5, 3_000))]
    pk_all = keys(I32, rng.integers(0, 3_000, 10_000))
    pk_none = keys(I32, rng.integers(3_000, 6_000, 10_000))
    for pk, matched in ((pk_all, 10_000), (pk_none, 0)):
        p = outer_plan([(I32, ok)] + opay, [(I32, pk), (I32, np.arange(10_000, dtype=np.int32))])
        got, _ = check(p, radix_bits)
        assert got.num_rows == 10_000
        assert int(pg.unpack_fixed(got.columns[1].pages, 10_000, I32)[1].sum()) == matched


# ------------------------------------------------------------------ nesting
def _three_tables(rng, n=30_000):
    a = keys(I32, rng.integers(0, 20_000, n))
    b = keys(I32, rng.integers(0, 20_000, n // 2))
    c = keys(I32, rng.integers(0, 40_000, n))
    return [pl.make_table([(I32, a, rng.random(n) >= 0.02), (I64, rng.integers(-9, 9, n))]),
            pl.make_table([(I32, b), (I32, b)]),
            pl.make_table([(I32, c), (F64, rng.standard_normal(n))])]


def _nest(tag):
    p = pl.Plan()
    for t in _three_tables(rng_for(tag)):
        p.new_input(t)
    return (p, p.new_scan_node(0, [(0, I32), (1, I64)]), p.new_scan_node(1, [(0, I32), (1, I32)]),
            p.new_scan_node(2, [(0, I32), (1, F64)]))


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_outer_under_inner_join_on_a_nullable_column(radix_bits):
    """a LEFT JOIN b, then joined with c on b's (nullable) copy of the key: padded rows drop out."""
    p, a, b, c = _nest("nest1")
    o = p.new_outer_join_node(False, a, b, 0, 0, [(0, I32), (1, I64), (3, I32)])
    p.root = p.new_join_node(False, o, c, 2, 0, [(0, I32), (1, I64), (2, I32), (4, F64)])
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_inner_join_under_outer_join(radix_bits):
    p, a, b, c = _nest("nest2")
    j = p.new_join_node(True, b, c, 0, 0, [(0, I32), (3, F64)])
    p.root = p.new_outer_join_node(True, j, a, 0, 0, [(2, I32), (3, I64), (1, F64), (0, I32)])  # a RIGHT-preserved
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_outer_under_outer(radix_bits):
    """(c LEFT JOIN b) LEFT JOIN-ed to a on b's nullable key; NULLs of the inner node stay NULL."""
    p, a, b, c = _nest("nest3")
    o1 = p.new_outer_join_node(False, c, b, 0, 0, [(0, I32), (1, F64), (3, I32)])
    p.root = p.new_outer_join_node(True, o1, a, 2, 0, [(3, I32), (4, I64), (2, I32), (1, F64)])
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_outer_over_semi_and_anti(radix_bits):
    p, a, b, c = _nest("nest4")
    s = p.new_semi_join_node(True, b, a, 0, 0, [(2, I32), (3, I64)])   # rows of a with a partner in b
    t = p.new_anti_join_node(True, b, c, 0, 0, [(2, I32), (3, F64)])   # rows of c without one
    p.root = p.new_outer_join_node(True, t, s, 0, 0, [(2, I32), (3, I64), (1, F64)])
    check(p, radix_bits)


# ------------------------------------------------------------------ VARCHAR, malformed nodes
def _vc_plan(n_pre, optional_vc=False, key_vc=False):
    rng = rng_for("vc", n_pre)
    no = 2_000
    ok = keys(I32, rng.integers(0, 1_500, no))
    pk = keys(I32, rng.integers(0, 3_000, n_pre))
    vo = [b"o%d" % i for i in range(no)]
    vp = [None if i % 11 == 0 else b"p%d" % (i % 1013) * (1 + i % 3) for i in range(n_pre)]
    if key_vc:
        return outer_plan([(VC, vo), (I32, ok)], [(VC, vp), (I32, pk)], True, [("p", 1), ("o", 1)])
    ocols = [(I32, ok), (VC, vo) if optional_vc else (I32, np.arange(no, dtype=np.int32))]
    pcols = [(I32, pk, rng.random(n_pre) >= 0.03), (VC, vp), (F64, rng.standard_normal(n_pre), rng.random(n_pre) >= 0.1)]
    return outer_plan(ocols, pcols, True, [("p", 1), ("o", 1), ("p", 0), ("p", 2)])


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 4])
def test_varchar_payload_on_the_preserved_side(radix_bits):
    check(_vc_plan(5_000), radix_bits)


@pytest.mark.gpu
def test_varchar_payload_on_the_preserved_side_large_result():
    """Enough rows for the device VARCHAR encoder."""
    got, _ = run(_vc_plan(400_000))
    want = _outerref.execute(_vc_plan(400_000))
    assert got.num_rows == want.num_rows
    g, w = pl.decode_table(got), pl.decode_table(want)
    assert sorted(x or b"\xff" for x in g[0]) == sorted(x or b"\xff" for x in w[0])
    fixed = lambda t: pl.ColumnarTable(t.num_rows, t.columns[1:])
    assert pl.table_digest(fixed(got)) == pl.table_digest(fixed(want))


@pytest.mark.gpu
def test_varchar_column_of_the_optional_side_is_refused():
    with pytest.raises(capi.RjError) as e:
        run(_vc_plan(5_000, optional_vc=True))
    assert e.value.code == 5 and "VARCHAR" in str(e.value) and "optional" in str(e.value)


@pytest.mark.gpu
def test_varchar_key_is_unsupported():
    with pytest.raises(capi.RjError) as e:
        run(_vc_plan(100, key_vc=True))
    assert e.value.code == 5  # RJ_ERR_UNSUPPORTED


@pytest.mark.gpu
def test_malformed_nodes_are_argument_errors():
    p = _small()
    p.nodes[p.root].output_attrs.append((9, I32))  # attr out of range
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 1  # RJ_ERR_ARG
    p = _small()
    p.nodes[p.root].output_attrs[1] = (1, I32)  # the column is INT64
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 1


# ------------------------------------------------------------------ multi-device contexts
@pytest.mark.gpu
def test_multi_device_context_falls_back_to_one_device():
    rng = rng_for("big")
    n = 2 * 1984 * 1007 + 17  # above the sharding cut of a two-device context
    pk = keys(I32, rng.integers(0, 3_000_000, n))
    ok = keys(I32, rng.integers(0, 3_000_000, 1_000_000))
    p = outer_plan([(I32, ok), (I32, np.arange(ok.shape[0], dtype=np.int32))], [(I32, pk), (I32, np.arange(n, dtype=np.int32))])
    ok_, why = capi.plan_shardable(p)
    assert not ok_ and "RJ_NODE_OUTER" in why
    got, _ = run(p, devices=[0, 0])
    _outerref.same(got, _outerref.execute(p))


@pytest.mark.gpu
def test_execute_sharded_refuses_outer_plans():
    p = _small()
    ctx = capi.Context(devices=[0, 0])
    try:
        tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
        try:
            with pytest.raises(capi.RjError) as e:
                ctx.execute_sharded(p, tables)
            assert e.value.code == 5 and "RJ_NODE_OUTER" in str(e.value)
        finally:
            for row in tables:
                for t in row:
                    t.release()
    finally:
        ctx.destroy()


# ------------------------------------------------------------------ mid scale
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["part", "bcast"])
def test_mid_scale(path):
    """20 M preserved rows against 20 M (partitioned) or 4 096 (broadcast) optional rows, about
    half of the preserved rows matched; row count and order-independent digest."""
    rng = rng_for("mid", path)
    n = 20_000_000
    no = n if path == "part" else JN_RMAX
    ok = rng.permutation(2 * no)[:no].astype(np.int32)
    pk = rng.integers(0, 4 * no, n).astype(np.int32)
    p = outer_plan([(I32, ok), (I32, np.arange(no, dtype=np.int32))], [(I32, pk), (I32, np.arange(n, dtype=np.int32))],
                   False, [("p", 0), ("p", 1), ("o", 1)])
    got, ran = run(p, log=True)
    want = _outerref.execute(p)
    assert got.num_rows == want.num_rows == n
    assert pl.table_digest(got) == pl.table_digest(want)
    assert fam(ran, "k_outer_join" if path == "part" else "k_outer_bcast")


# ------------------------------------------------------------------ every compiled instantiation
# Carry shapes by key words (KW 1: INT32 keys, KW 2: FP64 keys).  Optional side: nothing; more than a
# wide carry holds (row index + k_outer_gather); wide carries of two and three words.  Preserved
# side: nothing, one 32-bit column, one 64-bit column, a wide carry of three words.
OPT_SHAPES = {1: {0: [], 1: [(I64, False), (I32, True), (I32, False)], 2: [(I32, False)], 3: [(I64, True)]},
              2: {0: [], 1: [(I64, False)], 2: [(I32, True)]}}
PRE_SHAPES = {1: {0: [], 1: [(I32, False)], 2: [(I64, False)], 3: [(I64, False), (I32, False)]},
              2: {0: [], 1: [(I32, False)], 2: [(F64, False)]}}
MATRIX = [(path, kw, cwb, cwp) for path in ("bcast", "part") for kw in (1, 2)
          for cwb in OPT_SHAPES[kw] for cwp in PRE_SHAPES[kw]]


def run_matrix_row(row):
    path, kw, cwb, cwp = row
    kt = I32 if kw == 1 else F64
    rng = rng_for("matrix", row)
    # INT32 preserved keys are nullable (k_outer_nullkeys) and therefore not output: the key would
    # travel as a carry; FP64 preserved keys may be NaN and go out through the key stream
    ok, ov, pk, pv = sides(kt, path, rng, pnull=kw == 1)
    ocols = [(kt, ok, ov)] + payload(rng, ok.shape[0], OPT_SHAPES[kw][cwb])
    pcols = [(kt, pk, pv)] + payload(rng, pk.shape[0], PRE_SHAPES[kw][cwp])
    outs = [("o", i) for i in range(1, len(ocols))] + [("p", i) for i in range(0 if kw == 2 else 1, len(pcols))]
    _, ran = check(outer_plan(ocols, pcols, cwb % 2 == 0, outs), PATHS[path][3], log=True, what=row)
    name = f"{'k_outer_bcast' if path == 'bcast' else 'k_outer_join'}<{kw},{cwb},{cwp}>"
    assert name in ran, (row, sorted(n for n in ran if n.startswith("k_outer")))
    return ran


@pytest.mark.gpu
def test_every_outer_instantiation_is_driven():
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(LIB)) if n.split("<")[0] in FAMILIES}
    assert len(compiled) == 25 + 25 + 7 + 2, sorted(compiled)
    reached = set()
    for row in MATRIX:
        reached |= {n for n in run_matrix_row(row) if n.split("<")[0] in FAMILIES}
    assert compiled <= reached, sorted(compiled - reached)
