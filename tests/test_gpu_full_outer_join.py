"""Full outer joins (RJ_NODE_FULL) on the device, through the C-ABI, against the numpy reference
tests/_fullref.py (the inner join's pairs, ANTI's rows one way padded on the built side, ANTI's rows
the other way padded on the probed side; tests/test_full_outer_join_plan.py ties it to the pinned
references on the CPU).  Inputs and helpers are those of tests/test_gpu_outer_join.py: there the
"optional" side is the built one and the "preserved" side the probed one.

Device paths: broadcast (k_full_bcast, then k_full_buildrows with the flags), partitioned
(k_full_join, k_full_unmatched, and for the rows the first radix pass drops k_outer_nullkeys on the
probed and k_full_buildrows on the built side), with heavy tasks and with several table rounds.
test_every_full_instantiation_is_driven runs MATRIX with the launch log on and checks it against the
compiled kernel handles (tests/_elfsyms.py)."""
import numpy as np
import pytest

import _elfsyms
import _fullref
import _oracle
import test_gpu_kernel_matrix as km
import test_gpu_outer_join as og
from pyrj import capi
from pyrj import hashing as hs
from pyrj import pages as pg
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
JN_RMAX, JN_HEAVY = og.JN_RMAX, og.JN_HEAVY
FAMILIES = ("k_full_bcast", "k_full_join", "k_full_unmatched", "k_full_buildrows")
LIB = km.LIB
PATHS = og.PATHS
keys, rng_for, sides, payload, run, fam = og.keys, og.rng_for, og.sides, og.payload, og.run, og.fam


def full_plan(bcols, pcols, build_left=True, outs=None, kind="full"):
    """Scan(built: key, payloads...) FULL OUTER Scan(probed: key, payloads...).  outs: list of
    ("b" | "p", column) in output order; default every column, the built side's first.
    kind: "full", "outer", "inner", or "anti" (the BUILT rows without a partner: the probed side
    filters, built columns only)."""
    lcols, rcols = (bcols, pcols) if build_left else (pcols, bcols)
    if outs is None:
        outs = [("b", i) for i in range(len(bcols))] + [("p", i) for i in range(len(pcols))]
    if kind == "anti":
        outs = [o for o in outs if o[0] == "b"]
    p = pl.Plan()
    ls = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
    rs = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])
    lw = len(lcols)
    oa = []
    for side, i in outs:
        left = (side == "b") == build_left
        oa.append(((i if left else lw + i), (bcols if side == "b" else pcols)[i][0]))
    mk = {"full": p.new_full_outer_join_node, "outer": p.new_outer_join_node, "inner": p.new_join_node,
          "anti": p.new_anti_join_node}[kind]
    p.root = mk(build_left if kind != "anti" else not build_left, ls, rs, 0, 0, oa)
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(rcols))
    return p


def check(p, radix_bits=0, log=False, what=""):
    got, ran = run(p, radix_bits, log=log)
    _fullref.same(got, _fullref.execute(p), what)
    return got, ran


def decode(t):
    return [(c.type,) + tuple(np.asarray(x) for x in pg.unpack_fixed(c.pages, t.num_rows, c.type)) for c in t.columns]


def n_valid(t, col):
    return int(np.asarray(pg.unpack_fixed(t.columns[col].pages, t.num_rows, t.columns[col].type)[1], dtype=bool).sum())


# ------------------------------------------------------------------ the main grid
B_SPECS = ([(I32, False), (I64, True)],   # row index + gather: nullable source column
           [(I32, False)],                # wide carry of two words
           [(I32, False), (I32, True)])   # wide carry of three words, a nullable source column
P_SPECS = ([(I32, True), (I64, True)],    # row index + gather
           [(I64, False)],                # wide carry of three words: a 64-bit column + validity
           [(I32, False)])                # wide carry of two words


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("kt", [I32, I64, F64], ids=["i32", "i64", "f64"])
@pytest.mark.parametrize("build_left", [True, False], ids=["build_left", "build_right"])
def test_full_grid(kt, path, build_left):
    """Both sides' keys with NULLs and specials, every column of both sides out (each key column the
    key of its own side), against the reference; the oracle's inner join of the same plan says that
    the case has pairs as well as padded rows.  (On the broadcast path og.sides() draws 20 000
    probed keys over 3 000 values: nearly every built key finds a partner there, so the built rows
    that come out padded are those with NULL / NaN keys.  Built rows padded because their flag stayed
    clear on that path are in test_dup_times_dup_outgrows_the_streams_and_is_rerun[0],
    test_broadcast_boundary[4096], test_all_rows_matched_and_no_row_matched[0] and
    test_mid_scale[bcast].)"""
    rng = rng_for("full-grid", kt, path, build_left)
    bk, bv, pk, pv = sides(kt, path, rng)
    sel = (kt + int(build_left) + list(PATHS).index(path)) % 3
    bcols = [(kt, bk, bv)] + payload(rng, bk.shape[0], B_SPECS[sel])
    pcols = [(kt, pk, pv)] + payload(rng, pk.shape[0], P_SPECS[sel])
    bcols[1] = (I32, np.arange(bk.shape[0], dtype=np.int32))  # never NULL at the source
    p = full_plan(bcols, pcols, build_left)
    got, ran = check(p, PATHS[path][3], log=True, what=(kt, path, build_left))
    if path == "bcast":
        assert fam(ran, "k_full_bcast") and fam(ran, "k_full_buildrows") and not fam(ran, "k_full_join")
    else:
        assert fam(ran, "k_full_join") and fam(ran, "k_full_unmatched") and fam(ran, "k_outer_nullkeys")
        assert fam(ran, "k_full_buildrows") and not fam(ran, "k_full_bcast")
    assert not fam(ran, "k_outer_join") and not fam(ran, "k_outer_bcast")
    if kt == I32 or path == "bcast":
        want = _oracle.execute(full_plan(bcols, pcols, build_left, kind="inner"))
        assert 0 < want.num_rows < got.num_rows


@pytest.mark.gpu
@pytest.mark.parametrize("bnull,pnull", [(True, False), (False, True), (False, False), (True, True)])
@pytest.mark.parametrize("key_out", ["both", "none", "built", "probed"])
def test_null_keys_and_key_columns(bnull, pnull, key_out):
    rng = rng_for("full-nullkeys", bnull, pnull, key_out)
    for path in ("bcast", "part"):
        bk, bv, pk, pv = sides(I32, path, rng, onull=bnull, pnull=pnull)
        bcols = [(I32, bk, bv)] + payload(rng, bk.shape[0], [(I32, False)])
        pcols = [(I32, pk, pv)] + payload(rng, pk.shape[0], [(I32, False)])
        outs = {"both": [("p", 0), ("b", 0), ("b", 1), ("p", 1)], "none": [("p", 1), ("b", 1)],
                "built": [("b", 0), ("p", 1)], "probed": [("p", 0), ("b", 1)]}[key_out]
        _, ran = check(full_plan(bcols, pcols, False, outs), log=True, what=(path, bnull, pnull, key_out))
        if path == "part":
            assert bool(fam(ran, "k_outer_nullkeys")) == pnull
            assert bool(fam(ran, "k_full_buildrows")) == bnull


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64], ids=["i32", "i64"])
def test_heavy_probe_key_flags_its_partners_once(kt):
    """A probe key above 3 x JN_HEAVY tuples is split over several tasks, each of which matches the
    same three build tuples: they are flagged by every task and emitted by none as unmatched."""
    rng = rng_for("full-heavy", kt)
    nb, hot = 30_000, 3 * JN_HEAVY + 777
    ids = rng.permutation(60_000)
    bk = keys(kt, np.concatenate([ids[:nb], [70_000] * 3]))
    pk = keys(kt, np.concatenate([ids[nb // 2:nb // 2 + 20_000], [70_000] * hot]))
    p = full_plan([(kt, bk), (I32, np.arange(bk.shape[0], dtype=np.int32))],
                  [(kt, pk), (I32, np.arange(pk.shape[0], dtype=np.int32))])
    got, ran = check(p, log=True)
    # pairs: 15 000 + 3 x hot; probed alone: 5 000; built alone: 15 000
    assert got.num_rows == 15_000 + 3 * hot + 5_000 + 15_000
    assert n_valid(got, 1) == got.num_rows - 5_000 and n_valid(got, 3) == got.num_rows - 15_000
    assert fam(ran, "k_full_join") and fam(ran, "k_full_unmatched")


@pytest.mark.gpu
def test_heavy_partition_without_build_keys():
    """The hot probed partition has no build tuple: k_heavy_tasks leaves it to the main pass, which
    pads it whole."""
    rng = rng_for("full-heavy-empty")
    bk, bv, pk, pv = sides(I32, "part", rng, hot_in_optional=False)
    p = full_plan([(I32, bk, bv)] + payload(rng, bk.shape[0], [(I64, True)]),
                  [(I32, pk, pv)] + payload(rng, pk.shape[0], [(I32, False)]))
    check(p)


# ------------------------------------------------------------------ duplicates, re-run, rounds
def _dup_plan(rng, nb, npr, bkeys, pkeys, kt=I32):
    bk = keys(kt, rng.integers(0, bkeys, nb))
    pk = keys(kt, rng.integers(0, pkeys, npr))
    return full_plan([(kt, bk), (I32, np.arange(nb, dtype=np.int32))], [(kt, pk), (I64, np.arange(npr, dtype=np.int64))])


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 3])
def test_dup_times_dup_outgrows_the_streams_and_is_rerun(radix_bits):
    """4 000 x 5 000 rows over 100 / 100 keys, half of each side's keys shared: ~100 K pairs against
    streams sized for ~10 K rows, so every kernel of the node runs twice (count, then exact size)."""
    rng = rng_for("full-rerun", radix_bits)
    bk = keys(I32, rng.integers(0, 100, 4_000))
    pk = keys(I32, rng.integers(50, 150, 5_000))
    p = full_plan([(I32, bk), (I32, np.arange(4_000, dtype=np.int32))], [(I32, pk), (I64, np.arange(5_000, dtype=np.int64))])
    got, ran = check(p, radix_bits, log=True)
    assert got.num_rows > 80_000
    assert list(fam(ran, "k_full_join" if radix_bits else "k_full_bcast").values()) == [2], ran
    assert list(fam(ran, "k_full_unmatched" if radix_bits else "k_full_buildrows").values()) == [2], ran


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 3])
def test_result_that_fits_is_not_rerun(radix_bits):
    """Unique keys on both sides: at most built + probed rows, which the first streams hold."""
    rng = rng_for("full-norerun")
    ids = rng.permutation(30_000)
    p = full_plan([(I32, keys(I32, ids[:3_000])), (I32, np.arange(3_000, dtype=np.int32))],
                  [(I32, keys(I32, ids[1_000:21_000])), (I64, np.arange(20_000, dtype=np.int64))])
    got, ran = check(p, radix_bits, log=True)
    assert got.num_rows == 1_000 + 20_000
    assert list(fam(ran, "k_full_join" if radix_bits else "k_full_bcast").values()) == [1], ran


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64], ids=["i32", "i64"])
def test_several_table_rounds_are_exact(kt):
    """One forced partition pair (radix_bits = 1) of ~10 K distinct build keys each: three table
    rounds.  The matched build tuples are spread over all rounds (some are matched only in the last
    one); every key occurs once on each side, so a build tuple flagged in one round and emitted as
    unmatched after another, or one emitted twice, would change the counts."""
    rng = rng_for("full-rounds", kt)
    ids = rng.permutation(40_000)
    bk = keys(kt, ids[:20_000])
    pk = keys(kt, ids[10_000:35_000])  # 10 000 pairs, 15 000 probed alone, 10 000 built alone
    p = full_plan([(kt, bk), (I32, np.arange(20_000, dtype=np.int32))], [(kt, pk), (I32, np.arange(25_000, dtype=np.int32))])
    got, ran = check(p, radix_bits=1, log=True)
    assert got.num_rows == 35_000
    assert n_valid(got, 1) == 20_000 and n_valid(got, 3) == 25_000
    assert fam(ran, "k_full_join")


@pytest.mark.gpu
def test_build_key_duplicated_beyond_a_table_round():
    """Two build keys occur 2 x JN_RMAX + 50 times each in one partition: their copies sit in three
    table rounds.  One has probe partners (every copy is flagged, in its own round), one has none
    (every copy comes out once, padded)."""
    rng = rng_for("full-dupbuild")
    d = 2 * JN_RMAX + 50
    bk = keys(I32, np.concatenate([rng.permutation(9_000), [100_001] * d, [100_002] * d]))
    pk = keys(I32, np.concatenate([rng.integers(4_000, 14_000, 8_000), [100_001] * 3]))
    p = full_plan([(I32, bk), (I32, np.arange(bk.shape[0], dtype=np.int32))], [(I32, pk), (I32, np.arange(pk.shape[0], dtype=np.int32))])
    for bits in (1, 0):
        got, ran = check(p, bits, log=True)
        assert fam(ran, "k_full_join")


@pytest.mark.gpu
@pytest.mark.parametrize("n_built", [JN_RMAX, JN_RMAX + 1])
def test_broadcast_boundary(n_built):
    rng = rng_for("full-boundary", n_built)
    p = _dup_plan(rng, n_built, 30_000, 6_000, 12_000)
    _, ran = check(p, log=True)
    assert bool(fam(ran, "k_full_bcast")) == (n_built == JN_RMAX)
    assert bool(fam(ran, "k_full_join")) == (n_built != JN_RMAX)


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64, F64], ids=["i32", "i64", "f64"])
def test_hash_adversarial_keys(kt):
    """Every key's hash shares its low bits: one partition holds every tuple (several table rounds,
    heavy tasks) and the buckets chain."""
    rng = rng_for("full-adversarial", kt)
    mask = 0xFFFFFFFF if kt != I32 else 0x3FFFF
    distinct = hs.keys_with_hash_bits(12_000, km.NP_OF[kt], 0x2A5A5, mask, rng=rng)
    bk = np.concatenate([distinct[:9_000], distinct[:500]])
    pk = rng.choice(distinct[4_000:], 90_000)
    p = full_plan([(kt, bk, rng.random(bk.shape[0]) >= 0.02), (I32, np.arange(bk.shape[0], dtype=np.int32))],
                  [(kt, pk, rng.random(pk.shape[0]) >= 0.02), (I64, np.arange(pk.shape[0], dtype=np.int64))])
    _, ran = check(p, log=True)
    assert fam(ran, "k_full_join")


# ------------------------------------------------------------------ edge cases
def _small(kt=I32, nb=500, npr=2_000, pkt=None, seed=0, build_left=True):
    rng = rng_for("full-small", kt, nb, npr, pkt, seed)
    bk = keys(kt, rng.integers(0, 300, nb))
    pk = keys(kt if pkt is None else pkt, rng.integers(0, 600, npr))
    pv = rng.random(npr) >= 0.05
    return full_plan([(kt, bk)] + payload(rng, nb, [(I64, True)]),
                     [(kt if pkt is None else pkt, pk, pv)] + payload(rng, npr, [(I32, True)]), build_left)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 5])
@pytest.mark.parametrize("build_left", [True, False])
@pytest.mark.parametrize("empty", ["left", "right"])
def test_one_empty_child(radix_bits, build_left, empty):
    """Every row of the other child, padded; nothing of the empty relation is dereferenced,
    whichever side the hint asks to build."""
    n = 6_000
    p = _small(nb=0 if (empty == "left") == build_left else n, npr=n if (empty == "left") == build_left else 0,
               build_left=build_left)
    got, _ = check(p, radix_bits)
    assert got.num_rows == n


@pytest.mark.gpu
def test_both_children_empty():
    got, _ = check(_small(nb=0, npr=0))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [I32, I64, I32, I32]
    assert all(c.pages.shape[0] == 0 for c in got.columns)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 5])
def test_key_type_mismatch_pads_every_row(radix_bits):
    p = _small(kt=I64, pkt=I32, nb=6_000)
    got, _ = check(p, radix_bits)
    assert got.num_rows == 8_000
    assert n_valid(got, 0) == 6_000  # the built key: valid in the built rows only


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 4])
def test_all_rows_matched_and_no_row_matched(radix_bits):
    rng = rng_for("full-allnone")
    bk = keys(I32, np.arange(3_000))
    bpay = [(I32, np.arange(3_000, dtype=np.int32)), (I64, rng.integers(-5, 5, 3_000))]
    pk_all = keys(I32, np.concatenate([np.arange(3_000), rng.integers(0, 3_000, 7_000)]))
    pk_none = keys(I32, rng.integers(3_000, 6_000, 10_000))
    for pk, rows in ((pk_all, 10_000), (pk_none, 13_000)):
        p = full_plan([(I32, bk)] + bpay, [(I32, pk), (I32, np.arange(10_000, dtype=np.int32))])
        got, _ = check(p, radix_bits)
        assert got.num_rows == rows


# ------------------------------------------------------------------ nesting
def _nest(tag):
    p = pl.Plan()
    for t in og._three_tables(rng_for(tag)):
        p.new_input(t)
    return (p, p.new_scan_node(0, [(0, I32), (1, I64)]), p.new_scan_node(1, [(0, I32), (1, I32)]),
            p.new_scan_node(2, [(0, I32), (1, F64)]))


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
@pytest.mark.parametrize("side", ["left", "right"])
def test_full_under_inner_join_on_a_nullable_column(radix_bits, side):
    """a FULL JOIN b, then joined with c on a's or b's (nullable) key: padded rows drop out."""
    p, a, b, c = _nest("full-nest1")
    o = p.new_full_outer_join_node(False, a, b, 0, 0, [(0, I32), (1, I64), (3, I32), (2, I32)])
    p.root = p.new_join_node(False, o, c, 0 if side == "left" else 3, 0, [(0, I32), (1, I64), (2, I32), (5, F64)])
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_inner_join_under_full_join(radix_bits):
    p, a, b, c = _nest("full-nest2")
    j = p.new_join_node(True, b, c, 0, 0, [(0, I32), (3, F64)])
    p.root = p.new_full_outer_join_node(True, j, a, 0, 0, [(2, I32), (3, I64), (1, F64), (0, I32)])
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_full_under_full(radix_bits):
    """(c FULL JOIN b) FULL JOIN-ed to a on b's nullable key; NULLs of the inner node stay NULL."""
    p, a, b, c = _nest("full-nest3")
    o1 = p.new_full_outer_join_node(False, c, b, 0, 0, [(0, I32), (1, F64), (3, I32)])
    p.root = p.new_full_outer_join_node(True, o1, a, 2, 0, [(3, I32), (4, I64), (2, I32), (1, F64), (0, I32)])
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_full_over_semi_anti_and_outer(radix_bits):
    p, a, b, c = _nest("full-nest4")
    s = p.new_semi_join_node(True, b, a, 0, 0, [(2, I32), (3, I64)])   # rows of a with a partner in b
    t = p.new_anti_join_node(True, b, c, 0, 0, [(2, I32), (3, F64)])   # rows of c without one
    f = p.new_full_outer_join_node(True, t, s, 0, 0, [(2, I32), (3, I64), (1, F64), (0, I32)])
    o = p.new_outer_join_node(True, b, c, 0, 0, [(2, I32), (1, I32)])  # c LEFT JOIN b
    p.root = p.new_full_outer_join_node(False, f, o, 0, 0, [(0, I32), (1, I64), (2, F64), (3, I32), (4, I32), (5, I32)])
    check(p, radix_bits)


# ------------------------------------------------------------------ VARCHAR, malformed nodes
def _vc_plan(which):
    rng = rng_for("full-vc", which)
    n = 2_000
    bk, pk = keys(I32, rng.integers(0, 1_500, n)), keys(I32, rng.integers(0, 3_000, n))
    vb, vp = [b"b%d" % i for i in range(n)], [b"p%d" % i for i in range(n)]
    if which == "key":
        return full_plan([(VC, vb), (I32, bk)], [(VC, vp), (I32, pk)], True, [("p", 1), ("b", 1)])
    if which == "probed_key":  # built key INT32, probed key VARCHAR
        return full_plan([(I32, bk), (I32, bk)], [(VC, vp), (I32, pk)], True, [("p", 1), ("b", 1)])
    bcols = [(I32, bk), (VC, vb) if which == "built" else (I32, np.arange(n, dtype=np.int32))]
    pcols = [(I32, pk), (VC, vp) if which == "probed" else (I32, np.arange(n, dtype=np.int32))]
    return full_plan(bcols, pcols, True, [("p", 1), ("b", 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["built", "probed"])
def test_varchar_column_of_either_side_is_refused(which):
    with pytest.raises(capi.RjError) as e:
        run(_vc_plan(which))
    assert e.value.code == 5 and "VARCHAR" in str(e.value)


@pytest.mark.gpu
def test_varchar_column_is_refused_whatever_the_children_hold():
    """The refusal is a property of the plan: two empty children do not let a VARCHAR column through."""
    e = np.zeros(0, dtype=np.int32)
    p = full_plan([(I32, e), (VC, [])], [(I32, e), (I32, e)], True, [("p", 1), ("b", 1)])
    with pytest.raises(capi.RjError) as err:
        run(p)
    assert err.value.code == 5 and "VARCHAR" in str(err.value)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["key", "probed_key"])
def test_varchar_key_is_unsupported(which):
    with pytest.raises(capi.RjError) as e:
        run(_vc_plan(which))
    assert e.value.code == 5  # RJ_ERR_UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("empty", [False, True])
def test_malformed_nodes_are_argument_errors(empty):
    mk = (lambda: _small(nb=0, npr=0)) if empty else _small
    p = mk()
    p.nodes[p.root].output_attrs.append((9, I32))  # attr out of range
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 1  # RJ_ERR_ARG
    p = mk()
    p.nodes[p.root].output_attrs[1] = (1, I32)  # the column is INT64
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 1


# ------------------------------------------------------------------ multi-device contexts
@pytest.mark.gpu
def test_multi_device_context_falls_back_to_one_device():
    rng = rng_for("full-big")
    n = 2 * 1984 * 1007 + 17  # above the sharding cut of a two-device context
    pk = keys(I32, rng.integers(0, 3_000_000, n))
    bk = keys(I32, rng.integers(0, 3_000_000, 1_000_000))
    p = full_plan([(I32, bk), (I32, np.arange(bk.shape[0], dtype=np.int32))], [(I32, pk), (I32, np.arange(n, dtype=np.int32))])
    ok_, why = capi.plan_shardable(p)
    assert not ok_ and "RJ_NODE_FULL" in why
    got, _ = run(p, devices=[0, 0])
    _fullref.same(got, _fullref.execute(p))


@pytest.mark.gpu
def test_execute_sharded_refuses_full_plans():
    p = _small()
    ctx = capi.Context(devices=[0, 0])
    try:
        tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
        try:
            with pytest.raises(capi.RjError) as e:
                ctx.execute_sharded(p, tables)
            assert e.value.code == 5 and "RJ_NODE_FULL" in str(e.value)
        finally:
            for row in tables:
                for t in row:
                    t.release()
    finally:
        ctx.destroy()


# ------------------------------------------------------------------ a device-only identity
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["bcast", "part", "rounds"])
def test_full_equals_device_outer_plus_device_anti(path):
    """FULL == the device's RJ_NODE_OUTER of the same inputs + the device's RJ_NODE_ANTI of the built
    side against the probed side, padded on the host with NULLs in the probed columns."""
    rng = rng_for("full-identity", path)
    bk, bv, pk, pv = sides(I64, path, rng)
    bcols = [(I64, bk, bv)] + payload(rng, bk.shape[0], [(I32, False), (I32, True)])
    pcols = [(I64, pk, pv)] + payload(rng, pk.shape[0], [(I32, True)])
    bits = PATHS[path][3]
    full, _ = run(full_plan(bcols, pcols), bits)
    outer, _ = run(full_plan(bcols, pcols, kind="outer"), bits)
    anti, _ = run(full_plan(bcols, pcols, kind="anti"), bits)
    assert full.num_rows == outer.num_rows + anti.num_rows and anti.num_rows > 0
    o, a = decode(outer), decode(anti)
    nb = len(bcols)
    cols = []
    for k, (dt, v, m) in enumerate(o):
        if k < nb:
            cols.append((dt, np.concatenate([v, a[k][1]]), np.concatenate([m, a[k][2]]).astype(bool)))
        else:
            cols.append((dt, np.concatenate([v, np.zeros(anti.num_rows, dtype=v.dtype)]),
                         np.concatenate([m, np.zeros(anti.num_rows, dtype=bool)]).astype(bool)))
    want = pl.make_table(cols)
    want.num_rows = full.num_rows
    _fullref.same(full, want, path)


# ------------------------------------------------------------------ mid scale
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["part", "bcast"])
def test_mid_scale(path):
    """20 M probed rows against 20 M (partitioned) or 4 096 (broadcast) built rows, rows without a
    partner on both sides (broadcast: the probed keys cover the lower half of the built keys'
    domain only); row count and order-independent digest."""
    rng = rng_for("full-mid", path)
    n = 20_000_000
    nb = n if path == "part" else JN_RMAX
    bk = rng.permutation(2 * nb)[:nb].astype(np.int32)
    pk = rng.integers(0, 4 * nb if path == "part" else nb, n).astype(np.int32)
    p = full_plan([(I32, bk), (I32, np.arange(nb, dtype=np.int32))], [(I32, pk), (I32, np.arange(n, dtype=np.int32))],
                  False, [("p", 0), ("p", 1), ("b", 1)])
    got, ran = run(p, log=True)
    want = _fullref.execute(p)
    assert got.num_rows == want.num_rows > n
    assert pl.table_digest(got) == pl.table_digest(want)
    assert fam(ran, "k_full_join" if path == "part" else "k_full_bcast")


# ------------------------------------------------------------------ every compiled instantiation
# Carry shapes by key words (KW 1: INT32 keys, KW 2: FP64 keys), the same rules on both sides:
# nothing; more than a wide carry holds (row index + k_outer_gather); wide carries of two and three
# words (the last word is the validity word an optional side always has).
SHAPES = {1: {0: [], 1: [(I64, False), (I32, True), (I32, False)], 2: [(I32, False)], 3: [(I64, True)]},
          2: {0: [], 1: [(I64, False)], 2: [(I32, True)]}}
MATRIX = [(path, kw, cwb, cwp) for path in ("bcast", "part") for kw in (1, 2) for cwb in SHAPES[kw] for cwp in SHAPES[kw]
          if cwb or cwp]
# <KW,0,0>: a node without output columns.  The executor runs it (the row count is the result), but
# no column could show a wrong row, so the rows below check its row count only.
MATRIX_NO_COLUMNS = [(path, kw, 0, 0) for path in ("bcast", "part") for kw in (1, 2)]


def run_matrix_row(row):
    path, kw, cwb, cwp = row
    kt = I32 if kw == 1 else F64
    rng = rng_for("full-matrix", row)
    bk, bv, pk, pv = sides(kt, path, rng)
    bcols = [(kt, bk, bv)] + payload(rng, bk.shape[0], SHAPES[kw][cwb])
    pcols = [(kt, pk, pv)] + payload(rng, pk.shape[0], SHAPES[kw][cwp])
    outs = [("b", i) for i in range(1, len(bcols))] + [("p", i) for i in range(1, len(pcols))]
    p = full_plan(bcols, pcols, (cwb + cwp) % 2 == 0, outs)
    got, ran = run(p, PATHS[path][3], log=True)
    want = _fullref.execute(p)
    assert got.num_rows == want.num_rows, row
    if outs:
        _fullref.same(got, want, row)
    probe = f"{'k_full_bcast' if path == 'bcast' else 'k_full_join'}<{kw},{cwb},{cwp}>"
    after = f"{'k_full_buildrows' if path == 'bcast' else 'k_full_unmatched'}<{kw},{cwb}>"
    assert probe in ran and after in ran, (row, sorted(n for n in ran if n.startswith("k_full")))
    if path == "part":
        assert f"k_full_buildrows<{kw},{cwb}>" in ran, row  # the built rows with NULL / NaN keys
    return ran


@pytest.mark.gpu
def test_every_full_instantiation_is_driven():
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(LIB)) if n.split("<")[0] in FAMILIES}
    assert len(compiled) == 25 + 25 + 7 + 7, sorted(compiled)
    reached = set()
    for row in MATRIX + MATRIX_NO_COLUMNS:
        reached |= {n for n in run_matrix_row(row) if n.split("<")[0] in FAMILIES}
    assert compiled <= reached, sorted(compiled - reached)
