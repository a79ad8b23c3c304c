"""Aggregation nodes (RJ_NODE_AGG) on the device, through the C-ABI, against the numpy reference
tests/_aggref.py (tests/test_agg_plan.py ties it to a Python dict and to the pinned C oracle on the
CPU).  Every group is compared: row by row (pl.canonical_rows) at small sizes, by row count and
order-independent digest (pl.table_digest) from 2 M rows on.

Device paths: k_agg_parts per partition (one table round, or several when a partition holds more
keys than the LDS table), heavy tasks that meet in the merge table (k_agg_merge_init, k_agg_emit),
k_agg_nullkey for the rows with a NULL key, k_agg_column for narrowed / nullable result columns.
test_every_agg_instantiation_is_driven runs MATRIX with the launch log on and checks it against the
compiled kernel handles (tests/_elfsyms.py)."""
import os
import re

import numpy as np
import pytest

import _aggref
import _elfsyms
import test_agg_plan as ap
import test_gpu_kernel_matrix as km
import test_gpu_outer_join as og
from pyrj import capi
from pyrj import hashing as hs
from pyrj import pages as pg
from pyrj import plan as pl

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
KEY, STAR, COUNT, SUM, MIN, MAX = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_COUNT, pl.AGG_SUM, pl.AGG_MIN, pl.AGG_MAX
JN_HEAVY = og.JN_HEAVY
# the LDS table's entries, read from the kernels' header: the round tests below prove from it that a
# workgroup's table cannot have held its keys in one round
AGG_CAP = int(re.search(r"constexpr int AGG_CAP\s*=\s*(\d+);", open(os.path.join(
    os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()).group(1))
FAMILIES = ("k_agg_parts", "k_agg_nullkey", "k_agg_emit", "k_agg_merge_init", "k_agg_column")
LIB = km.LIB
rng_for, run, fam, keys, agg_plan = og.rng_for, og.run, og.fam, og.keys, ap.agg_plan
ALL = ap.ALL


def check(p, radix_bits=0, log=False, what="", rows=None):
    got, ran = run(p, radix_bits, log=log)
    want = _aggref.execute(p)
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    if rows is None:
        rows = want.num_rows <= 50_000
    if rows:
        assert pl.canonical_rows(got) == pl.canonical_rows(want), what
    else:
        assert pl.table_digest(got) == pl.table_digest(want), what
    return got, ran


def table(rng, n, kt=I32, vt=I64, groups=1000, key_nulls=0.05, val_nulls=0.1):
    k = keys(kt, rng.integers(0, groups, n))
    v = km.payload(rng, vt, n, False)[1]
    cols = [(kt, k, rng.random(n) >= key_nulls) if key_nulls else (kt, k)]
    cols.append((vt, v, rng.random(n) >= val_nulls) if val_nulls else (vt, v))
    return cols



def keys_per_partition(kt, k, valid, bits):
    """Distinct non-NULL keys of every radix partition (the low `bits` bits of the library's hash),
    and the tuples of each."""
    k = np.asarray(k)[np.asarray(valid, dtype=bool)]
    h = hs.key_hash(k, kt != I32).astype(np.uint64) & np.uint64((1 << bits) - 1)
    tuples = np.bincount(h.astype(np.int64), minlength=1 << bits)
    uk = np.unique(k)
    uh = hs.key_hash(uk, kt != I32).astype(np.uint64) & np.uint64((1 << bits) - 1)
    return np.bincount(uh.astype(np.int64), minlength=1 << bits), tuples


# ------------------------------------------------------------------ functions and types
@pytest.mark.gpu
@pytest.mark.parametrize("func", [KEY, STAR, COUNT, SUM, MIN, MAX, "all"])
@pytest.mark.parametrize("kt,vt", [(I32, I64), (I64, I32), (I32, I32)], ids=["k32v64", "k64v32", "k32v32"])
def test_each_function_alone_and_all_together(func, kt, vt):
    rng = rng_for("funcs", func, kt, vt)
    cols = table(rng, 30_000, kt, vt)
    outs = ALL if func == "all" else [o for o in ALL if o[0] == func]
    got, _ = check(agg_plan(cols, outs), what=(func, kt, vt))
    assert got.num_rows == np.unique(cols[0][1][cols[0][2]]).shape[0] + 1


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64], ids=["i32", "i64"])
@pytest.mark.parametrize("nulls", ["some", "none", "only"])
def test_null_key_group(kt, nulls):
    """The NULL group is there, is absent without NULL keys, and can be the only group."""
    rng = rng_for("nullgroup", kt, nulls)
    cols = table(rng, 20_000, kt, I64 if kt == I32 else I32, key_nulls={"some": 0.1, "none": 0.0, "only": 0.5}[nulls])
    if nulls == "only":
        cols[0] = (kt, cols[0][1], np.zeros(20_000, dtype=bool))
    got, ran = check(agg_plan(cols, ALL), log=True, what=(kt, nulls))
    null_keys = [r for r in pl.table_rows(got) if r[0] is None]
    assert len(null_keys) == (0 if nulls == "none" else 1)
    assert got.num_rows == (1 if nulls == "only" else 1000 + (nulls == "some"))
    assert bool(fam(ran, "k_agg_nullkey")) == (nulls != "none")


@pytest.mark.gpu
def test_nullable_values_and_a_group_without_any_value():
    rng = rng_for("allnull")
    cols = table(rng, 40_000, I32, I32, groups=50)
    dead = cols[0][1] == keys(I32, np.array([7]))[0]
    cols[1] = (I32, cols[1][1], cols[1][2] & ~dead)
    got, ran = check(agg_plan(cols, ALL), log=True)
    row = [r for r in pl.table_rows(got) if r[0] == int(keys(I32, np.array([7]))[0])]
    assert len(row) == 1 and row[0][2] == 0 and row[0][3:] == (None, None, None) and row[0][1] > 0
    assert fam(ran, "k_agg_column")


@pytest.mark.gpu
def test_sum_wraps_and_int32_limits():
    n = 9_000
    k = np.repeat(np.arange(3, dtype=np.int32), n // 3)
    big = np.full(n, 2**62 + 12345, dtype=np.int64)
    lim = np.resize(np.array([-2**31, 2**31 - 1, 0, -1], dtype=np.int32), n)
    got, _ = check(agg_plan([(I32, k), (I64, big), (I32, lim)], [(KEY, 0, None), (SUM, 1, I64), (MIN, 2, None), (MAX, 2, None),
                                                               (SUM, 2, I64)]))
    for r in pl.table_rows(got):
        assert r[1] == ((n // 3) * (2**62 + 12345) + 2**63) % 2**64 - 2**63 and r[2] == -2**31 and r[3] == 2**31 - 1


# ------------------------------------------------------------------ carry layouts and refusals
# (key type, value columns as (type, nullable)) -> carry words
LAYOUTS = [
    (I32, [], 0), (I32, [(I32, False)], 1), (I32, [(I64, False)], 2), (I32, [(I32, True)], 2),
    (I32, [(I32, False), (I32, False)], 2), (I32, [(I32, False), (I32, False), (I32, False)], 3),
    (I32, [(I64, False), (I32, False)], 3), (I32, [(I64, True)], 3), (I32, [(I32, True), (I32, False)], 3),
    (I64, [], 0), (I64, [(I32, False)], 1), (I64, [(I64, False)], 2), (I64, [(I32, True)], 2),
    (I64, [(I32, False), (I32, False)], 2),
]
OVER = [
    (I32, [(I64, False), (I64, False)]), (I32, [(I64, True), (I32, False)]), (I32, [(I32, False)] * 4),
    (I32, [(I32, True), (I32, True), (I32, False)]), (I64, [(I64, True)]), (I64, [(I64, False), (I32, False)]),
    (I64, [(I32, False)] * 3),
]


def layout_plan(rng, kt, spec, n=30_000, key_nulls=0.05, groups=700):
    cols = table(rng, n, kt, I32, groups=groups, key_nulls=key_nulls, val_nulls=0)[:1]
    cols += [km.payload(rng, t, n, nl) for t, nl in spec]
    cols.append(km.payload(rng, F64, n, True))          # columns the node does not name may be of any type
    cols.append(km.payload(rng, VC, n, False))
    outs = [(KEY, 0, None), (STAR, 0, I64)]
    for i in range(len(spec)):
        outs += [(COUNT, 1 + i, I64), (SUM, 1 + i, I64), (MIN, 1 + i, None), (MAX, 1 + i, None)]
    return agg_plan(cols, outs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAYOUTS, ids=lambda c: f"k{c[0]}-" + "".join(f"{'q' if t == I64 else 'd'}{'n' if nl else ''}" for t, nl in c[1]))
def test_every_carry_layout(case):
    kt, spec, cw = case
    _, ran = check(layout_plan(rng_for("layout", case), kt, spec), log=True, what=case)
    assert f"k_agg_parts<{1 if kt == I32 else 2},{cw}>" in ran, sorted(ran)
    assert f"k_agg_nullkey<{cw}>" in ran


@pytest.mark.gpu
@pytest.mark.parametrize("case", OVER, ids=lambda c: f"k{c[0]}-" + "".join(f"{'q' if t == I64 else 'd'}{'n' if nl else ''}" for t, nl in c[1]))
def test_over_the_carry_limit_is_unsupported(case):
    with pytest.raises(capi.RjError) as e:
        run(layout_plan(rng_for("over", case), case[0], case[1], n=2_000))
    assert e.value.code == 5 and "carry words" in str(e.value) and f"at most {3 if case[0] == I32 else 2}" in str(e.value)


def _bad(mutate, cols=None):
    rng = rng_for("bad")
    cols = cols or (table(rng, 500, I32, I64) + [km.payload(rng, I32, 500, False)])
    p = agg_plan(cols, ALL)
    mutate(p.nodes[p.root])
    with pytest.raises(capi.RjError) as e:
        run(p)
    return e.value.code


@pytest.mark.gpu
def test_malformed_nodes_are_argument_errors():
    def out(i, f, c, t):
        def m(node):
            node.output_attrs[i] = (pl.agg_out(f, c), t)
        return m
    assert _bad(out(0, KEY, 0, I64)) == 1        # the key is INT32
    assert _bad(out(1, STAR, 0, I32)) == 1       # COUNT(*) is INT64
    assert _bad(out(2, COUNT, 1, I32)) == 1
    assert _bad(out(3, SUM, 2, I32)) == 1        # SUM is INT64 whatever the column is
    assert _bad(out(4, MIN, 1, I32)) == 1        # the column is INT64
    assert _bad(out(5, MAX, 2, I64)) == 1        # the column is INT32
    assert _bad(out(0, 6, 0, I32)) == 1          # unknown function code
    assert _bad(out(0, 255, 0, I32)) == 1
    assert _bad(out(3, SUM, 3, I64)) == 1        # column out of range
    assert _bad(out(0, KEY, 2, I32)) == 1        # RJ_AGG_KEY on another column
    assert _bad(out(1, STAR, 1, I64)) == 1       # COUNT(*) with a column

    def key_attr(node):
        node.data.key_attr = 9
    assert _bad(key_attr) == 1
    # the other kinds keep rejecting encoded values as out of range
    p = og._small()
    p.nodes[p.root].output_attrs[0] = (pl.agg_out(SUM, 0), I32)
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 1


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [F64, VC], ids=["fp64", "varchar"])
@pytest.mark.parametrize("where", ["key", "value"])
def test_fp64_and_varchar_are_unsupported(bad, where):
    rng = rng_for("unsup", bad, where)
    n = 300
    cols = [km.payload(rng, bad, n, False), km.payload(rng, I32, n, False)]
    if where == "key":
        p = agg_plan(cols, [(KEY, 0, bad), (STAR, 0, I64), (SUM, 1, I64)], key_attr=0)
    else:
        p = agg_plan(cols, [(KEY, 1, I32), (COUNT, 0, I64)], key_attr=1)
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 5


@pytest.mark.gpu
def test_empty_child():
    got, _ = run(agg_plan([(I32, np.zeros(0, np.int32)), (I64, np.zeros(0, np.int64))], ALL))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [I32, I64, I64, I64, I64, I64]
    assert all(c.pages.shape[0] == 0 for c in got.columns)


# ------------------------------------------------------------------ group shapes
@pytest.mark.gpu
def test_one_row():
    got, _ = check(agg_plan([(I32, np.array([5], np.int32)), (I64, np.array([-9], np.int64))], ALL))
    assert pl.table_rows(got) == [(5, 1, 1, -9, -9, -9)]


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64], ids=["i32", "i64"])
def test_one_group_of_three_million_rows_is_split_and_merged(kt):
    rng = rng_for("hot", kt)
    n = 3_000_000
    cols = [(kt, keys(kt, np.full(n, 4242))), km.payload(rng, I64 if kt == I32 else I32, n, True)]
    got, ran = check(agg_plan(cols, ALL), log=True)
    assert got.num_rows == 1 and pl.table_rows(got)[0][1] == n
    assert sum(fam(ran, "k_agg_parts").values()) == 1 and sum(fam(ran, "k_agg_emit").values()) == 1


@pytest.mark.gpu
def test_all_distinct_keys():
    rng = rng_for("distinct")
    n = 2_500_000
    cols = [(I32, keys(I32, rng.permutation(n))), km.payload(rng, I64, n, False)]
    got, _ = check(agg_plan(cols, ALL))
    assert got.num_rows == n


@pytest.mark.gpu
def test_zipf_keys():
    rng = rng_for("zipf")
    n = 4_000_000
    z = np.minimum(rng.zipf(1.3, n), 1_000_000)
    cols = [(I32, keys(I32, np.asarray(z, dtype=np.int64))), km.payload(rng, I64, n, True)]
    _, ran = check(agg_plan(cols, ALL), log=True)
    assert fam(ran, "k_agg_parts")


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vspec", [(I32, [(I64, True)]), (I64, [(I32, True)]), (I32, [(I32, False)])], ids=["aos-free3", "k64", "packed"])
def test_table_overflow_rounds_with_one_radix_bit(kt, vspec):
    """Two partitions of 100 K distinct keys each: heavy tasks, each of which sees far more keys than
    its LDS table holds and works them off round by round; all groups meet in the merge table."""
    rng = rng_for("rounds", kt, vspec)
    n = 260_000
    k = np.concatenate([rng.permutation(200_000), rng.integers(0, 200_000, n - 200_000)])
    cols = [(kt, keys(kt, k), rng.random(n) >= 0.01)] + [km.payload(rng, t, n, nl) for t, nl in vspec]
    got, ran = check(agg_plan(cols, ALL), radix_bits=1, rows=True, log=True)
    # every partition is heavy; k_heavy_tasks cuts one of t tuples into exactly ceil(t / JN_HEAVY)
    # tasks, so by pigeonhole some task holds at least distinct / tasks keys — more than the table has
    # entries: it cannot have finished in one round
    distinct, tuples = keys_per_partition(kt, cols[0][1], cols[0][2], 1)
    for d, t in zip(distinct, tuples):
        assert t > JN_HEAVY and d / -(-t // JN_HEAVY) > AGG_CAP, (d, t)
    # ... and the merge table held them all at its first size: one probe, one emit
    assert sum(fam(ran, "k_agg_parts").values()) == 1 and sum(fam(ran, "k_agg_emit").values()) == 1


@pytest.mark.gpu
def test_table_overflow_rounds_in_unsplit_partitions():
    """2^6 partitions of ~1250 distinct keys, below JN_HEAVY tuples: the main workgroups run rounds."""
    rng = rng_for("rounds-main")
    n = 160_000
    k = np.concatenate([rng.permutation(80_000), rng.integers(0, 80_000, n - 80_000)])
    cols = [(I32, keys(I32, k)), km.payload(rng, I32, n, True), km.payload(rng, I32, n, False)]
    outs = ALL + [(SUM, 2, I64), (MAX, 2, None)]
    got, ran = check(agg_plan(cols, outs), radix_bits=6, rows=True, log=True)
    distinct, tuples = keys_per_partition(I32, cols[0][1], np.ones(n, dtype=bool), 6)
    assert got.num_rows == distinct.sum()
    # no partition is split, and most hold more distinct keys than the table has entries (any such
    # partition needs a second round whatever the fill at which a round stops taking keys)
    assert tuples.max() <= JN_HEAVY and (distinct > AGG_CAP).sum() >= 8, (tuples.max(), distinct)
    assert sum(fam(ran, "k_agg_parts").values()) == 1


@pytest.mark.gpu
def test_merge_table_grows_when_heavy_partitions_hold_many_groups():
    """More than 2^20 distinct keys in heavy partitions: the capped merge table overflows and the node
    runs once more with the full bound."""
    rng = rng_for("grow")
    n = 2_300_000
    cols = [(I32, keys(I32, rng.permutation(n))), km.payload(rng, I32, n, False)]
    got, ran = check(agg_plan(cols, [(KEY, 0, None), (STAR, 0, I64), (SUM, 1, I64)]), radix_bits=3, log=True)
    assert got.num_rows == n
    # the launch log shows the second attempt: everything from the partitioning on ran twice
    for f in ("k_agg_merge_init", "k_agg_parts", "k_agg_emit"):
        assert sum(fam(ran, f).values()) == 2, (f, fam(ran, f))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [12, 18])
def test_forced_bit_plans(bits):
    rng = rng_for("bits", bits)
    cols = table(rng, 300_000, I32, I64, groups=40_000)
    check(agg_plan(cols, ALL), radix_bits=bits, rows=True)


# ------------------------------------------------------------------ partitioning inputs
@pytest.mark.gpu
def test_short_pages_and_irregular_inputs():
    """A table whose pages hold fewer rows than they could (decoded by K1), and one of 1 .. 3 rows
    around a page boundary."""
    rng = rng_for("short")
    for n in (1, 2, 1983, 1984, 1985, 1007, 1008, 5_001):
        cols = table(rng, n, I32, I64, groups=13)
        check(agg_plan(cols, ALL), what=n)
    cols = table(rng, 20_000, I64, I32, groups=300, key_nulls=0, val_nulls=0)
    p = agg_plan(cols, ALL)
    # every page cut down to 600 rows: the column is no longer "regular" and goes through the page decode
    # (every other legal layout under an aggregation: tests/test_gpu_layouts.py)
    t = p.inputs[0]
    for ci, (dt, v) in enumerate(cols):
        chunks = [pg.pack_fixed(v[i:i + 600], None, dt) for i in range(0, v.shape[0], 600)]
        t.columns[ci] = pl.Column(dt, np.concatenate(chunks))
    check(p)


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64], ids=["i32", "i64"])
def test_hash_adversarial_keys(kt):
    """Keys chosen through the library's hash so that they share their low hash bits: one partition
    takes them all, its LDS table sees one long collision chain."""
    rng = rng_for("adv", kt)
    n = 150_000
    k = hs.keys_with_hash_bits(5_000, np.int32 if kt == I32 else np.int64, value=0x155, mask=0xFFF, rng=rng)
    kk = k[rng.integers(0, k.shape[0], n)]
    cols = [(kt, kk), km.payload(rng, I64 if kt == I32 else I32, n, True)]
    got, _ = check(agg_plan(cols, ALL), rows=True)
    assert got.num_rows == np.unique(kk).shape[0]


# ------------------------------------------------------------------ nesting
def _abc(rng, n=30_000):
    a = [(I32, keys(I32, rng.integers(0, 2_000, n)), rng.random(n) >= 0.03), km.payload(rng, I64, n, True)]
    b = [(I32, keys(I32, rng.integers(0, 3_000, n // 2)), rng.random(n // 2) >= 0.03), km.payload(rng, I32, n // 2, False)]
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["join", "outer", "full"])
@pytest.mark.parametrize("radix_bits", [0, 4])
def test_agg_over_join_results(kind, radix_bits):
    rng = rng_for("over", kind)
    a, b = _abc(rng)
    p = pl.Plan()
    sa = p.new_scan_node(0, [(0, I32), (1, I64)])
    sb = p.new_scan_node(1, [(0, I32), (1, I32)])
    mk = {"join": p.new_join_node, "outer": p.new_outer_join_node, "full": p.new_full_outer_join_node}[kind]
    j = mk(False, sa, sb, 0, 0, [(0, I32), (1, I64), (3, I32)])
    # (one nullable INT32 column — the optional side's in an outer / full join — is two carry words; the
    # INT64 column rides along unnamed)
    p.root = p.new_agg_node(j, 0, [(KEY, 0, I32), (STAR, 0, I64), (SUM, 2, I64), (COUNT, 2, I64), (MAX, 2, I32)])
    p.new_input(pl.make_table(a))
    p.new_input(pl.make_table(b))
    check(p, radix_bits, what=(kind, radix_bits))


@pytest.mark.gpu
@pytest.mark.parametrize("parent", ["join-key", "join-count", "semi-key", "semi-count", "agg"])
def test_parents_use_an_agg_result(parent):
    rng = rng_for("under", parent)
    a, b = _abc(rng)
    b[1] = (I64, rng.integers(0, 40, b[0][1].shape[0]).astype(np.int64))  # meets the COUNT column
    p = pl.Plan()
    sa = p.new_scan_node(0, [(0, I32), (1, I64)])
    g = p.new_agg_node(sa, 0, [(KEY, 0, I32), (STAR, 0, I64), (MIN, 1, I64)])
    sb = p.new_scan_node(1, [(0, I32), (1, I64)])
    if parent == "join-key":
        p.root = p.new_join_node(True, g, sb, 0, 0, [(0, I32), (1, I64), (2, I64), (4, I64)])
    elif parent == "join-count":
        p.root = p.new_join_node(False, g, sb, 1, 1, [(0, I32), (1, I64), (3, I32)])
    elif parent == "semi-key":
        p.root = p.new_semi_join_node(False, g, sb, 0, 0, [(0, I32), (1, I64), (2, I64)])
    elif parent == "semi-count":
        p.root = p.new_semi_join_node(True, g, sb, 1, 1, [(3, I32), (4, I64)])
    else:  # AGG over AGG: how many keys have each row count, and the largest key among them (the NULL key counts as none)
        p.root = p.new_agg_node(g, 1, [(KEY, 1, I64), (STAR, 0, I64), (MAX, 0, I32), (COUNT, 0, I64)])
    p.new_input(pl.make_table(a))
    p.new_input(pl.make_table(b))
    got, _ = check(p, what=parent)
    assert got.num_rows > 0


# ------------------------------------------------------------------ entry points
@pytest.mark.gpu
def test_resident_tables_and_results_kept_on_the_device():
    rng = rng_for("resident")
    cols = table(rng, 200_000, I32, I64, groups=30_000)
    p = agg_plan(cols, ALL)
    want = _aggref.execute(p)
    ctx = capi.Context()
    try:
        t = ctx.upload(p.inputs[0])
        try:
            for keep in (True, False):
                r = ctx.execute_resident(p, [t], keep_on_device=keep)
                try:
                    if keep:
                        assert all(r.device_pages(c) for c in range(r.num_cols))
                    _aggref.same(r.to_table(), want, keep)
                finally:
                    r.free()
        finally:
            t.release()
    finally:
        ctx.destroy()


@pytest.mark.gpu
def test_multi_device_context_falls_back_to_one_device():
    rng = rng_for("two")
    n = 2 * 1984 * 1007 + 17  # above the sharding cut of a two-device context
    cols = [(I32, keys(I32, rng.integers(0, 500_000, n))), (I32, np.arange(n, dtype=np.int32))]
    p = agg_plan(cols, [(KEY, 0, None), (STAR, 0, I64), (SUM, 1, I64), (MAX, 1, None)])
    ok, why = capi.plan_shardable(p)
    assert not ok and "RJ_NODE_AGG" in why
    got, _ = run(p, devices=[0, 0])
    _aggref.same(got, _aggref.execute(p))


@pytest.mark.gpu
def test_execute_sharded_refuses_agg_plans():
    p = agg_plan(table(rng_for("sh"), 1_000, key_nulls=0, val_nulls=0), ALL)
    ctx = capi.Context(devices=[0, 0])
    try:
        tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
        try:
            with pytest.raises(capi.RjError) as e:
                ctx.execute_sharded(p, tables)
            assert e.value.code == 5 and "RJ_NODE_AGG" in str(e.value)
        finally:
            for row in tables:
                for t in row:
                    t.release()
    finally:
        ctx.destroy()


# ------------------------------------------------------------------ every compiled instantiation
MATRIX = LAYOUTS


@pytest.mark.gpu
def test_every_agg_instantiation_is_driven():
    compiled = {n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(LIB)) if n.split("<")[0] in FAMILIES}
    assert len(compiled) == 7 + 4 + 2 + 1 + 2, sorted(compiled)
    reached = set()
    for case in MATRIX:
        kt, spec, _ = case
        _, ran = check(layout_plan(rng_for("matrix", case), kt, spec, n=8_000), log=True, what=case)
        reached |= {n for n in ran if n.split("<")[0] in FAMILIES}
    assert compiled <= reached, sorted(compiled - reached)
