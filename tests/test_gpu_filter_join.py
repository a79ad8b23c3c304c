"""Semi and anti joins (RJ_NODE_SEMI / RJ_NODE_ANTI) on the device against a numpy reference
(tests/_filterref.py: np.isin over key bit patterns with the NULL, NaN and type rules of
include/rj.h), and tied to the pinned C oracle by two identities:
  * semi(P, B) = P inner-joined with distinct(B.key), projected to P's columns (the oracle);
  * semi(P, B) ⊎ anti(P, B) = P as multisets.

Three device paths: broadcast (a filter side of at most JN_RMAX rows, k_filter_bcast), partitioned
(k_filter_join, with a preserved partition above JN_HEAVY tuples that is split into heavy tasks,
and k_filter_nullkeys for the rows ANTI keeps although the first radix pass drops them), and
partitioned with forced radix bits so that a partition holds more distinct filter keys than one
LDS set (several set rounds).  test_every_filter_instantiation_is_driven runs MATRIX with the launch
log on and checks it against the compiled kernel handles (tests/_elfsyms.py)."""
import os
import zlib

import numpy as np
import pytest

import _elfsyms
import _filterref
import _oracle
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import plan as pl
from test_gpu_sharded import combine

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
SEMI, ANTI = pl.NODE_SEMI, pl.NODE_ANTI
JN_RMAX, JN_HEAVY = 4096, 65536
FAMILIES = ("k_filter_bcast", "k_filter_join", "k_filter_nullkeys")
LIB = km.LIB

# path -> (filter rows, preserved rows, hot preserved tuples, forced radix bits)
PATHS = {
    "bcast": (3_000, 20_000, 0, 0),
    "part": (24_000, 30_000, JN_HEAVY + 3_210, 0),
    "overflow": (40_000, 30_000, 0, 2),  # 4 partitions of ~10 K distinct filter keys: several set rounds
}


def keys(kt, k):
    return km.key_values(kt, np.asarray(k))


def sides(kt, path, rng, fnull=True, pnull=True, hot_in_filter=True):
    """-> (filter keys, filter valid, preserved keys, preserved valid): duplicates on both sides,
    about half of the preserved keys without partner, the type's special keys on both sides."""
    nf, npr, hot, _ = PATHS[path]
    dom = max(nf // 2, 10)
    fk = list(rng.integers(0, dom, nf - 40))
    pk = list(rng.integers(0, 2 * dom, npr))
    h = 3 * dom  # a hot preserved key: one partition above JN_HEAVY tuples
    pk += [h] * hot
    if hot_in_filter:
        fk += [h, h]
    fkv, pkv = keys(kt, fk), keys(kt, pk)
    sp = km.SPECIAL_KEYS[kt]
    fkv = np.concatenate([fkv, sp[1:], sp[2:4]])  # (F64: no NaN in the filter but -0.0, +-inf, subnormals)
    pkv = np.concatenate([pkv, sp, sp])
    fv = rng.random(fkv.shape[0]) >= (0.03 if fnull else 0.0)
    pv = rng.random(pkv.shape[0]) >= (0.03 if pnull else 0.0)
    pf, pp = rng.permutation(fkv.shape[0]), rng.permutation(pkv.shape[0])
    return fkv[pf], fv[pf], pkv[pp], pv[pp]


def filter_plan(kind, kt, fk, fv, pk, pv, ppay, build_left=True, key_out=True, pkt=None):
    """Scan(filter: key, INT32 payload) (SEMI|ANTI) Scan(preserved: key, *ppay) with every
    preserved column out (the key only if key_out)."""
    fcols = [(kt, fk, fv), (I32, np.arange(fk.shape[0], dtype=np.int32))]
    pcols = [(kt if pkt is None else pkt, pk, pv)] + list(ppay)
    lcols, rcols = (fcols, pcols) if build_left else (pcols, fcols)
    p = pl.Plan()
    ls = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
    rs = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])
    base = len(lcols) if build_left else 0
    outs = [(base + i, c[0]) for i, c in enumerate(pcols) if i > 0 or key_out]
    mk = p.new_semi_join_node if kind == SEMI else p.new_anti_join_node
    p.root = mk(build_left, ls, rs, 0, 0, outs)
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(rcols))
    return p


def make_ctx(radix_bits=0, devices=None):
    kw = dict(radix_bits=radix_bits)
    if devices:
        kw["devices"] = devices
    return capi.Context(**kw)


def run(p, radix_bits=0, devices=None, log=False):
    ctx = make_ctx(radix_bits, devices)
    try:
        if log:
            ctx.launch_log(True)
        got = capi.execute(p, ctx)
        ran = km.launched(ctx) if log else {}
    finally:
        ctx.destroy()
    return got, ran


def same(got, want, what=""):
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    if any(c.type == VC for c in want.columns):
        assert pl.canonical_rows(got) == pl.canonical_rows(want), what
    elif want.columns:
        assert pl.table_digest(got) == pl.table_digest(want), what


def check(p, radix_bits=0, log=False, what=""):
    got, ran = run(p, radix_bits, log=log)
    same(got, _filterref.execute(p), what)
    return got, ran


def payload(rng, n, spec):
    return [km.payload(rng, t, n, nl) for t, nl in spec]


def rng_for(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


# ------------------------------------------------------------------ the main grid
P_NONE = []
P_NULLABLE_WIDE = [(I32, True), (I64, True)]      # nullable + 64-bit payloads (row index + gather)
P_WIDE = [(I64, False), (I32, False)]             # a wide carry that travels with the key
P_VC = [(VC, False), (F64, True)]                 # a VARCHAR payload (row ids) + a nullable FP64


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("kt", [I32, I64, F64], ids=["i32", "i64", "f64"])
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
@pytest.mark.parametrize("build_left", [True, False], ids=["fl", "fr"])
def test_filter_grid(kind, kt, path, build_left):
    rng = rng_for(kind, kt, path, build_left)
    fk, fv, pk, pv = sides(kt, path, rng)
    spec = (P_NULLABLE_WIDE, P_WIDE, P_VC)[(kt + int(build_left)) % 3]
    p = filter_plan(kind, kt, fk, fv, pk, pv, payload(rng, pk.shape[0], spec), build_left)
    check(p, PATHS[path][3], what=(kind, kt, path, build_left))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
def test_heavy_partition_without_filter_keys(kind):
    """The hot preserved partition has no filter tuple: k_heavy_tasks leaves it to the main pass."""
    rng = rng_for("heavy-empty", kind)
    fk, fv, pk, pv = sides(I32, "part", rng, hot_in_filter=False)
    p = filter_plan(kind, I32, fk, fv, pk, pv, payload(rng, pk.shape[0], [(I32, False)]))
    check(p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
def test_duplicate_heavy_filter_side_fits_one_set(kind):
    """200 K filter tuples over 3 K distinct keys in ONE forced partition: duplicates collapse."""
    rng = rng_for("dups", kind)
    fk = keys(I64, rng.integers(0, 3_000, 200_000))
    pk = keys(I64, rng.integers(0, 6_000, 50_000))
    p = filter_plan(kind, I64, fk, np.ones(fk.shape[0], bool), pk, np.ones(pk.shape[0], bool),
                    payload(rng, pk.shape[0], [(I32, False)]))
    check(p, radix_bits=1)


# ------------------------------------------------------------------ edge cases
def _small(kind, kt=I32, nf=500, npr=2_000, pkt=None, seed=0):
    rng = rng_for("small", kind, kt, nf, npr, pkt, seed)
    fk = keys(kt, rng.integers(0, 300, nf))
    pk = keys(kt if pkt is None else pkt, rng.integers(0, 600, npr))
    pv = rng.random(npr) >= 0.05
    return filter_plan(kind, kt, fk, np.ones(nf, bool), pk, pv, payload(rng, npr, [(I32, True)]), pkt=pkt)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
@pytest.mark.parametrize("radix_bits", [0, 5])
def test_empty_filter_side(kind, radix_bits):
    p = _small(kind, nf=0)
    got, _ = check(p, radix_bits)
    assert got.num_rows == (0 if kind == SEMI else 2_000)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
def test_empty_preserved_side(kind):
    got, _ = check(_small(kind, npr=0))
    assert got.num_rows == 0 and [c.type for c in got.columns] == [I32, I32]
    assert all(c.pages.shape[0] == 0 for c in got.columns)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
@pytest.mark.parametrize("radix_bits", [0, 5])
def test_key_type_mismatch(kind, radix_bits):
    """The filter key is INT64, the preserved key INT32: no row matches."""
    p = _small(kind, kt=I64, pkt=I32, nf=6_000)
    got, _ = check(p, radix_bits)
    assert got.num_rows == (0 if kind == SEMI else 2_000)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
def test_varchar_key_is_unsupported(kind):
    p = pl.Plan()
    a = p.new_scan_node(0, [(0, VC), (1, I32)])
    b = p.new_scan_node(1, [(0, VC)])
    mk = p.new_semi_join_node if kind == SEMI else p.new_anti_join_node
    p.root = mk(False, a, b, 0, 0, [(1, I32)])
    p.new_input(pl.make_table([(VC, [b"a", b"b", None]), (I32, np.arange(3, dtype=np.int32))]))
    p.new_input(pl.make_table([(VC, [b"a", b"c"])]))
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 5  # RJ_ERR_UNSUPPORTED


@pytest.mark.gpu
def test_filter_side_column_in_output_is_an_argument_error():
    p = _small(SEMI)
    p.nodes[p.root].output_attrs.append((1, I32))  # column 1 of the left (filter) child
    with pytest.raises(capi.RjError) as e:
        run(p)
    assert e.value.code == 1  # RJ_ERR_ARG


# ------------------------------------------------------------------ nesting
def _three_tables(rng, n=30_000):
    a = keys(I32, rng.integers(0, 20_000, n))
    b = keys(I32, rng.integers(0, 20_000, n // 2))
    c = keys(I32, rng.integers(0, 40_000, n))
    return [pl.make_table([(I32, a, rng.random(n) >= 0.02), (I64, rng.integers(-9, 9, n))]),
            pl.make_table([(I32, b), (I32, np.arange(n // 2, dtype=np.int32))]),
            pl.make_table([(I32, c), (F64, rng.standard_normal(n))])]


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_semi_under_inner_join(radix_bits):
    rng = rng_for("nest1")
    p = pl.Plan()
    for t in _three_tables(rng):
        p.new_input(t)
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    b = p.new_scan_node(1, [(0, I32)])
    c = p.new_scan_node(2, [(0, I32), (1, F64)])
    s = p.new_semi_join_node(False, a, b, 0, 0, [(0, I32), (1, I64)])  # rows of a with a partner in b
    p.root = p.new_join_node(True, s, c, 0, 0, [(0, I32), (1, I64), (3, F64)])
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_inner_join_as_filter_side(radix_bits):
    rng = rng_for("nest2")
    p = pl.Plan()
    for t in _three_tables(rng):
        p.new_input(t)
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    b = p.new_scan_node(1, [(0, I32), (1, I32)])
    c = p.new_scan_node(2, [(0, I32), (1, F64)])
    j = p.new_join_node(True, b, c, 0, 0, [(0, I32), (3, F64)])
    p.root = p.new_anti_join_node(False, a, j, 0, 0, [(0, I32), (1, I64)])  # filter = the join (right)
    check(p, radix_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("radix_bits", [0, 6])
def test_anti_over_semi(radix_bits):
    rng = rng_for("nest3")
    p = pl.Plan()
    for t in _three_tables(rng):
        p.new_input(t)
    a = p.new_scan_node(0, [(0, I32), (1, I64)])
    b = p.new_scan_node(1, [(0, I32)])
    c = p.new_scan_node(2, [(0, I32)])
    s = p.new_semi_join_node(True, b, a, 0, 0, [(1, I32), (2, I64)])
    p.root = p.new_anti_join_node(True, c, s, 0, 0, [(2, I64), (1, I32)])
    check(p, radix_bits)


# ------------------------------------------------------------------ multi-device contexts
def _big_plan(kind):
    rng = rng_for("big", kind)
    n = 2 * 1984 * 1007 + 17  # above the sharding cut of a two-device context (ROWS32 * ROWS64 per device)
    pk = keys(I32, rng.integers(0, 3_000_000, n))
    fk = keys(I32, rng.integers(0, 3_000_000, 1_000_000))
    return filter_plan(kind, I32, fk, np.ones(fk.shape[0], bool), pk, np.ones(n, bool),
                       [(I32, np.arange(n, dtype=np.int32))])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SEMI, ANTI], ids=["semi", "anti"])
def test_multi_device_context_falls_back_to_one_device(kind):
    p = _big_plan(kind)
    ok, why = capi.plan_shardable(p)
    assert not ok and ("semi" if kind == SEMI else "anti") in why
    got, _ = run(p, devices=[0, 0])
    same(got, _filterref.execute(p))


@pytest.mark.gpu
def test_execute_sharded_refuses_filter_plans():
    p = _small(ANTI)
    ctx = make_ctx(devices=[0, 0])
    try:
        tables = [[ctx.lane(d).upload(t) for t in p.inputs] for d in range(2)]
        try:
            with pytest.raises(capi.RjError) as e:
                ctx.execute_sharded(p, tables)
            assert e.value.code == 5 and "anti" in str(e.value)
        finally:
            for row in tables:
                for t in row:
                    t.release()
    finally:
        ctx.destroy()


# ------------------------------------------------------------------ identities with the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, F64], ids=["i32", "f64"])
@pytest.mark.parametrize("path", ["bcast", "part"])
def test_semi_is_inner_join_with_distinct_filter_keys(kt, path):
    rng = rng_for("ident1", kt, path)
    fk, fv, pk, pv = sides(kt, path, rng)
    pay = payload(rng, pk.shape[0], [(I64, True)])
    p = filter_plan(SEMI, kt, fk, fv, pk, pv, pay)
    got, _ = run(p)
    # distinct usable filter keys, inner-joined by the oracle
    bits, ok = _filterref._usable_keys((kt, fk, fv))
    d = np.unique(bits[ok])
    dk = d.view(np.float64) if kt == F64 else d.astype(km.NP_OF[kt])
    q = pl.Plan()
    ps = q.new_scan_node(0, [(0, kt), (1, I64)])
    ds = q.new_scan_node(1, [(0, kt)])
    q.root = q.new_join_node(False, ps, ds, 0, 0, [(0, kt), (1, I64)])
    q.new_input(pl.make_table([(kt, pk, pv)] + pay))
    q.new_input(pl.make_table([(kt, dk)]))
    want = _oracle.execute(q)
    assert got.num_rows == want.num_rows
    assert pl.table_digest(got) == pl.table_digest(want)


@pytest.mark.gpu
@pytest.mark.parametrize("kt", [I32, I64, F64], ids=["i32", "i64", "f64"])
@pytest.mark.parametrize("path", list(PATHS))
def test_semi_and_anti_partition_the_preserved_side(kt, path):
    rng = rng_for("ident2", kt, path)
    fk, fv, pk, pv = sides(kt, path, rng)
    pay = payload(rng, pk.shape[0], [(I32, True)])
    dig = []
    for kind in (SEMI, ANTI):
        got, _ = run(filter_plan(kind, kt, fk, fv, pk, pv, pay), PATHS[path][3])
        dig.append(pl.table_digest(got))
    whole = pl.make_table([(kt, pk, pv)] + pay)
    assert combine(dig) == pl.table_digest(whole)


# ------------------------------------------------------------------ every compiled instantiation
# (kind, key type, preserved payload, key out, nullable preserved keys, path).  ANTI rows reach
# k_filter_nullkeys on the partitioned path (NULL keys, or FP64 keys that may be NaN); a nullable
# key column an ANTI join outputs travels as a carry, so the rows that must reach the carry-less
# instantiations of one key word output nothing or non-nullable keys.
def _matrix():
    kw1 = [([], False, True), ([(I32, False)], False, True), ([(I64, False)], False, True),
           ([(I64, True)], False, True), ([], True, False)]
    kw2 = [([], True, False), ([(I32, False)], True, False), ([(I64, False)], True, False)]
    rows = []
    for path in ("bcast", "part"):
        for pay, key_out, pnull in kw1:
            rows.append((ANTI, I32, pay, key_out, pnull, path))
        for pay, key_out, pnull in kw2:
            rows.append((ANTI, F64, pay, key_out, pnull, path))
        rows.append((SEMI, I64, [(VC, False)], True, True, path))
    return rows


MATRIX = _matrix()


def run_matrix_row(row):
    kind, kt, pay, key_out, pnull, path = row
    rng = rng_for("matrix", row)
    fk, fv, pk, pv = sides(kt, path, rng, pnull=pnull)
    p = filter_plan(kind, kt, fk, fv, pk, pv, payload(rng, pk.shape[0], pay), key_out=key_out)
    _, ran = check(p, PATHS[path][3], log=True, what=row)
    return ran


def compiled_filter_kernels():
    return sorted(n for n in map(_elfsyms.short_name, _elfsyms.kernel_handles(LIB)) if n.split("<")[0] in FAMILIES)


@pytest.mark.gpu
def test_every_filter_instantiation_is_driven():
    compiled = set(compiled_filter_kernels())
    assert len(compiled) == 21, sorted(compiled)
    reached = set()
    for row in MATRIX:
        reached |= {n for n in run_matrix_row(row) if n.split("<")[0] in FAMILIES}
    assert compiled <= reached, sorted(compiled - reached)
