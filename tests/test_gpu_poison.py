"""Every kernel family on dirty memory: the suite's own cases, in contexts whose block cache fills
every block it hands out and takes back (RJ_DEBUG_POISON, DESIGN.md "Block cache").

Production keeps ONE context for a whole run, so a kernel finds in its buffers whatever an earlier
plan left there; the path-specific GPU tests mostly create a context per case and get fresh driver
memory.  Here nothing is new but the memory: plans, references, exactness and launch-log assertions
are the borrowed tests' own (they are called as they stand, with the knob in the environment while
their contexts are created), so a case that fails here and passes in its home module read a byte
that no memset and no kernel of that plan had written.  Three cases are the home modules' builders at
other sizes, because the originals take the references many seconds: the aggregation's heavy partition
and merge-table growth, and the partitioned VARCHAR-key join with forced collisions; each proves by the
launch log or by the partition sizes that it reaches its path.

Every context the module creates is destroyed by it (test_gpu_result_pages' shared contexts included:
their cache key holds the knob), so the modules collected after this one get contexts of their own.
The long-lived contexts of (g) and (h) are per mode and ordered: those tests are meant to run whole.

Modes: 0x15A (byte 0x5A: neither zero nor a sentinel) and 0x1FF (all-ones: what EMPTY words look
like), both on alloc and on release, one after the other.  RJ_POISON_TEST_MODES=0x100 runs the
module with zeros instead: the first run on a machine, which checks the plumbing alone.

Unwritten bytes of result Page images (slack behind the last row, bitmap bits beyond num_rows) are
not asserted: the strict reader tests/_pagecheck.py defines what a page must hold."""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

import _aggref
import _pagecheck
import test_gpu_agg as ag
import test_gpu_edges as ed
import test_gpu_filter_join as fj
import test_gpu_full_outer_join as fo
import test_gpu_fuzz_mixed as fm
import test_gpu_ingest as ing
import test_gpu_kernel_matrix as km
import test_gpu_outer_join as og
import test_gpu_result_pages as rp
import test_gpu_varchar_keys as vk
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
MODES = [int(m, 0) for m in os.environ.get("RJ_POISON_TEST_MODES", "0x15A,0x1FF").split(",")]
KNOB = "RJ_DEBUG_POISON"


@pytest.fixture(scope="module", params=MODES, ids=[f"{m:#x}" for m in MODES])
def mode(request):
    """module-scoped: every test of one mode runs before the first of the next"""
    return request.param


@pytest.fixture(autouse=True)
def _knob_in_the_environment(mode, monkeypatch):
    """read once per context, when it is created: every context a borrowed test creates has it"""
    monkeypatch.setenv(KNOB, str(mode))
    # test_gpu_result_pages shares one context per configuration (rp.context, which rp.run and three of its
    # tests call): the knob is part of the configuration, so it is part of every key of that cache
    plain_context = rp.context
    monkeypatch.setattr(rp, "context", lambda env=None, **kw: plain_context({**(env or {}), KNOB: str(mode)}, **kw))


@pytest.fixture(scope="module", autouse=True)
def _close_result_page_contexts():
    before = set(rp._contexts)
    yield
    made = [k for k in rp._contexts if k not in before]
    assert all(KNOB in dict(k[0]) for k in made), made  # nothing of this module is left for rp's own tests
    for key in made:
        rp._contexts.pop(key).destroy()


def cases_of(fn):
    """The parameter sets of a borrowed test, from its own parametrize marks: [pytest.param(kwargs)]."""
    cases = [((), {})]
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        assert isinstance(m.args[0], str), (fn.__name__, "argnames given as a list are not handled")
        names = [n.strip() for n in m.args[0].split(",")]
        ids = m.kwargs.get("ids")
        grown = []
        for i, v in enumerate(m.args[1]):
            assert not hasattr(v, "marks"), (fn.__name__, "pytest.param values are not handled")
            tup = tuple(v) if len(names) > 1 else (v,)
            ident = ids(v) if callable(ids) else ids[i] if ids else "-".join(getattr(x, "__name__", str(x)) for x in tup)
            grown += [(parts + (str(ident),), {**kw, **dict(zip(names, tup))}) for parts, kw in cases]
        cases = grown
    return [pytest.param(kw, id="-".join(parts)[:80]) for parts, kw in cases]


def poisoned_context(mode, env=None, **kw):
    return fm.tuned_context({**(env or {}), KNOB: str(mode)}, **kw)


# ------------------------------------------------------------------ the knob itself
def test_the_knob_fills_and_is_off_by_default(mode, monkeypatch):
    p = og._small()
    c = capi.Context()
    try:
        capi.execute(p, c)
        s = c.pool()
        assert s["fills"] > 0 and s["filled_bytes"] >= s["in_use"] + s["cached"] > 0, s
        if mode & 0x100:  # every block was filled when it left and when it came back
            assert s["filled_bytes"] >= 2 * s["cached"], s
    finally:
        c.destroy()
    monkeypatch.delenv(KNOB)
    c = capi.Context()
    try:
        capi.execute(p, c)
        s = c.pool()
        assert s["fills"] == 0 and s["filled_bytes"] == 0 and s["cached"] > 0, s
    finally:
        c.destroy()


# ------------------------------------------------------------------ a. the kernel matrix
@pytest.mark.parametrize("case", km.CASES, ids=[c.id + ("-sharded" if c.ranks > 1 else "") for c in km.CASES])
def test_kernel_matrix_row(mode, case):
    # (Case.knobs travels through km.make_ctx; check_case keeps the row's launch-log assertion)
    km.check_case(dataclasses.replace(case, knobs={**case.knobs, KNOB: str(mode)}))


# ------------------------------------------------------------------ b. semi / anti, outer, full outer
KTS = pytest.mark.parametrize("kt", [I32, I64, F64], ids=["i32", "i64", "f64"])


@KTS
@pytest.mark.parametrize("path", list(fj.PATHS))
@pytest.mark.parametrize("kind", [fj.SEMI, fj.ANTI], ids=["semi", "anti"])
def test_filter_paths(kind, kt, path):
    fj.test_filter_grid(kind, kt, path, build_left=bool((kt + list(fj.PATHS).index(path)) & 1))


@KTS
@pytest.mark.parametrize("path", list(og.PATHS))
def test_outer_paths(kt, path):
    og.test_outer_grid(kt, path, build_left=bool((kt + list(og.PATHS).index(path)) & 1))


@KTS
@pytest.mark.parametrize("path", list(fo.PATHS))
def test_full_outer_paths(kt, path):
    fo.test_full_grid(kt, path, build_left=bool((kt + list(fo.PATHS).index(path)) & 1))


@pytest.fixture
def row_index_launches(monkeypatch):
    """RJ_TUNE_WIDE_CARRY=0 (a row index travels, every column is gathered afterwards), and the launch log
    of every context created meanwhile, merged when the context is destroyed: {kernel family: launches}"""
    monkeypatch.setenv("RJ_TUNE_WIDE_CARRY", "0")
    ran = {}
    init, destroy = capi.Context.__init__, capi.Context.destroy

    def logged_init(self, *a, **kw):
        init(self, *a, **kw)
        if self.group is None:
            self.launch_log(True)

    def logged_destroy(self):
        if self.group is None and getattr(self, "h", None):
            for n, c in km.launched(self).items():
                ran[n.split("<")[0]] = ran.get(n.split("<")[0], 0) + c
        destroy(self)
    monkeypatch.setattr(capi.Context, "__init__", logged_init)
    monkeypatch.setattr(capi.Context, "destroy", logged_destroy)
    return ran


def test_filter_row_index_carry(row_index_launches):
    # (kt + build_left) % 3 == 1: fj.P_WIDE, the preserved payload that would travel as a wide carry
    fj.test_filter_grid(fj.ANTI, I32, "part", True)
    assert row_index_launches.get("k_filter_join") and row_index_launches.get("k_gather"), sorted(row_index_launches)
    assert "k_split_records" not in row_index_launches, sorted(row_index_launches)


def test_outer_row_index_carry(row_index_launches):
    og.test_outer_grid(I32, "part", False)  # O_SPECS[1] / P_SPECS[1]: wide carries on both sides by default
    ran = row_index_launches
    assert ran.get("k_outer_join") and ran.get("k_outer_gather"), sorted(ran)
    assert "k_split_records" not in ran, sorted(ran)


def test_full_outer_row_index_carry(row_index_launches):
    fo.test_full_grid(I32, "part", False)
    ran = row_index_launches
    assert ran.get("k_full_join") and ran.get("k_outer_gather"), sorted(ran)
    assert "k_split_records" not in ran, sorted(ran)


# ------------------------------------------------------------------ c. aggregation
# slots of the merge table's first size: two per heavy tuple, the tuples capped by agg() in rj_exec.hip at first
_CAP = re.search(r"if \(attempt == 0\) heavy_tuples = std::min<uint64_t>\(heavy_tuples, 1u << (\d+)\);",
                 open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_exec.hip")).read())
MERGE_FIRST = 2 << int(_CAP.group(1))


def _layout_id(c):
    return f"k{c[0]}-" + "".join(f"{'q' if t == I64 else 'd'}{'n' if nl else ''}" for t, nl in c[1])


@pytest.mark.parametrize("case", ag.LAYOUTS, ids=_layout_id)
def test_agg_layouts(case):
    kt, spec, cw = case
    _, ran = ag.check(ag.layout_plan(ag.rng_for("layout", case), kt, spec, n=8_000), log=True, what=case)
    assert f"k_agg_parts<{1 if kt == I32 else 2},{cw}>" in ran, sorted(ran)
    assert f"k_agg_nullkey<{cw}>" in ran


@pytest.mark.parametrize("kw", cases_of(ag.test_table_overflow_rounds_with_one_radix_bit))
def test_agg_table_overflow_rounds_in_heavy_tasks(kw):
    ag.test_table_overflow_rounds_with_one_radix_bit(**kw)


def test_agg_table_overflow_rounds_in_unsplit_partitions():
    ag.test_table_overflow_rounds_in_unsplit_partitions()


def test_agg_heavy_partition_meets_in_the_merge_table():
    """One key above JN_HEAVY tuples: its partition is cut into tasks, whose partial groups meet in the merge
    table (entries that k_agg_merge_init has to have written); 3 000 other groups around it."""
    rng = ag.rng_for("poison-heavy")
    n_hot, n = ag.JN_HEAVY + 1_111, ag.JN_HEAVY + 1_111 + 9_000
    k = np.concatenate([np.full(n_hot, 4242), rng.integers(0, 3_000, n - n_hot)])[rng.permutation(n)]
    cols = [(I32, ag.keys(I32, k), rng.random(n) >= 0.02), km.payload(rng, I64, n, True)]
    got, ran = ag.check(ag.agg_plan(cols, ag.ALL), radix_bits=2, rows=True, log=True)
    _, tuples = ag.keys_per_partition(I32, cols[0][1], cols[0][2], 2)
    assert tuples.max() > ag.JN_HEAVY > np.sort(tuples)[-2], tuples  # one split partition, three whole ones
    assert sum(ag.fam(ran, "k_agg_merge_init").values()) == 1 and sum(ag.fam(ran, "k_agg_parts").values()) == 1


def test_agg_merge_table_grows():
    """More distinct keys in heavy partitions than the merge table's first size has slots (pigeonhole: it
    overflows), the fewest rows with which that is certain: the node runs once more with the full bound,
    over arrays that the first attempt has written.  (Fewer rows would have to rely on a walk of
    AGG_MERGE_WALK = 4096 occupied slots turning up, which at a fill of 98 % is likely and not certain.
    0.4 s on an MI355X.)"""
    assert MERGE_FIRST == 1 << 21
    rng = ag.rng_for("poison-grow")
    n = MERGE_FIRST + 1_024
    cols = [(I32, ag.keys(I32, rng.permutation(n))), km.payload(rng, I32, n, False)]
    got, ran = ag.check(ag.agg_plan(cols, [(ag.KEY, 0, None), (ag.STAR, 0, I64), (ag.SUM, 1, I64)]), radix_bits=3, log=True)
    assert got.num_rows == n and n // 8 > 2 * ag.JN_HEAVY  # (eight partitions, every one of them heavy)
    for f in ("k_agg_merge_init", "k_agg_parts", "k_agg_emit"):
        assert sum(ag.fam(ran, f).values()) == 2, (f, ag.fam(ran, f))


# ------------------------------------------------------------------ d. result-page writers
def _borrowed(fn):
    return pytest.mark.parametrize("kw", cases_of(fn))


@_borrowed(rp.test_streams_without_nulls)
def test_pages_streams_without_nulls(kw):
    rp.test_streams_without_nulls(**kw)


def test_pages_streams_whose_last_pages_differ():
    rp.test_int32_and_int64_streams_whose_last_pages_differ()


@_borrowed(rp.test_nullable_columns)
def test_pages_nullable_columns(kw):
    rp.test_nullable_columns(**kw)


@_borrowed(rp.test_nullable_agg_outputs)
def test_pages_nullable_agg_outputs(kw):
    rp.test_nullable_agg_outputs(**kw)


def test_pages_nullable_columns_partitioned_and_gathered():
    rp.test_nullable_columns_partitioned_and_gathered()


@_borrowed(rp.test_varchar_string_lengths)
def test_pages_varchar_string_lengths(kw):
    rp.test_varchar_string_lengths(**kw)


@_borrowed(rp.test_varchar_equal_strings_that_fill_a_page_exactly)
def test_pages_varchar_equal_strings_that_fill_a_page_exactly(kw):
    rp.test_varchar_equal_strings_that_fill_a_page_exactly(**kw)


@_borrowed(rp.test_varchar_null_arrives_at_the_full_page)
def test_pages_varchar_null_arrives_at_the_full_page(kw):
    rp.test_varchar_null_arrives_at_the_full_page(**kw)


@_borrowed(rp.test_varchar_chunk_edges)
def test_pages_varchar_chunk_edges(kw):
    rp.test_varchar_chunk_edges(**kw)


@_borrowed(rp.test_varchar_long_string_at_a_chunk_edge)
def test_pages_varchar_long_string_at_a_chunk_edge(kw):
    rp.test_varchar_long_string_at_a_chunk_edge(**kw)


@_borrowed(rp.test_varchar_all_null_column_at_the_largest_page)
def test_pages_varchar_all_null_column_at_the_largest_page(kw):
    rp.test_varchar_all_null_column_at_the_largest_page(**kw)


def test_pages_result_kept_on_the_device():
    rp.test_result_kept_on_the_device()


def test_pages_two_ranks_concatenated():
    rp.test_two_ranks_pages_concatenated()


def test_pages_group_context_concatenates_its_ranks():
    rp.test_group_context_concatenates_its_ranks_pages()


def test_pages_root_without_rows():
    rp.test_root_without_rows_has_no_pages()


# ------------------------------------------------------------------ e. VARCHAR and ingest
def test_varchar_gather_and_encode_on_the_device(monkeypatch):
    monkeypatch.setenv("RJ_TUNE_VARCHAR_DEV", "1")
    og.test_varchar_payload_on_the_preserved_side(0)
    og.test_varchar_payload_on_the_preserved_side(4)


@pytest.mark.parametrize("build_left", [True, False])
def test_varchar_keys_with_forced_collisions_small_build(build_left):
    vk.test_varchar_keys_small_build(build_left, {"RJ_DEBUG_VKEY_HASH_BITS": "6"})


def test_varchar_keys_with_forced_collisions_partitioned():
    """vk.test_varchar_keys_partitioned's plan with a build side just above two LDS tables, the fewest rows
    that leave the broadcast kernels with a margin (its 60 000 x 150 000 rows join 3.6 M pairs of empty
    strings, which takes the reference 20 s); a 10-bit hash makes most joined pairs collisions."""
    rng = np.random.default_rng(61)
    nb, npr = 2 * km.JN_RMAX + 1_000, 20_000
    bt = pl.make_table([(pl.VARCHAR, vk.words(rng, nb, 7_000)), (pl.VARCHAR, [b"p%d" % i for i in range(nb)])])
    pt = pl.make_table([(pl.VARCHAR, vk.words(rng, npr, 8_000)), (I32, np.arange(npr, dtype=np.int32))])
    c = vk.ctx_with({"RJ_DEBUG_VKEY_HASH_BITS": "10"})
    try:
        c.launch_log(True)
        got = vk.check(c, vk.two(bt, pt, True, [(0, pl.VARCHAR), (1, pl.VARCHAR)], [(0, pl.VARCHAR), (1, I32)],
                                 [(1, pl.VARCHAR), (3, I32), (0, pl.VARCHAR)]))
        assert _pagecheck.same_as(_pagecheck.check_table(got), pl.decode_table(got))
        ran = {n.split("<")[0] for n in km.launched(c)}
    finally:
        capi.destroy_context(c)
    assert {"k_join", "k_vc_hash", "k_vc_verify", "k_vc_compact"} <= ran and "k_join_bcast" not in ran, sorted(ran)


@pytest.fixture(scope="module")
def ingest_ctx(mode):
    c = poisoned_context(mode)
    yield c
    c.destroy()


@pytest.mark.parametrize("seed", [0, 1, 6])  # three type lists, VARCHAR and FP64 among them; 0 has long strings
def test_from_csv_with_filters_and_like(ingest_ctx, seed):
    """pages byte for byte the oracle's, unfiltered and under three random filters (LIKE among their terms)"""
    ing.test_random_tables_and_filters(ingest_ctx, seed)


def test_like_on_the_device(ingest_ctx):
    ing.test_like_on_the_device(ingest_ctx)


# ------------------------------------------------------------------ f. the tagged table
def test_tagged_table():
    ed.test_tagged_table_path_forced_bits(16, I64)


# ------------------------------------------------------------------ g. long-lived contexts
class Lived:
    """a context that lives as long as the module runs one mode, and what its cache held when it was new"""

    def __init__(self, mode):
        self.ctx = poisoned_context(mode)
        self.in_use0 = self.ctx.pool()["in_use"]


@pytest.fixture(scope="module")
def lived(mode):
    ctxs = {name: Lived(mode) for name in ("forward", "reverse", "mid", "errors")}
    yield ctxs
    for c in ctxs.values():
        c.ctx.destroy()


SEEDS = list(range(40))


@pytest.mark.parametrize("seed", SEEDS)
def test_mixed_plans_on_one_context(lived, seed):
    fm.same(capi.execute(fm.case(seed)[0], lived["forward"].ctx), seed, what="forward")


@pytest.mark.parametrize("seed", SEEDS[::-1])
def test_mixed_plans_in_reverse_on_a_second_context(lived, seed):
    fm.same(capi.execute(fm.case(seed)[0], lived["reverse"].ctx), seed, what="reverse")


@functools.lru_cache(maxsize=None)
def mid_order():
    size = {s: sum(t.num_rows for t in fm.case(s, "mid")[0].inputs) for s in fm.MID}
    return sorted(fm.MID, key=lambda s: -size[s])


@pytest.mark.parametrize("rank", range(len(fm.MID)))
def test_mid_plans_largest_first(lived, rank):
    """best-fit reuse then hands the large blocks of the early plans, dirty, to the small requests of the later ones"""
    seed = mid_order()[rank]
    fm.same(capi.execute(fm.case(seed, "mid")[0], lived["mid"].ctx), seed, "mid", what=f"rank {rank}")


# ------------------------------------------------------------------ h. error paths in between
def _argument_error():
    p = og._small(seed=1)
    p.nodes[p.root].output_attrs.append((9, I32))  # attr out of range
    return p, 1


def _unsupported():
    return og._vc_plan(100, key_vc=True), 5


def _scan_type_mismatch():
    p = og._small(seed=2)
    p.nodes[0].output_attrs[0] = (0, I64)  # the left scan declares INT64 for its INT32 key column
    return p, 1


def _key_types_differ(kind):
    rng = og.rng_for("poison-mismatch", kind)
    no, npr = 6_000, 2_000
    ocols = [(I64, og.keys(I64, rng.integers(0, 300, no)))] + og.payload(rng, no, [(I64, True)])
    pcols = [(I32, og.keys(I32, rng.integers(0, 600, npr)), rng.random(npr) >= 0.05)] + og.payload(rng, npr, [(I32, True)])
    return og.outer_plan(ocols, pcols, True, kind=kind)


def test_failed_executes_between_good_ones(lived):
    """A failed execute leaves nothing behind: the next plan is exact, and when every result and table is
    freed the cache holds as many bytes in use as before.  Keys of two types are no failure: OUTER pads
    every row, JOIN has no rows; a type mismatch that does fail is a scan that declares another type than
    its column has, an argument error found after the uploads were started."""
    L = lived["errors"]
    c = L.ctx
    good = [3, 17, 5, 29]

    def exact(seed, what):
        fm.same(capi.execute(fm.case(seed)[0], c), seed, what=what)

    exact(good[0], "before")
    for i, make in enumerate((_argument_error, _unsupported, _scan_type_mismatch)):
        p, code = make()
        with pytest.raises(capi.RjError) as e:
            capi.execute(p, c)
        assert e.value.code == code, (make.__name__, str(e.value))
        exact(good[i + 1], f"after {make.__name__}")
        assert c.pool()["in_use"] == L.in_use0, (make.__name__, c.pool())
    # key types that differ, on resident tables with the result kept on the device
    for kind, rows in (("outer", 2_000), ("inner", 0)):
        p = _key_types_differ(kind)
        tables = [c.upload(t) for t in p.inputs]
        try:
            r = c.execute_resident(p, tables, keep_on_device=True)
            try:
                got, want = r.to_table(), _aggref.execute(p)
                assert got.num_rows == want.num_rows == rows, (kind, got.num_rows, want.num_rows)
                assert pl.canonical_rows(got) == pl.canonical_rows(want), kind
            finally:
                r.free()
        finally:
            for t in tables:
                t.release()
    exact(good[0], "after the key type mismatch")
    assert c.pool()["in_use"] == L.in_use0, c.pool()


def test_long_lived_contexts_leak_nothing(lived):
    """closes (g) and (h): every result freed, every table released — the cache has all its blocks back"""
    for name, L in lived.items():
        s = L.ctx.pool()
        assert s["in_use"] == L.in_use0, (name, s)
        L.ctx.upload(pl.make_table([(I32, np.arange(10, dtype=np.int32))])).release()  # (run alone, it has not allocated yet)
        s = L.ctx.pool()
        assert s["in_use"] == L.in_use0 and s["fills"] > 0, (name, s)  # the knob reached this context
