"""Every writer of result pages at the fills where it switches branches, held to the page format by
the strict reader tests/_pagecheck.py (tests/test_pagecheck.py pins that reader on the CPU).

Every case runs through the C-ABI; every result column goes through check_column, has to decode to what
pyrj.pages decodes, and the rows of the strict decode have to equal the reference result of the plan
(tests/_aggref.py; the C oracle for inner joins).  The launch log names the kernel that wrote the pages:
k_finish_streams / k_finish_pages (streams without NULLs, written in place by the probe, split out of
wide carries, or gathered by k_gather), k_encode_nullable<4|8> (columns with NULLs: nullable sources,
the padded side of OUTER / FULL, and behind k_agg_column<4|8> the SUM / MIN / MAX of groups without a
value), and k_vc_walk / k_vc_encode of the device VARCHAR encoder; the host VARCHAR encoder launches
nothing, which the log shows as well.

Result sizes are exact: unique build keys, and a probe side that hits each of them once.

Where a pattern of NULLs or strings is meant for certain ROWS OF THE RESULT, the input is laid out
through the inverse of the order in which the broadcast probe kernels write their rows, and the decoded
result has to show the pattern where it was meant (the validity of the column row by row; the row ids of
a VARCHAR case in ascending order).  That order: a workgroup takes a chunk of JN_THREADS * JN_SPT probe
rows, thread t holding the rows j * JN_THREADS + t, and writes them wave by wave, inside a wave by j,
inside a j by lane (k_join_bcast in rj_bcast.hip, outer_emit in rj_outer_util.hpp).  It is probe order up to JN_THREADS
rows only, and it is fixed as long as the probe side is one chunk, which every placed case is.  Not
placed, and said so where they are run:
  - RJ_NODE_AGG outputs: the groups come out in the order of the aggregation's hash table;
  - the partitioned kernels (radix_bits=3) and the two-rank contexts: rows come out by partition / rank;
  - VARCHAR cases of more than one chunk of rows, which hold equal rows or need no position.
Those assert format, content, counts, and page boundaries that do not depend on the order."""
import os
import re

import numpy as np
import pytest

import _aggref
import _oracle
import _pagecheck as pc
import test_agg_plan as ap
import test_gpu_fuzz_mixed as fm
import test_gpu_kernel_matrix as km
from pyrj import capi
from pyrj import plan as pl

pytestmark = pytest.mark.gpu

I32, I64, F64, VC = pl.INT32, pl.INT64, pl.FP64, pl.VARCHAR
NPT = {I32: np.int32, I64: np.int64, F64: np.float64}
_HPP = open(os.path.join(os.path.dirname(km.LIB), "csrc", "rj_device.hpp")).read()
ROWS32, ROWS64, VC_CHUNK = (int(re.search(r"constexpr uint32_t %s\s*=\s*(\d+);" % name, _HPP).group(1))
                            for name in ("ROWS32", "ROWS64", "VC_CHUNK"))
JN_THREADS, JN_SPT = (int(re.search(r"#define RJ_%s\s+(\d+)" % name, _HPP).group(1)) for name in ("JN_THREADS", "JN_SPT"))
JN_SUB = JN_THREADS * JN_SPT
RF = {4: ROWS32, 8: ROWS64}
PS = 8192
ROWIDX = {"RJ_TUNE_WIDE_CARRY": "0"}  # a row index travels, every column is gathered afterwards
VDEV = {"RJ_TUNE_VARCHAR_DEV": "1"}   # every VARCHAR result column is encoded on the device


def test_constants_read_from_the_header():
    assert (ROWS32, ROWS64) == (km.ROWS32, km.ROWS64) == (1984, 1007) and VC_CHUNK == 512
    assert (JN_THREADS, JN_SPT) == (512, 8)


def probe_order(n):
    """order[i]: the probe row that the broadcast probe kernels write as result row i, when each of
    the first n probe rows emits one row and the probe side is one chunk (see the module's docstring)"""
    assert n <= JN_SUB, n
    r = np.arange(n)
    return np.lexsort((r, r // JN_THREADS, (r % JN_THREADS) // 64))


def in_probe_rows(by_result_row):
    """lay out what is meant for result row i at the probe row that ends up there"""
    a = np.asarray(by_result_row)
    out = np.empty_like(a)
    out[probe_order(a.shape[0])] = a
    return out


def test_probe_order_is_probe_order_up_to_a_workgroup_of_rows():
    assert probe_order(JN_THREADS).tolist() == list(range(JN_THREADS))
    o = probe_order(2 * JN_THREADS + 1)
    # wave 0: its 64 rows of j = 0, of j = 1, and the one row of j = 2; then wave 1
    assert o[:130].tolist() == list(range(64)) + list(range(512, 576)) + [1024, 64]
    assert sorted(o.tolist()) == list(range(2 * JN_THREADS + 1))
    assert in_probe_rows(np.arange(1025))[o].tolist() == list(range(1025))


# ------------------------------------------------------------------------------------ running
_contexts = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _contexts.values():
        c.destroy()
    _contexts.clear()


def context(env=None, **kw):
    """one context per configuration, shared by the cases (the launch log is cleared for each)"""
    key = (tuple(sorted((env or {}).items())), tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _contexts:
        _contexts[key] = fm.tuned_context(env or {}, **kw)
    return _contexts[key]


def run(p, env=None, **kw):
    c = context(env, **kw)
    c.launch_log(True)
    try:
        got = capi.execute(p, c)
        ran = km.launched(c)
    finally:
        c.launch_log(False)
    return got, ran


def fams(ran):
    return {n.split("<")[0] for n in ran}


def strict(got, want, what=""):
    """the format of every column, then the content"""
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    rows = pc.strict_rows(got)
    assert rows == pl.canonical_rows(want), what
    return rows


def perm(rng, n):
    return rng.permutation(n).astype(np.int64)


def join_plan(bcols, pcols, outs, kind="join", build_left=True):
    """Scan(bcols) <kind> Scan(pcols) on column 0 of both; outs index the build side's columns, then
    the probe side's.  For OUTER the build side is the optional one."""
    lcols, rcols = (bcols, pcols) if build_left else (pcols, bcols)
    nb, lw = len(bcols), len(lcols)
    both = [c[0] for c in lcols] + [c[0] for c in rcols]
    p = pl.Plan()
    ls = p.new_scan_node(0, [(i, c[0]) for i, c in enumerate(lcols)])
    rs = p.new_scan_node(1, [(i, c[0]) for i, c in enumerate(rcols)])

    def at(o):  # build / probe numbering -> left / right numbering
        if build_left:
            return o
        return o + len(pcols) if o < nb else o - nb
    mk = {"join": p.new_join_node, "outer": p.new_outer_join_node, "full": p.new_full_outer_join_node}[kind]
    p.root = mk(build_left, ls, rs, 0, 0, [(at(o), both[at(o)]) for o in outs])
    p.new_input(pl.make_table(lcols))
    p.new_input(pl.make_table(rcols))
    assert lw == len(lcols)
    return p


def values(rng, dt, n):
    v = km.payload(rng, dt, max(n, 1), False)[1][:n]
    return np.asarray(v, dtype=NPT[dt])


# ------------------------------------------------------------------------------------ streams without NULLs
N32 = [1, 7, 8, 9, 31, 32, 33, ROWS32 - 1, ROWS32, ROWS32 + 1, 2 * ROWS32, 2 * ROWS32 + 1]
N64 = [1, ROWS64 - 1, ROWS64, ROWS64 + 1, 2 * ROWS64, 2 * ROWS64 + 9]


def stream_plan(n, wide, build_left=True):
    """n unique build keys, each hit once.  INT32 plan: key, two build payloads, one probe payload, all
    INT32.  64-bit plan: INT64 and INT32 build payloads (three carry words), an FP64 probe payload, the INT32
    keys — streams whose last pages differ."""
    rng = ap.rng_for("streams", n, wide)
    k = km.key_values(I32, np.arange(n))
    pb, pp = perm(rng, n), perm(rng, n)
    ta, tb, tc = (I64, I32, F64) if wide else (I32, I32, I32)
    bcols = [(I32, k[pb]), (ta, values(rng, ta, n)), (tb, values(rng, tb, n))]
    pcols = [(I32, k[pp]), (tc, values(rng, tc, n))]
    return join_plan(bcols, pcols, [4, 1, 2, 3, 0], build_left=build_left)


def page_counts(col):
    return [int(x) for x in col.pages[:, :2].copy().view(np.uint16)[:, 0]]


def expect_full_pages(got, n):
    for c in got.columns:
        rf = ROWS32 if c.type == I32 else ROWS64
        assert page_counts(c) == [rf] * (n // rf) + ([n % rf] if n % rf else []), (c.type, n)


@pytest.mark.parametrize("bits", [0, 3], ids=["bcast", "radix3"])
@pytest.mark.parametrize("how", ["in-place", "gathered"])
@pytest.mark.parametrize("wide,n", [(False, n) for n in N32] + [(True, n) for n in N64],
                         ids=[f"i32-{n}" for n in N32] + [f"i64f64-{n}" for n in N64])
def test_streams_without_nulls(wide, n, how, bits):
    p = stream_plan(n, wide, build_left=bool(n & 1))
    got, ran = run(p, ROWIDX if how == "gathered" else None, radix_bits=bits)
    strict(got, _oracle.execute(p), (wide, n, how, bits))
    expect_full_pages(got, n)
    f = fams(ran)
    assert ("k_join_bcast" if bits == 0 else "k_join") in f, sorted(ran)
    assert ("k_join" if bits == 0 else "k_join_bcast") not in f, sorted(ran)
    # the key stream (and a lone carried column) is written in place by the probe and finished by
    # k_finish_streams from the row count on the device
    assert "k_finish_streams" in f, sorted(ran)
    if how == "gathered":
        # both build payloads through the row index: k_gather into page images, k_finish_pages
        assert "k_finish_pages" in f and ("k_gather<8>" if wide else "k_gather<4>") in ran, sorted(ran)
    else:
        # ... out of the wide carry's records into page images, k_finish_pages
        assert "k_finish_pages" in f and "k_split_records" in f, sorted(ran)
    assert "k_encode_nullable" not in f, sorted(ran)


def test_int32_and_int64_streams_whose_last_pages_differ():
    n = 2 * ROWS32 + 1  # INT32: two full pages and one row; INT64 / FP64: three full pages and 948 rows
    p = stream_plan(n, True)
    got, ran = run(p)
    strict(got, _oracle.execute(p), n)
    w64, w32 = [ROWS64] * 3 + [n - 3 * ROWS64], [ROWS32, ROWS32, 1]
    assert [c.type for c in got.columns] == [F64, I64, I32, I32, I32]
    assert [page_counts(c) for c in got.columns] == [w64, w64, w32, w32, w32]
    assert "k_finish_streams" in fams(ran)


# ------------------------------------------------------------------------------------ columns with NULLs
PATTERNS = ["all-null", "all-valid", "alternating", "first-only", "last-only", "255-mod-256", "random-half"]


def pattern(name, n, rng):
    i = np.arange(n)
    return {"all-null": np.zeros(n, bool), "all-valid": np.ones(n, bool), "alternating": i % 2 == 0,
            "first-only": i == 0, "last-only": i == n - 1, "255-mod-256": i % 256 == 255,
            "random-half": rng.random(n) < 0.5}[name]


def n_grid(width):
    rf = RF[width]
    return [1, 255, 256, 257, 511, 512, 513, rf - 1, rf, rf + 1, 2 * rf + 3]


def nullable_source_plan(n, valid, dt, rng):
    """the probe side carries a nullable column, valid[i] placed for result row i; one more probe row
    behind them (no partner, NULL) keeps the column nullable when every row of the result is valid"""
    assert n + 1 <= JN_SUB
    k = km.key_values(I32, np.arange(n + 2))
    pb = perm(rng, n)
    bcols = [(I32, k[:n][pb]), (I32, values(rng, I32, n))]
    pcols = [(I32, np.concatenate([k[:n], k[n:n + 1]])), (dt, values(rng, dt, n + 1), np.concatenate([in_probe_rows(valid), [False]]))]
    return join_plan(bcols, pcols, [2, 3, 1])


def padded_plan(kind, n, valid, dt, rng):
    """OUTER / FULL: n preserved rows, a partner on the optional side for the row that becomes result
    row i where valid[i]: the optional side's column is NULL in the padded rows"""
    k = km.key_values(I32, np.arange(n))
    ko = k[in_probe_rows(valid)][perm(rng, int(valid.sum()))]
    ocols = [(I32, ko), (dt, values(rng, dt, ko.shape[0]))]
    pcols = [(I32, k), (I32, values(rng, I32, n))]
    return join_plan(ocols, pcols, [2, 1, 3, 0], kind=kind)


def agg_plan(n, valid, dt, rng):
    """n groups of two rows; a group has a value where the pattern says valid: SUM (INT64), MIN and MAX
    (the column's type) are NULL elsewhere"""
    k = np.repeat(km.key_values(I32, np.arange(n)), 2)
    v = values(rng, dt, 2 * n)
    vv = np.repeat(valid, 2) & (np.arange(2 * n) % 2 == 0)  # one of a valid group's two rows is NULL too
    outs = [(pl.AGG_KEY, 0, None), (pl.AGG_SUM, 1, I64), (pl.AGG_MIN, 1, None), (pl.AGG_MAX, 1, None), (pl.AGG_COUNT, 1, I64)]
    cols = [(I32, k), (dt, v, vv)]
    if dt == I32:  # (a nullable INT64 column fills the three carry words by itself)
        cols.append((I32, values(rng, I32, 2 * n)))
        outs.append((pl.AGG_MIN, 2, None))
    return ap.agg_plan(cols, outs)


@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("dt", [I32, I64, F64], ids=["i32", "i64", "f64"])
@pytest.mark.parametrize("where", ["source", "outer", "full"])
def test_nullable_columns(where, dt, pat):
    w = 4 if dt == I32 else 8
    for n in n_grid(w):
        rng = ap.rng_for("nullable", where, dt, pat, n)
        valid = pattern(pat, n, rng)
        p = nullable_source_plan(n, valid, dt, rng) if where == "source" else padded_plan(where, n, valid, dt, rng)
        got, ran = run(p)
        what = (where, dt, pat, n)
        strict(got, _aggref.execute(p), what)
        assert got.num_rows == n, what
        col = got.columns[1]
        assert col.type == dt and page_counts(col) == [RF[w]] * (n // RF[w]) + ([n % RF[w]] if n % RF[w] else []), what
        # the pattern sits where it was meant: row by row, not just as many
        realised = pc.check_column(col, n)[1]
        assert np.array_equal(realised, valid), (what, np.flatnonzero(realised != valid)[:8].tolist())
        assert f"k_encode_nullable<{w}>" in ran, (what, sorted(ran))
        fam = {"source": "k_join_bcast", "outer": "k_outer_bcast", "full": "k_full_bcast"}[where]
        if valid.any():  # (an empty optional side has nothing to probe)
            assert fam in fams(ran), (what, sorted(ran))


@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("dt", [I32, I64], ids=["i32", "i64"])
def test_nullable_agg_outputs(dt, pat):
    """Not placed: the groups come out in the order of the aggregation's hash table, so the patterns
    set HOW MANY groups have no value and which keys those are, not which rows of the result; the three
    nullable outputs are held to the format, to the reference's content and to the count.  (The node
    takes INT32 and INT64 values only: there is no FP64 MIN / MAX to send through k_agg_column<8>.)"""
    for n in n_grid(8) + ([ROWS32 - 1, ROWS32, ROWS32 + 1, 2 * ROWS32 + 3] if dt == I32 else []):
        rng = ap.rng_for("nullable-agg", dt, pat, n)
        valid = pattern(pat, n, rng)
        p = agg_plan(n, valid, dt, rng)
        got, ran = run(p)
        what = (dt, pat, n)
        strict(got, _aggref.execute(p), what)
        assert got.num_rows == n, what
        for ci in (1, 2, 3):  # SUM, MIN, MAX
            assert int(pc.check_column(got.columns[ci], n)[1].sum()) == int(valid.sum()), (what, ci)
        # SUM is INT64: k_agg_column<8> adds the validity, k_encode_nullable<8> writes the pages; MIN /
        # MAX of an INT32 column are narrowed by k_agg_column<4> and written by k_encode_nullable<4>
        want = {"k_agg_column<8>", "k_encode_nullable<8>"} | ({"k_agg_column<4>", "k_encode_nullable<4>"} if dt == I32 else set())
        assert want <= set(ran), (what, sorted(ran))
        # COUNT has no NULLs: k_gather into page images + k_finish_pages (col_to_result)
        assert "k_finish_pages" in fams(ran), (what, sorted(ran))


def test_nullable_columns_partitioned_and_gathered():
    """the same writers behind the partitioned kernels, and with the nullable column gathered through a
    row index (k_gather / k_outer_gather with validity bytes) instead of split out of a wide carry.
    A random half: nothing is meant for a certain row (partitioned rows come out by partition)."""
    for env, bits in ((None, 3), (ROWIDX, 0), (ROWIDX, 3)):
        for dt in (I32, I64):
            w = 4 if dt == I32 else 8
            for n in (RF[w], RF[w] + 1, 2 * RF[w] + 3):
                rng = ap.rng_for("nullable-part", dt, n)
                valid = pattern("random-half", n, rng)
                for p in (nullable_source_plan(n, valid, dt, rng), padded_plan("outer", n, valid, dt, rng), padded_plan("full", n, valid, dt, rng)):
                    got, ran = run(p, env, radix_bits=bits)
                    strict(got, _aggref.execute(p), (env, bits, dt, n))
                    assert f"k_encode_nullable<{w}>" in ran, sorted(ran)
                    if bits:
                        assert not [f for f in fams(ran) if f.endswith("_bcast")], sorted(ran)


# ------------------------------------------------------------------------------------ VARCHAR
ENCODERS = [("host", None), ("device", VDEV)]


def vc_plan(strings, rng, placed):
    """the probe row with id i meets the build row that holds strings[i]; placed: id i sits at the probe
    row that becomes result row i"""
    n = len(strings)
    ids = np.arange(n, dtype=np.int32)
    pb = perm(rng, n)
    bcols = [(I32, ids[pb]), (VC, [strings[i] for i in pb])]
    return join_plan(bcols, [(I32, in_probe_rows(ids) if placed else ids)], [2, 1])


def vc_check(strings, env, what, radix_bits=0):
    n = len(strings)
    placed = 0 < n <= JN_SUB and radix_bits == 0
    p = vc_plan(strings, ap.rng_for("vc", what), placed)
    got, ran = run(p, env, radix_bits=radix_bits)
    assert got.num_rows == n and [c.type for c in got.columns] == [I32, VC], what
    (ids, ok) = pc.check_column(got.columns[0], n)
    strs = pc.check_column(got.columns[1], n)  # the strict decode alone: no pyrj.pages decoder
    assert ok.all() and sorted(ids.tolist()) == list(range(n)), what
    if placed:  # result row i holds strings[i]: the encoder met the rows in the order of `strings`
        assert np.array_equal(ids, np.arange(n)), (what, np.flatnonzero(ids != np.arange(n))[:8].tolist())
    bad = [int(i) for i, s in zip(ids, strs) if s != strings[int(i)]]
    assert not bad, (what, bad[:5])
    assert pc.same_as([strs], [pl.decode_table(got)[1]]), what
    f = fams(ran)
    if env:
        assert ("k_vc_walk<true>" in ran and "k_vc_walk<false>" in ran and "k_vc_encode" in f and "k_vc_resolve" in f) or n == 0, (what, sorted(ran))
    else:
        assert not [x for x in f if x.startswith("k_vc_")], (what, sorted(ran))
    return got.columns[1], ids


def text(n, tag):
    """n characters that depend on the position and the string (a misplaced copy shows)"""
    if n == 0:
        return b""
    return (np.arange(n, dtype=np.int64) * 7 + tag * 13).astype(np.uint8).tobytes()


LENGTHS = [0, 1, 8184, 8185, 8186, 8188, 8189, 2 * 8188, 2 * 8188 + 1, 3 * 8188 - 1]


@pytest.mark.parametrize("enc,env", ENCODERS, ids=[e[0] for e in ENCODERS])
@pytest.mark.parametrize("length", LENGTHS)
def test_varchar_string_lengths(length, enc, env):
    col, _ = vc_check([text(length, 1)], env, (length, "alone"))
    kinds = page_counts(col)
    assert kinds == ([1] if length <= 8185 else [0xFFFF] + [0xFFFE] * (-(-length // 8188) - 1)), kinds
    col, ids = vc_check([b"a", text(length, 2), b"bc"], env, (length, "between"))
    if length > 8185:
        assert page_counts(col).count(0xFFFF) == 1 and page_counts(col).count(0xFFFE) == -(-length // 8188) - 1
    col, _ = vc_check([None, text(length, 3), None, text(length, 4), b""], env, (length, "twice, between NULLs"))


def fill_sum(k, length):
    """what the fill rule compares with 8192 when row k (0-based) of a page of equal strings arrives"""
    return 4 + 2 * (k + 1) + (k + 1) * length + k // 8 + 1


def equal_runs(target, null_arrives=False, k_max=VC_CHUNK):
    """(k, L): k rows of L characters are in the page — each of them fitted when it came — and the row
    that arrives, another string of L characters or a NULL, makes the fill rule's sum land exactly on
    `target`"""
    out = []
    for k in range(1, k_max):
        if null_arrives:
            rest, per = target - (4 + 2 * k + k // 8 + 1), k
        else:
            rest, per = target - (4 + 2 * (k + 1) + k // 8 + 1), k + 1
        if rest >= 0 and rest % per == 0 and rest // per <= 8185 and fill_sum(k - 1, rest // per) <= 8192:
            out.append((k, rest // per))
    return out


@pytest.mark.parametrize("enc,env", ENCODERS, ids=[e[0] for e in ENCODERS])
@pytest.mark.parametrize("target", [8192, 8193])
def test_varchar_equal_strings_that_fill_a_page_exactly(target, enc, env):
    sols = equal_runs(target)
    assert len(sols) >= 2, sols  # (8192: k = 2 and 30; 8193: k = 1 ... 108 — every solution is run)
    for k, length in sols:
        assert fill_sum(k, length) == target and 0 < length <= 8185
        # at 8192 row k still fits (k + 1 rows per page), at 8193 it opens the next page (k rows)
        per_page = k + 1 if target == 8192 else k
        assert fill_sum(per_page - 1, length) <= 8192 < fill_sum(per_page, length)
        n = 2 * per_page + 1
        col, _ = vc_check([text(length, i) for i in range(n)], env, (target, k, length))
        counts = page_counts(col)
        # equal strings: the boundaries do not depend on the order of the rows.  The host encoder fills
        # like the reference; the device encoder as well, but opens a page at every VC_CHUNK rows
        if env is None:
            assert counts == [per_page, per_page, 1], (k, length, counts)
        else:
            want, r = [], 0
            while r < n:
                take = min(per_page, n - r, VC_CHUNK - r % VC_CHUNK)
                want.append(take)
                r += take
            assert counts == want, (k, length, counts, want)


@pytest.mark.parametrize("enc,env", ENCODERS, ids=[e[0] for e in ENCODERS])
@pytest.mark.parametrize("target", [8192, 8193])
def test_varchar_null_arrives_at_the_full_page(target, enc, env):
    """A NULL costs a page nothing but its bitmap bit: with k strings in, its sum is the k-th string's
    own sum plus one where the NULL opens a bitmap byte (k a multiple of 8) and the same otherwise.  So a
    NULL lands on 8193 only behind a k-th string that landed on 8192 with k a multiple of 8; with equal
    strings that is k = 736, L = 9 alone — more rows than a device chunk holds, so the device encoder
    gets there with 503 strings of 14 characters and one of 75.  Every run is one chunk of probe rows, laid
    out so that the NULL is row k of the result, which is asserted."""
    sols = equal_runs(target, null_arrives=True, k_max=4000)
    assert sols == ([(1, 8185), (3, 2727), (24, 339), (31, 262), (2620, 1), (3853, 0)] if target == 8192 else [(736, 9)]), sols
    runs = [[length] * k for k, length in sols]
    if target == 8193:
        assert all(k % 8 == 0 for k, _ in sols)
        runs.append([14] * 503 + [75])
        assert len(runs[-1]) < VC_CHUNK
    for lens in runs:
        k, chars = len(lens), sum(lens)
        assert 4 + 2 * k + chars + k // 8 + 1 == target                       # the NULL's sum
        assert 4 + 2 * k + chars + (k - 1) // 8 + 1 <= 8192                    # the k-th string fitted
        reps = 3 if 3 * (k + 1) <= JN_SUB else 1
        assert reps * (k + 1) <= JN_SUB  # one chunk of probe rows: every row is placed
        strings = []
        for rep in range(reps):
            strings += [text(n, rep * k + i) for i, n in enumerate(lens)] + [None]
        col, _ = vc_check(strings, env, ("null arrives", target, k, lens[0]))
        strs = pc.check_column(col, len(strings))
        assert strs[k] is None and None not in strs[:k], (k, lens[0])  # the NULL is row k of the result
        # at 8192 the NULL still joins the k strings, at 8193 it opens the next page.  The device
        # encoder opens a page every VC_CHUNK rows, so only runs below that get to the sum there
        if env is None or k < VC_CHUNK:
            assert page_counts(col)[0] == (k + 1 if target == 8192 else k), (k, lens[0], page_counts(col)[:3])
        else:
            assert page_counts(col)[0] == VC_CHUNK


@pytest.mark.parametrize("enc,env", ENCODERS, ids=[e[0] for e in ENCODERS])
@pytest.mark.parametrize("n", [VC_CHUNK - 1, VC_CHUNK, VC_CHUNK + 1, 2 * VC_CHUNK + 1])
@pytest.mark.parametrize("what", ["empty", "one-byte", "null"])
def test_varchar_chunk_edges(what, n, enc, env):
    s = {"empty": b"", "one-byte": b"x", "null": None}[what]
    col, _ = vc_check([s] * n, env, (what, n))
    counts = page_counts(col)
    if env is None:
        assert counts == [n]  # one page: more than 256 rows (the device encoder's slab) in all of them
    else:
        assert counts == [VC_CHUNK] * (n // VC_CHUNK) + ([n % VC_CHUNK] if n % VC_CHUNK else [])


@pytest.mark.parametrize("enc,env", ENCODERS, ids=[e[0] for e in ENCODERS])
@pytest.mark.parametrize("at", [0, VC_CHUNK - 1, VC_CHUNK, 2 * VC_CHUNK - 1, 2 * VC_CHUNK])
def test_varchar_long_string_at_a_chunk_edge(at, enc, env):
    n = 2 * VC_CHUNK + 1
    strings = [b"s%d" % i for i in range(n)]
    strings[at] = text(8188 + 700, at)
    strings[(at + 300) % n] = None
    col, ids = vc_check(strings, env, ("long at", at))
    counts = page_counts(col)
    assert counts.count(0xFFFF) == 1 and counts.count(0xFFFE) == 1
    # the long string is row `at` of the result: exactly `at` rows lie in the pages in front of its chain
    first = counts.index(0xFFFF)
    assert int(ids[at]) == at and sum(counts[:first]) == at and counts[first + 1] == 0xFFFE, (at, counts)
    if env is not None and at:  # the device encoder: whole chunks in front of / up to the edge
        assert counts[:first] == [VC_CHUNK] * (at // VC_CHUNK) + ([at % VC_CHUNK] if at % VC_CHUNK else []), counts


@pytest.mark.parametrize("enc,env", ENCODERS, ids=[e[0] for e in ENCODERS])
@pytest.mark.parametrize("n", [65_503, 65_504, 65_505])
def test_varchar_all_null_column_at_the_largest_page(n, enc, env):
    col, _ = vc_check([None] * n, env, ("all null", n))
    counts = page_counts(col)
    if env is None:
        assert counts == ([n] if n <= 65_504 else [65_504, 1]), counts
    else:
        assert counts == [VC_CHUNK] * (n // VC_CHUNK) + ([n % VC_CHUNK] if n % VC_CHUNK else [])


# ------------------------------------------------------------------------------------ other sources of pages
def test_result_kept_on_the_device():
    n = 2 * ROWS32 + 1
    rng = ap.rng_for("resident")
    valid = pattern("random-half", n, rng)
    for p in (stream_plan(n, True), nullable_source_plan(n, valid, I64, rng), agg_plan(n, valid, I32, rng)):
        want = _aggref.execute(p)
        c = context()
        tables = [c.upload(t) for t in p.inputs]
        try:
            r = c.execute_resident(p, tables, keep_on_device=True)
            try:
                assert all(r.device_pages(k) for k in range(r.num_cols))
                strict(r.to_table(), want)
            finally:
                r.free()
        finally:
            for t in tables:
                t.release()


def test_two_ranks_pages_concatenated():
    """Two virtual ranks on one GPU.  execute_sharded leaves each rank's pages on its rank: each is a
    column of its own, and put one behind the other (what the host path of a group context returns)
    they are a column with partial pages in the middle."""
    from test_gpu_sharded import shard_table

    rng = ap.rng_for("two ranks")
    n = 2 * ROWS32 * 2 + 777
    k = km.key_values(I32, np.arange(n))
    bcols = [(I32, k[perm(rng, n)]), (I64, values(rng, I64, n))]
    pcols = [(I32, k[perm(rng, n)]), (I32, values(rng, I32, n), rng.random(n) < 0.5)]
    p = join_plan(bcols, pcols, [0, 1, 3])
    want = _oracle.execute(p)
    c = context(devices=[0, 0])
    shards = [shard_table(t, 2) for t in p.inputs]
    tables = [[c.lane(d).upload(shards[i][d]) for i in range(2)] for d in range(2)]
    try:
        res = c.execute_sharded(p, tables)
        parts = [r.to_table() for r in res]
        for r in res:
            r.free()
    finally:
        for row in tables:
            for t in row:
                t.release()
    assert sum(t.num_rows for t in parts) == n
    for t in parts:
        pc.strict_rows(t)
        # ragged: no rank's share is a whole number of pages of either width
        assert t.num_rows % ROWS32 and t.num_rows % ROWS64, [x.num_rows for x in parts]
    whole = pl.ColumnarTable(n, [pl.Column(a.type, np.concatenate([a.pages, b.pages])) for a, b in zip(parts[0].columns, parts[1].columns)])
    assert pc.strict_rows(whole) == pl.canonical_rows(want)
    for col in whole.columns:
        counts = page_counts(col)
        assert any(x < (ROWS32 if col.type == I32 else ROWS64) for x in counts[:-1]), counts


def test_group_context_concatenates_its_ranks_pages():
    """Contest::execute on a context of two virtual ranks: inputs from 2 * 1984 * 1007 rows on are cut
    at that multiple and joined rank by rank; rank 0's result takes rank 1's pages behind its own."""
    rng = ap.rng_for("group")
    n_probe = 2 * ROWS32 * ROWS64 + 17
    n = 3 * ROWS32 + 5
    k = km.key_values(I32, np.arange(n))
    miss = km.key_values(I32, np.array([n + 7]))[0]
    pk = np.full(n_probe, miss, dtype=np.int32)
    pk[rng.choice(n_probe, n, replace=False)] = k  # every build key is hit once, by rows of both shards
    pv = np.arange(n_probe, dtype=np.int64)
    p = join_plan([(I32, k[perm(rng, n)]), (I64, values(rng, I64, n))], [(I32, pk), (I64, pv)], [0, 1, 3])
    ok, why = capi.plan_shardable(p)
    assert ok, why
    got, _ = run(p, devices=[0, 0])
    strict(got, _oracle.execute(p))
    assert got.num_rows == n
    for col in got.columns:
        counts = page_counts(col)
        rf = ROWS32 if col.type == I32 else ROWS64
        assert sum(counts) == n and any(x < rf for x in counts[:-1]), counts


def test_root_without_rows_has_no_pages():
    rng = ap.rng_for("empty")
    k = km.key_values(I32, np.arange(200))
    bcols = [(I32, k[:100]), (I64, values(rng, I64, 100)), (VC, [b"s%d" % i for i in range(100)])]
    pcols = [(I32, k[100:]), (I32, values(rng, I32, 100), rng.random(100) < 0.5)]
    for env in (None, VDEV):
        for bits in (0, 3):
            for kind in ("join", "outer"):
                outs = [0, 1, 3, 4] + ([2] if kind == "join" else [])
                p = join_plan(bcols, pcols, outs, kind=kind, build_left=True)
                if kind == "outer":  # an empty preserved side: nothing to pad
                    p.inputs[1] = pl.make_table([(I32, k[:0]), (I32, values(rng, I32, 0))])
                got, _ = run(p, env, radix_bits=bits)
                assert got.num_rows == 0 and len(got.columns) == len(outs)
                assert all(c.pages.shape[0] == 0 for c in got.columns)
                assert pc.strict_rows(got) == []
    p = ap.agg_plan([(I32, np.zeros(0, np.int32)), (I64, np.zeros(0, np.int64))], ap.ALL)
    got, _ = run(p)
    assert got.num_rows == 0 and all(c.pages.shape[0] == 0 for c in got.columns) and pc.strict_rows(got) == []
