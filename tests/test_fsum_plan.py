"""RJ_AGG_FSUM (include/rj.h, RJ_NODE_GROUP) without a GPU: the reference tests/_fsumref.py against
math.fsum and a row-at-a-time dictionary of Fractions, and the host twin of the kernels' arithmetic
(rj_debug_fsum: csrc/rj_fsum.hpp's split, add, propagate, merge and round) against that reference, bit
for bit.  tests/test_gpu_fsum.py compares the device with the same reference."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _fsumref
import _groupref
import test_group_plan as gp
import test_sort_plan as sp
from pyrj import capi
from pyrj import plan as pl

I32, I64, F64 = pl.INT32, pl.INT64, pl.FP64
KEY, STAR, COUNT, MIN, MAX, FSUM = pl.AGG_KEY, pl.AGG_COUNT_STAR, pl.AGG_COUNT, pl.AGG_MIN, pl.AGG_MAX, pl.AGG_FSUM
rng_for, bits_of, f64_of = sp.rng_for, sp.bits_of, sp.f64_of
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX, TINY = bits_of(sp.DBL_MAX), 1                      # bit patterns
PINF, NINF, NAN = _fsumref.PINF, _fsumref.NINF, _fsumref.CANON_NAN
NEG = 1 << 63
pow2 = lambda e: bits_of(math.ldexp(1.0, e))                # 2^e, -1074 <= e <= 1023


# ------------------------------------------------------------------ the edge grid (shared with the GPU tests)
def edge_grid():
    """name -> (bits, valid or None)"""
    every = [pow2(e) for e in range(-1074, 1024)]
    g = {
        "every-power-of-two": every,
        "every-power-of-two-negated": [b | NEG for b in every],
        "every-power-of-two-and-its-negative": every + [b | NEG for b in every],
        "tie-to-even-down": [pow2(53), bits_of(1.0)],
        "tie-broken-by-the-smallest-subnormal": [pow2(53), bits_of(1.0), TINY],
        "tie-to-even-up-missed-by-one-unit": [pow2(53), bits_of(3.0), TINY | NEG],
        "tie-to-even-up": [pow2(53), bits_of(3.0)],
        "max-plus-max-minus-max": [DBL_MAX, DBL_MAX, DBL_MAX | NEG],
        "no-intermediate-overflow": [bits_of(1e308), bits_of(1e308), bits_of(-1e308), bits_of(-1e308), bits_of(1.0)],
        "lands-on-the-overflow-threshold": [DBL_MAX, pow2(970)],                 # 2^1024 - 2^970: a tie, the even side is 2^1024
        "just-below-the-overflow-threshold": [DBL_MAX, pow2(970), TINY | NEG],
        "negative-overflow-threshold": [DBL_MAX | NEG, pow2(970) | NEG],
        "max-twice": [DBL_MAX, DBL_MAX],
        "subnormal-sum": [TINY] * 5 + [3 | NEG],
        "subnormals-into-the-normals": [(1 << 52) - 1, TINY],
        "largest-subnormal-twice": [(1 << 52) - 1] * 2,
        "full-cancellation": [bits_of(1.5), bits_of(-1.5), DBL_MAX, DBL_MAX | NEG, TINY, TINY | NEG],
        "negative-cancellation-to-zero": [bits_of(-2.5), bits_of(2.5)],
        "all-negative-zero": [NEG] * 7,
        "both-zeros": [NEG, 0],
        "one-value": [bits_of(-0.1)],
        "one-negative-zero": [NEG],
        "two-values": [bits_of(0.1), bits_of(0.2)],
        "large-cancellation-then-a-tiny-rest": [DBL_MAX, bits_of(1e300), TINY, DBL_MAX | NEG, bits_of(-1e300)],
        "negative-result-with-sticky-bits": [pow2(200) | NEG, pow2(100) | NEG, TINY | NEG],
        "n=0": [],
    }
    specials = {"pinf": [PINF], "ninf": [NINF], "both-inf": [PINF, NINF], "nan": [bits_of(math.nan)], "neg-nan": [sp.NEG_NAN],
                "snan": [sp.SNAN], "nan-and-inf": [sp.PAYLOAD_NAN, PINF], "nan-and-both": [NINF, sp.QNAN, PINF], "pinf-twice": [PINF, PINF]}
    for name, sv in specials.items():
        g["special-" + name] = (sv, None)
        g["special-" + name + "-with-finite"] = ([DBL_MAX, bits_of(-3.5)] + sv + [DBL_MAX, TINY], None)
    g = {k: (v if isinstance(v, tuple) else (v, None)) for k, v in g.items()}
    base = [bits_of(1.0), pow2(53), bits_of(-0.75)]
    for pos in range(3):
        g[f"null-at-{pos}"] = (base, [i != pos for i in range(3)])
    g["null-everywhere"] = (base, [False] * 3)
    g["null-hides-nan-and-inf"] = ([bits_of(math.nan), bits_of(2.0), PINF], [False, True, False])
    g["one-null"] = ([bits_of(1.0)], [False])
    return g


EDGE = edge_grid()


def lib_fsum(bits, valid=None):
    return capi.fsum(np.array(bits, dtype=np.uint64), None if valid is None else ~np.asarray(valid, dtype=bool))


def random_multiset(rng, n):
    """random bit patterns (finite), a narrow exponent band, and pairs that cancel, mixed"""
    kind = rng.integers(0, 3, n)
    raw = rng.integers(0, 2**64, n, dtype=np.uint64)
    raw = np.where((raw >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF), raw & np.uint64(0xBFFFFFFFFFFFFFFF), raw)
    band = (rng.random(n) * 2 - 1) * np.exp2(rng.integers(-3, 4, n)) * math.ldexp(1.0, int(rng.integers(-1000, 1000)))
    v = np.where(kind == 0, raw, band.view(np.uint64))
    half = n // 2
    pair = (kind == 2)[:half]
    v[half:2 * half][pair] = v[:half][pair] ^ np.uint64(NEG)
    return v


# ------------------------------------------------------------------ the reference
def test_reference_agrees_with_math_fsum():
    rng = rng_for("ref-fsum")
    seen = 0
    for _ in range(300):
        bits = random_multiset(rng, int(rng.integers(1, 400)))
        try:
            want = math.fsum(bits.view(np.float64).tolist())
        except OverflowError:
            continue
        seen += 1
        assert _fsumref.fsum_bits(bits) == bits_of(want + 0.0 if want else 0.0)
    assert seen > 100
    for name, (bits, valid) in EDGE.items():
        if valid is None and bits and not name.startswith("special") and "overflow" not in name and name != "max-twice":
            try:
                want = math.fsum([f64_of(b) for b in bits])
            except OverflowError:       # (math.fsum gives up on an intermediate overflow; the exact sum does not have one)
                continue
            assert _fsumref.fsum_bits(bits) == bits_of(want if want else 0.0), name


def test_reference_rules():
    f = _fsumref.fsum_bits
    assert f([]) is None and f([1, 2], [False, False]) is None
    assert f(EDGE["lands-on-the-overflow-threshold"][0]) == PINF and f(EDGE["negative-overflow-threshold"][0]) == NINF
    assert f(EDGE["just-below-the-overflow-threshold"][0]) == DBL_MAX and f(EDGE["max-twice"][0]) == PINF
    assert f(EDGE["no-intermediate-overflow"][0]) == bits_of(1.0) and f(EDGE["all-negative-zero"][0]) == 0
    assert f(EDGE["tie-to-even-down"][0]) == pow2(53) and f(EDGE["tie-broken-by-the-smallest-subnormal"][0]) == pow2(53) + 1
    assert f(EDGE["tie-to-even-up"][0]) == pow2(53) + 2 and f(EDGE["tie-to-even-up-missed-by-one-unit"][0]) == pow2(53) + 1
    assert f(EDGE["special-nan-and-both"][0]) == NAN and f(EDGE["special-both-inf-with-finite"][0]) == NAN
    assert f(EDGE["special-pinf-with-finite"][0]) == PINF and f(EDGE["special-ninf"][0]) == NINF
    assert f(EDGE["null-hides-nan-and-inf"][0], EDGE["null-hides-nan-and-inf"][1]) == bits_of(2.0)


def dictionary_groups(rows, n_keys):
    """row-at-a-time: key tuple -> [count, Fraction sum, flags]; rows = (key..., value or None)"""
    groups = {}
    for r in rows:
        g = groups.setdefault(r[:n_keys], [0, Fraction(0), set()])
        v = r[n_keys]
        if v is None:
            continue
        g[0] += 1
        if math.isnan(v):
            g[2].add("nan")
        elif math.isinf(v):
            g[2].add("+" if v > 0 else "-")
        else:
            g[1] += Fraction(v)
    out = {}
    for k, (cnt, total, flags) in groups.items():
        if cnt == 0:
            out[k] = None
        elif "nan" in flags or {"+", "-"} <= flags:
            out[k] = NAN
        elif flags:
            out[k] = PINF if "+" in flags else NINF
        else:
            try:
                x = float(total)
            except OverflowError:
                x = math.inf if total > 0 else -math.inf
            out[k] = bits_of(x if x else 0.0)
    return out


def fsum_table(rng, n, groups, null_p=0.2, specials=True):
    """an INT32 key and a nullable FP64 column of mixed magnitudes, signs, cancelling pairs and a few non-finite values"""
    k = rng.integers(0, groups, n).astype(np.int32)
    v = random_multiset(rng, n).view(np.float64).copy()
    if specials and n > 8:
        at = rng.integers(0, n, 4)
        v[at[0]], v[at[1]], v[at[2]] = np.inf, -np.inf, np.nan
    return [(I32, k, np.ones(n, dtype=bool)), (F64, v, rng.random(n) >= null_p)]


@pytest.mark.parametrize("seed", range(6))
def test_reference_agrees_with_a_dictionary_of_fractions(seed):
    rng = rng_for("dict", seed)
    n = int(rng.integers(1, 1500))
    cols = fsum_table(rng, n, int(rng.integers(1, 40)))
    ng, out = _fsumref.group(cols, [(0, 0)], [(KEY, 0, I32), (FSUM, 1, F64), (COUNT, 1, I64), (FSUM, 1, F64)])
    rows = [(int(k), None if not ok else float(v)) for k, v, ok in zip(cols[0][1], cols[1][1], cols[1][2])]
    want = dictionary_groups(rows, 1)
    assert ng == len(want)
    for i in range(ng):
        w = want[(int(out[0][1][i]),)]
        assert bool(out[1][2][i]) == (w is not None)
        assert int(out[1][1].view(np.uint64)[i]) == (w or 0) == int(out[3][1].view(np.uint64)[i])
    # the scalar aggregate, and everything but FSUM is _groupref's
    ng, out = _fsumref.group(cols, [], [(FSUM, 1, F64), (STAR, 0, I64)])
    assert ng == 1 and int(out[0][1].view(np.uint64)[0]) == (dictionary_groups([(0, r[1]) for r in rows], 1)[(0,)] or 0)
    assert int(out[1][1][0]) == n
    ng, out = _fsumref.group([(I32, np.zeros(0, np.int32), np.zeros(0, bool)), (F64, np.zeros(0), np.zeros(0, bool))], [], [(FSUM, 1, F64)])
    assert ng == 1 and not out[0][2][0]


# ------------------------------------------------------------------ the host twin of the kernels' arithmetic
@pytest.mark.parametrize("name", sorted(EDGE))
def test_library_on_the_edge_grid(name):
    bits, valid = EDGE[name]
    want = _fsumref.fsum_bits(bits, valid)
    got = lib_fsum(bits, valid)
    assert got == want, (name, got and hex(got), want and hex(want))
    if bits:
        at = rng_for("edge", name).permutation(len(bits))
        assert lib_fsum([bits[i] for i in at], None if valid is None else [valid[i] for i in at]) == want


@pytest.mark.parametrize("block", range(20))
def test_library_on_random_multisets_in_two_orders(block):
    """2 000 seeded multisets of 1 to 5 000 values, each again shuffled: the same bits"""
    rng = rng_for("random", block)
    for case in range(100):
        n = int(rng.integers(1, 5001)) if case % 10 == 0 else int(rng.integers(1, 300))
        bits = random_multiset(rng, n)
        valid = rng.random(n) >= 0.1 if case % 3 == 0 else None
        want = _fsumref.fsum_bits(bits, valid)
        assert lib_fsum(bits, valid) == want, (block, case)
        at = rng.permutation(n)
        assert lib_fsum(bits[at], None if valid is None else valid[at]) == want, (block, case, "shuffled")


ONES = (1 << 52) - 1      # with the hidden bit: a significand of 53 ones


@pytest.mark.parametrize("name,bits", [("dbl-max", DBL_MAX), ("smallest-subnormal", TINY), ("negative-dbl-max", DBL_MAX | NEG),
                                        ("53-ones-at-shift-0", 1025 << 52 | ONES), ("53-ones-at-shift-31", 1056 << 52 | ONES)])
def test_library_on_four_million_copies(name, bits):
    """carries across many chunks, and a thousand partial sums merged: n * x in closed form.  (No double
    fills all three 32-bit pieces: a significand has 53 bits.  53 ones fill the low piece at shift 0 and
    the middle one at shift 31, the largest pieces there are.)"""
    n = 1 << 22
    if name.startswith("53-ones"):
        p = ((bits >> 52) & 0x7FF) - 1
        v = (ONES | 1 << 52) << (p & 31)
        assert p & 31 == int(name.split("-")[-1]) and 0xFFFFFFFF in (v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF)
    want = _fsumref.round_units(n * _fsumref.units(bits))
    assert lib_fsum(np.full(n, bits, dtype=np.uint64)) == want
    both = np.full(n, bits, dtype=np.uint64)
    both[1::2] ^= np.uint64(NEG)
    assert lib_fsum(both) == 0


def test_library_argument_checks():
    L = capi.load()
    assert L.rj_debug_fsum(None, None, 0, None, None) == 1          # RJ_ERR_ARG: no output pointers
    assert capi.fsum([]) is None and capi.fsum([bits_of(1.0)], [1]) is None and capi.fsum([bits_of(1.0)], [0]) == bits_of(1.0)
    with pytest.raises(ValueError):
        capi.fsum([1, 2], [0])


# ------------------------------------------------------------------ the plan, the header, the exports
def test_code_8_is_marshalled_and_the_header_and_exports_agree():
    assert pl.AGG_FSUM == 8 and pl.AGG_MAX == 5
    cols = [(I32, np.arange(4, dtype=np.int32)), (F64, np.arange(4) * 0.5)]
    p = gp.group_plan(cols, [(0, 0)], [(KEY, 0, I32), (FSUM, 1, F64), (COUNT, 1, I64)])
    cplan, keep = pl.plan_to_c(p)
    node = cplan.nodes[p.root]
    assert node.n_out == 3 and node.out_idx[1] == (8 << 56) | 1 and node.out_type[1] == F64
    assert pl.agg_func(node.out_idx[1]) == 8 and pl.agg_col(node.out_idx[1]) == 1
    del keep
    header = open(os.path.join(ROOT, "include", "rj.h")).read()
    for text in ("RJ_AGG_FSUM       = 8", "RJ_AGG_MAX        = 5", "int rj_debug_fsum(const uint64_t* bits, const uint8_t* is_null",
                 "FSUM(x) / TO_F64(COUNT(x))", "ties to even"):
        assert text in header, text
    assert not re.search(r"RJ_AGG_\w+\s*=\s*[67]\b", header)
    assert "rj_debug_fsum" in capi.EXPORTS and capi.load().rj_abi_version() == 3
    n, out = _fsumref.evaluate(p)
    assert n == 4 and out[1][1].tolist() == [0.0, 0.5, 1.0, 1.5]
    # everything but FSUM is _groupref's
    q = gp.group_plan(cols, [(0, 0)], [(KEY, 0, I32), (COUNT, 1, I64)])
    assert _groupref.rel_rows(*reversed(_groupref.evaluate(q))) == _fsumref.rel_rows(*reversed(_fsumref.evaluate(q)))
