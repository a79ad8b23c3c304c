"""The pass plan of the radix partition driver (csrc/rj_radix_plan.cpp, C-ABI rj_debug_partition_plan): every decision a
partition call takes before its first launch, checked without a GPU —
  * against the independent host model tests/_specref.py: bits per pass, the speculative first pass' capacity bound,
    tiles per group of the first pass;
  * a decision table: which layout, histogram and speculation each (key words, carry words, bits, knobs) case gets;
  * the requests that switch speculation (and, where the driver has no kernels for it, the fine histogram) off;
  * invariants over a sweep of bits x carry shapes x knob settings.
The library reads the RJ_TUNE_* variables at every call, as a context reads them when it is made."""
import itertools

import pytest

import _specref
from pyrj import capi

KNOBS = ["RJ_TUNE_BLOCKED_MID", "RJ_TUNE_MALL_CHUNK", "RJ_TUNE_P1_BITS", "RJ_TUNE_FINE", "RJ_TUNE_PACK", "RJ_TUNE_AOS3",
         "RJ_TUNE_AOS_MID", "RJ_TUNE_TPG1", "RJ_TUNE_TPG2", "RJ_TUNE_PACKED_SIDE", "RJ_TUNE_XCD_MIN_ROWS", "RJ_TUNE_XCD_SPLIT",
         "RJ_TUNE_SPEC_P1", "RJ_TUNE_SPEC_MIN_ROWS", "RJ_TUNE_SPEC_SAMPLE", "RJ_TUNE_SPEC_Z", "RJ_TUNE_SPEC_P2",
         "RJ_TUNE_SPEC2_MIN_ROWS", "RJ_TUNE_SPEC2_SAMPLE", "RJ_TUNE_SPEC2_Z"]
MIN_ROWS_0 = {"RJ_TUNE_XCD_MIN_ROWS": 0, "RJ_TUNE_SPEC_MIN_ROWS": 0, "RJ_TUNE_SPEC2_MIN_ROWS": 0}
N = 1 << 20
PACKED_MIDS = ("packed", "packed_side", "blocked")
AOS_MIDS = ("aos3", "aos3_side")


@pytest.fixture
def plan(monkeypatch):
    """plan(knobs, n, kw, cw, bits, **request) under exactly these knobs (every other one at its default)"""
    def run(knobs, *a, **kw):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in knobs.items():
            monkeypatch.setenv(k, str(v))
        return capi.partition_plan(*a, **kw)
    return run


# ------------------------------------------------------------------------------------------ against tests/_specref.py
def test_bits_per_pass_follow_the_model(plan):
    for bits in range(28):
        p = plan({}, N, 1, 1, bits)
        assert p["pbits"] == _specref.pass_bits(bits) and p["passes"] == len(p["pbits"]), bits
        assert [ps["bits"] for ps in p["pass"]] == p["pbits"]


@pytest.mark.parametrize("n", [1029, 3 * 16384 + 1029, 20 * 16384 + 1029, 1 << 30])
def test_first_pass_capacity_bound_follows_the_model(plan, n):
    for s, z in itertools.product(range(1, 6), (0, 25, 60)):
        for bits in (18, 15):  # 9 and 8 bits in the first pass
            p = plan({"RJ_TUNE_SPEC_SAMPLE": s, "RJ_TUNE_SPEC_Z": z}, n, 1, 1, bits)
            assert p["spec_cap_max"] == _specref.cap_max(n, p["pbits"][0], s, z), (n, s, z, bits)


def test_first_pass_group_size_follows_the_model(plan):
    for n in (0, 1, 1029, 16384 * 4096, 16384 * 4096 + 1, 3 * 16384 * 4096 + 5, 1 << 30, (1 << 32) - 16):
        p = plan({}, n, 1, 1, 18)
        assert p["tpg_first"] == _specref.tiles_per_group(n) == p["pass"][0]["tiles_per_group"], n
    assert plan({"RJ_TUNE_TPG1": 3}, N, 1, 1, 18)["tpg_first"] == 3


# ------------------------------------------------------------------------------------------------- the decision table
def test_one_pass_packed(plan):
    p = plan({}, 1000, 1, 1, 8, flag_word=True, spec2_ok=True)
    assert p["pbits"] == [8] and (p["mid"], p["last"]) == ("packed", "packed")
    assert not (p["fine"] or p["fine_xcd"] or p["spec"] or p["spec2"])
    assert (p["pass"][0]["offsets"], p["pass"][0]["hist"], p["pass"][0]["scatter"]) == ("hist", "src", "src_packed")


def test_14_bits_fine_packed(plan):
    p = plan({}, N, 1, 1, 14)
    assert p["pbits"] == [7, 7] and p["fine"] and (p["mid"], p["last"]) == ("packed", "packed")
    assert [ps["offsets"] for ps in p["pass"]] == ["fine", "fine"]
    assert [ps["hist"] for ps in p["pass"]] == ["fine_src", "none"]
    assert [ps["scatter"] for ps in p["pass"]] == ["src_packed", "packed"]
    assert p["fine_grid"] == 64 and not p["fine_xcd"]  # 64 tiles, below RJ_TUNE_XCD_MIN_ROWS


def test_18_bits_blocked_between_passes(plan):
    for flag in (False, True):
        p = plan({}, N, 1, 1, 18, flag_word=flag, spec2_ok=flag)
        assert p["pbits"] == [9, 9] and not p["fine"] and (p["mid"], p["last"]) == ("blocked", "packed")
        assert [(ps["xcd_log2"], ps["xcd_remap"]) for ps in p["pass"]] == [(0, 0), (0, 0)]
        assert not p["spec"] and not p["spec2"]
        assert [ps["hist"] for ps in p["pass"]] == ["src", "blocked"]
        assert [ps["scatter"] for ps in p["pass"]] == ["src_packed", "blocked"]


@pytest.mark.parametrize("spec2_ok", [False, True])
def test_18_bits_speculative(plan, spec2_ok):
    p = plan(MIN_ROWS_0, N, 1, 1, 18, flag_word=True, spec2_ok=spec2_ok)
    assert p["spec"] and p["spec2"] == spec2_ok and p["mid"] == "blocked"
    assert p["pass"][0]["offsets"] == "sample" and p["pass"][0]["hist"] == "sample_src"
    assert p["pass"][1]["offsets"] == ("sample" if spec2_ok else "hist")
    assert p["pass"][1]["hist"] == ("last_sample" if spec2_ok else "blocked")
    assert p["pass"][1]["scatter"] == ("last_blocked" if spec2_ok else "blocked")
    assert p["pass"][1]["nseg_in"] == 8 << 9 and p["pass"][1]["n_oseg"] == 1 << 9
    assert not plan(MIN_ROWS_0, N, 1, 1, 18, spec2_ok=True)["spec"]  # no flag word
    p = plan(dict(MIN_ROWS_0, RJ_TUNE_BLOCKED_MID=0), N, 1, 1, 18, flag_word=True, spec2_ok=spec2_ok)
    assert p["spec"] and not p["spec2"] and p["mid"] == "packed"


@pytest.mark.parametrize("spec2_ok", [False, True])
def test_two_word_carry_18_bits(plan, spec2_ok):
    p = plan(MIN_ROWS_0, N, 1, 2, 18, flag_word=True, spec2_ok=spec2_ok)
    assert (p["mid"], p["last"]) == ("dense", "aos3")  # key + pair arrays between the passes
    assert p["spec"] and p["spec2"] == spec2_ok
    assert [ps["scatter"] for ps in p["pass"]] == ["src", "last_dense" if spec2_ok else "dense"]


def test_two_word_carry_14_bits(plan):
    p = plan({}, N, 1, 2, 14)
    assert p["fine"] and (p["mid"], p["last"]) == ("aos3", "aos3")
    assert [ps["scatter"] for ps in p["pass"]] == ["src", "aos3"]


def test_two_word_carry_aos_mid_knob(plan):
    p = plan(dict(MIN_ROWS_0, RJ_TUNE_AOS_MID=1), N, 1, 2, 18, flag_word=True, spec2_ok=True)
    assert (p["mid"], p["last"]) == ("aos3_side", "aos3") and not p["spec"] and not p["spec2"]
    assert [ps["hist"] for ps in p["pass"]] == ["src", "digits"]
    p = plan(dict(MIN_ROWS_0, RJ_TUNE_AOS_MID=3), N, 1, 2, 18, flag_word=True, spec2_ok=True)
    assert (p["mid"], p["last"]) == ("aos3", "aos3") and not p["spec"]
    assert [ps["hist"] for ps in p["pass"]] == ["src", "aos3"]


def test_two_key_words_dense(plan):
    p = plan(MIN_ROWS_0, N, 2, 1, 18, flag_word=True, spec2_ok=True)
    assert (p["mid"], p["last"]) == ("dense", "dense") and p["spec"] and not p["spec2"]
    assert not plan(MIN_ROWS_0, N, 2, 1, 18)["spec"]


def test_packed_side_knob(plan):
    p = plan({"RJ_TUNE_PACKED_SIDE": 1, "RJ_TUNE_XCD_MIN_ROWS": 0, "RJ_TUNE_SPEC_MIN_ROWS": 0}, N, 1, 1, 18, flag_word=True)
    assert p["mid"] == "packed_side" and not p["spec"]
    assert [ps["hist"] for ps in p["pass"]] == ["src", "digits"]


def test_chunked_second_pass_knob(plan):
    p = plan({"RJ_TUNE_MALL_CHUNK": 8, "RJ_TUNE_XCD_MIN_ROWS": 0, "RJ_TUNE_SPEC_MIN_ROWS": 0}, N, 1, 1, 18, flag_word=True)
    assert p["mid"] == "packed" and not p["spec"]
    assert [ps["offsets"] for ps in p["pass"]] == ["hist", "chunked"]
    assert [ps["scatter"] for ps in p["pass"]] == ["src_packed", "packed"]
    # ... and only there: below RJ_TUNE_XCD_MIN_ROWS the pass runs in one launch, from blocked pairs
    p = plan({"RJ_TUNE_MALL_CHUNK": 8}, N, 1, 1, 18)
    assert p["mid"] == "blocked" and [ps["offsets"] for ps in p["pass"]] == ["hist", "hist"]


def test_pack_knob(plan):
    assert plan({"RJ_TUNE_PACK": 2}, N, 1, 1, 14)["last"] == "packed"
    assert plan({"RJ_TUNE_PACK": 2}, N, 1, 1, 18)["last"] == "dense"
    for bits in (8, 14, 18, 27):
        p = plan({"RJ_TUNE_PACK": 0}, N, 1, 1, bits)
        assert (p["mid"], p["last"]) == ("dense", "dense")


def test_p1_bits_knob(plan):
    assert plan({"RJ_TUNE_P1_BITS": 8}, N, 1, 1, 17)["pbits"] == [8, 9]
    assert plan({"RJ_TUNE_P1_BITS": 8}, N, 1, 1, 19)["pbits"] == [7, 6, 6]  # three passes: the knob is ignored


def test_later_pass_group_size(plan):
    # 2^21 tuples per segment: eight tiles per group; the last pass of 12-byte-tuple plans takes at most two
    assert [ps["tiles_per_group"] for ps in plan({}, 1 << 30, 1, 1, 18)["pass"]] == [8, 8]
    assert [ps["tiles_per_group"] for ps in plan({}, 1 << 30, 1, 2, 18)["pass"]] == [8, 2]
    assert [ps["tiles_per_group"] for ps in plan({"RJ_TUNE_TPG2": 5}, 1 << 30, 1, 2, 18)["pass"]] == [8, 5]
    p = plan({}, N, 1, 1, 18)["pass"]
    assert p[0]["n_groups"] == 64 and p[1]["n_groups"] == 64 + 512  # exact; n / (tiles * 16384) + segments


# --------------------------------------------------------------------------- requests that switch speculation off
@pytest.mark.parametrize("cw", [1, 2])
def test_requests_that_never_speculate(plan, cw):
    base = dict(flag_word=True, spec2_ok=True)
    assert plan(MIN_ROWS_0, N, 1, cw, 18, **base)["spec"]
    for bits in (14, 18):
        for how in (dict(external=True, single_pass=True), dict(external=True), dict(single_pass=True), dict(word_source=1),
                    dict(composite=True), dict(composite=True, single_pass=True), dict(preseg=(8, 2)), dict(after_offsets=True)):
            p = plan(MIN_ROWS_0, N, 1, cw, 9 if how.get("single_pass") else bits, **base, **how)
            assert not p["spec"] and not p["spec2"], how
            assert p["n_first_out"] == N and p["n_last_out"] == N
            assert all(ps["offsets"] in ("fine", "hist") for ps in p["pass"]), how
            # the fine histogram counts one segment of a source into arrays of the call's own
            if "external" in how or "single_pass" in how or "composite" in how or "preseg" in how:
                assert not p["fine"], how
            else:
                assert p["fine"] == (bits == 14), how


def test_a_packed_word_source_stays_packed(plan):
    for pack in (0, 1, 2):
        for bits in (8, 14, 18):
            p = plan({"RJ_TUNE_PACK": pack}, N, 1, 1, bits, word_source=2)
            assert p["last"] == "packed" and p["mid"] in ("packed",), (pack, bits)
            assert p["pass"][0]["hist"] == ("fine_words" if bits == 14 else "packed")
            assert plan({"RJ_TUNE_PACK": pack}, N, 1, 1, bits, word_source=1)["last"] == "dense"


def test_a_presegmented_first_pass_reads_its_runs(plan):
    p = plan({}, N, 1, 1, 12, shift0=3, word_source=2, preseg=(32, 8))
    assert p["pbits"] == [6, 6] and not p["fine"]
    assert (p["pass"][0]["nseg_in"], p["pass"][0]["n_oseg"], p["pass"][0]["bins"]) == (32, 8, 8 << 6)
    assert (p["pass"][1]["nseg_in"], p["pass"][1]["n_oseg"], p["pass"][1]["bins"]) == (8 << 6, 8 << 6, 8 << 12)


def test_bad_requests_are_refused():
    for bad in (dict(kw=0), dict(kw=3), dict(kw=2, cw=3), dict(bits=33), dict(bits=10, single_pass=True), dict(kw=1, cw=2, word_source=2)):
        with pytest.raises(capi.RjError) as e:
            capi.partition_plan(N, **dict(dict(kw=1, cw=1, bits=8), **bad))
        assert e.value.code == 1  # RJ_ERR_ARG


# ---------------------------------------------------------------------------------------------- invariants, swept
SETTINGS = [{}, MIN_ROWS_0, dict(MIN_ROWS_0, RJ_TUNE_BLOCKED_MID=0), dict(MIN_ROWS_0, RJ_TUNE_AOS_MID=1), dict(MIN_ROWS_0, RJ_TUNE_AOS_MID=3),
            {"RJ_TUNE_PACKED_SIDE": 1, "RJ_TUNE_XCD_MIN_ROWS": 0}, dict(MIN_ROWS_0, RJ_TUNE_PACKED_SIDE=1),
            {"RJ_TUNE_MALL_CHUNK": 8, "RJ_TUNE_XCD_MIN_ROWS": 0}, dict(MIN_ROWS_0, RJ_TUNE_MALL_CHUNK=8), dict(MIN_ROWS_0, RJ_TUNE_PACK=2),
            dict(MIN_ROWS_0, RJ_TUNE_PACK=0), dict(MIN_ROWS_0, RJ_TUNE_P1_BITS=8), dict(MIN_ROWS_0, RJ_TUNE_AOS3=0),
            dict(MIN_ROWS_0, RJ_TUNE_FINE=0), dict(MIN_ROWS_0, RJ_TUNE_XCD_SPLIT=0)]
SHAPES = [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2)]


@pytest.mark.parametrize("knobs", SETTINGS, ids=lambda k: ",".join(f"{a[8:]}={b}" for a, b in k.items()) or "defaults")
def test_invariants_over_a_sweep(plan, knobs):
    for (kw, cw), bits, n, flag, ok2 in itertools.product(SHAPES, range(28), (N, (1 << 31) + 5), (False, True), (False, True)):
        p = plan(knobs, n, kw, cw, bits, flag_word=flag, spec2_ok=ok2)
        what = (kw, cw, bits, n, flag, ok2)
        # one between-pass layout, and it is one the last pass' layout goes with
        assert (p["mid"] in PACKED_MIDS) == (p["last"] == "packed"), what
        assert p["mid"] not in AOS_MIDS or p["last"] == "aos3", what
        assert p["mid"] in ("dense", "packed") or p["passes"] >= 2, what
        assert p["last"] != "packed" or (kw, cw) == (1, 1), what
        assert p["last"] != "aos3" or (kw, cw) == (1, 2), what
        chunked = [ps["offsets"] == "chunked" for ps in p["pass"]]
        assert not any(chunked) or (chunked == [False, True] and p["mid"] == "packed"), what
        assert [ps["offsets"] == "fine" for ps in p["pass"]] == [p["fine"]] * p["passes"], what
        assert not p["fine_xcd"] or p["fine"], what
        # speculation
        assert p["spec"] or not p["spec2"], what
        if p["spec"]:
            assert flag and p["passes"] == 2 and not p["fine"], what
            assert p["pass"][0]["xcd_log2"] == 3 and p["pass"][1]["xcd_remap"] == 1, what
            assert p["spec_cap_max"] < 1 << 31 and p["n_first_out"] == p["spec_cap_max"] + 16384, what
            assert p["mid"] in ("dense", "packed", "blocked"), what
        else:
            assert p["n_first_out"] == n, what
        if p["spec2"]:
            assert ok2 and p["spec2_cap_max"] < 1 << 31 and p["n_last_out"] == p["spec2_cap_max"] + 16384, what
            assert p["last"] == "aos3" or p["mid"] == "blocked", what
        else:
            assert p["n_last_out"] == n, what
        assert (p["pass"][0]["offsets"] == "sample") == p["spec"], what
        assert (p["passes"] > 1 and p["pass"][1]["offsets"] == "sample") == p["spec2"], what
        # geometry
        nseg = 1
        for i, ps in enumerate(p["pass"]):
            assert ps["n_oseg"] == nseg and ps["bins"] == nseg << ps["bits"], what
            assert ps["nseg_in"] == (nseg << 3 if i == 1 and p["spec"] else nseg), what
            assert 1 <= ps["tiles_per_group"] <= 8, what
            nseg = ps["bins"]
        assert nseg == 1 << bits, what
