"""The kernel handles compiled into librj.so (tests/_elfsyms.py, no GPU): every kernel family of
the join path is there, the compact names agree with c++filt, and the kernel matrix
(test_gpu_kernel_matrix.py) names only instantiations that exist and covers all of them; so does the table of the
speculative first pass (test_gpu_spec_matrix.py) for its three families."""
import os
import shutil

import pytest

import _elfsyms
import test_gpu_kernel_matrix as km
import test_gpu_spec_matrix as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "radix-join_amd", "librj.so")


@pytest.fixture(scope="module")
def handles():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    return _elfsyms.kernel_handles(LIB)


def test_reader_finds_every_kernel_family(handles):
    fams = {_elfsyms.family(h) for h in handles}
    for f in km.FAMILIES + ("k_heavy_tasks", "k_scan_fine", "k_gather", "k_decode_pages", "k_finish_streams"):
        assert f in fams, f"no {f} kernel handle in librj.so"
    # several instantiations per templated family
    by = {}
    for h in handles:
        by.setdefault(_elfsyms.family(h), []).append(h)
    assert len(by["k_join"]) > 60 and len(by["k_join_bcast"]) == 25 and len(by["k_fine_hist"]) == 4


def test_offsets_resolve_to_their_symbols(handles):
    objs = _elfsyms.dynsym_objects(LIB)
    for h in handles[:10]:
        assert _elfsyms.symbol_at(LIB, objs[h]) == h


def test_short_names_agree_with_cxxfilt(handles):
    if not shutil.which("c++filt"):
        pytest.skip("c++filt is not on the PATH")
    for h in handles:
        want = _elfsyms.readable(h).replace(" ", "").replace("rj::", "")
        assert _elfsyms.short_name(h) == want


def test_matrix_names_only_compiled_instantiations(handles):
    compiled = set(map(_elfsyms.short_name, handles))
    for name in km.UNREACHABLE:
        assert name in compiled, f"UNREACHABLE names {name}, which librj.so does not compile"
    for c in km.CASES:
        for name in c.expect:
            assert name in compiled, f"row {c.id} expects {name}, which librj.so does not compile"


def test_matrix_rows_cover_every_compiled_instantiation(handles):
    """Statically: the rows' expectations plus UNREACHABLE account for every in-scope instantiation
    (the GPU test then checks that the rows really reach them)."""
    scope = {n for n in map(_elfsyms.short_name, handles) if n.split("<")[0] in km.FAMILIES}
    named = {e for c in km.CASES for e in c.expect}
    assert not scope - named - set(km.UNREACHABLE), sorted(scope - named - set(km.UNREACHABLE))
    assert not named & set(km.UNREACHABLE)


def test_speculative_matrix_names_exactly_the_compiled_instantiations(handles):
    """The same two checks for the speculative first pass (test_gpu_spec_matrix.py): every name a row expects is
    compiled, and every compiled k_pass_sample / k_spec_scatter / k_spec_scatter_packed is named by some row.  All of
    them are reachable: there is no UNREACHABLE list."""
    assert sm.FAMILIES == ("k_pass_sample", "k_spec_scatter", "k_spec_scatter_packed")
    assert not hasattr(sm, "UNREACHABLE")
    compiled = set(map(_elfsyms.short_name, handles))
    for c in sm.CASES:
        for name in c.expect:
            assert name in compiled, f"row {c.id} expects {name}, which librj.so does not compile"
        for name in c.expect[:-1]:
            assert sm.exact_of(name) in compiled, f"row {c.id}: no exact kernel {sm.exact_of(name)}"
    for name in sm.VARCHAR_EXPECT:
        assert name in compiled, f"the VARCHAR row expects {name}, which librj.so does not compile"
    scope = {n for n in compiled if n.split("<")[0] in sm.FAMILIES}
    assert scope == set(sm.compiled_in_scope())
    # (without the VARCHAR row: it repeats a shape, a table row must name it too)
    named = {e for c in sm.CASES for e in c.expect}
    assert not scope - named, sorted(scope - named)
    assert len(scope) == 14
