"""The kernel handles of the speculative last pass compiled into librj.so (tests/_elfsyms.py, no GPU), against the
table of test_gpu_spec_pass2.py — what test_kernel_symbols.py does for the first pass' table: every compiled
instantiation of the k_last_* families is expected by some row of the GPU file, and every name a row expects is
compiled."""
import os

import pytest

import _elfsyms
import test_gpu_spec_pass2 as sp2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "radix-join_amd", "librj.so")


@pytest.fixture(scope="module")
def compiled():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    return set(map(_elfsyms.short_name, _elfsyms.kernel_handles(LIB)))


def test_every_compiled_instantiation_is_expected_by_a_row(compiled):
    scope = {n for n in compiled if n.split("<")[0] in sp2.FAMILIES}
    assert scope, "no k_last_* kernel handle in librj.so"
    assert not scope - sp2.expected_instantiations(), sorted(scope - sp2.expected_instantiations())


def test_every_expected_name_is_compiled(compiled):
    missing = sorted(sp2.expected_instantiations() - compiled)
    assert not missing, missing
    for name in sp2.expected_instantiations():
        assert name.split("<")[0] in sp2.FAMILIES, name
