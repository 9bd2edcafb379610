"""The window kernels (csrc/ca_window.hip) are a thread a row with three grid words and one universe row in registers: the unit is in
OBJS, it holds exactly its four kernels — cut, stamp (or / erase) and clear — and each has no scratch, nothing spilled, at most 128
VGPRs and no LDS. Read out of the kernel metadata of the gfx950 assembly, built with the Makefile's compiler and flags. It needs
hipcc, no GPU."""
import re

import pytest

import codegen_lib as cg

KERNELS = {
    "cut": r"\d+ca_window_cutE",
    "or": r"\d+ca_window_stampILb0EE",
    "erase": r"\d+ca_window_stampILb1EE",
    "clear": r"\d+ca_window_clearE",
}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    assert re.search(r"^OBJS\s*:=.*\bca_window\.o\b", cg.makefile(), re.M)
    return cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_window"])["ca_window"]


@pytest.fixture(scope="module")
def kernels(listing):
    return cg.kernel_metadata(listing)


def test_unit_holds_exactly_its_kernels(kernels):
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for pattern in KERNELS.values():
        cg.one_kernel(kernels, pattern)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_window_kernel_resources(kernels, name):
    k = cg.one_kernel(kernels, KERNELS[name])
    print("ca_window", name, k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] == 0


def test_overlaps_go_through_vector_atomics_and_the_cut_through_none(listing):
    """Windows of a stamp share grid words: every write to the grid is a global atomic whose result is not used; a cut writes universe
    words once each and needs none."""
    bodies = {}
    for name, pattern in KERNELS.items():
        m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)s_endpgm" % pattern, listing, re.S | re.M)
        assert m, name
        bodies[name] = m.group(2)
    assert "global_atomic" not in bodies["cut"] and bodies["cut"].count("global_store_dwordx2") == 2
    assert "global_atomic_or" in bodies["or"] and "global_store" not in bodies["or"]
    for name in ("erase", "clear"):
        assert "global_atomic_and" in bodies[name] and "global_store" not in bodies[name]
