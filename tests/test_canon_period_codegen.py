"""The three kernels of csrc/ca_canon_period.hip — ca_ensemble_canon_period_vn64, _moore64, _clustered64 — hold a universe, the
orientation pass of ca_canon.hip and a step policy with its leaves in registers, 1024 threads a workgroup: no scratch, nothing spilled,
at most 128 VGPRs (1024 threads are four waves a SIMD of 512 registers) and at most 163 840 B of static LDS, what a workgroup may hold
on gfx950 — one parity of the step's exchange, compose's image, the digests' shares, the kept rows. The file holds those three kernels
and no others. Read out of the kernel metadata of the gfx950 assembly, built with the Makefile's compiler and flags. It needs hipcc, no
GPU."""
import re

import pytest

import codegen_lib as cg

KINDS = ("vn64", "moore64", "clustered64")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of ca_canon_period.hip."""
    assert re.search(r"^OBJS\s*:=.*\bca_canon_period\.o\b", cg.makefile(), re.M)
    lst = cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_canon_period"])
    return cg.kernel_metadata(lst["ca_canon_period"])


def test_the_three_kernels_and_no_others(kernels):
    for kind in KINDS:
        cg.one_kernel(kernels, r"\d+ca_ensemble_canon_period_%sE" % kind)
    assert len(kernels) == len(KINDS), sorted(kernels)


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_resources(kernels, kind):
    k = cg.one_kernel(kernels, r"\d+ca_ensemble_canon_period_%sE" % kind)
    print("ca_ensemble_canon_period_" + kind, k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] <= 163840
