"""The nine kernels of csrc/ca_damage.hip — ca_ensemble_damage_{vn,moore,clustered}64 and their _torus and _closed forms — hold a
universe and its perturbed twin (in registers beside the von Neumann step, parked in LDS beside the other two) and a step policy with its
leaves in registers, 1024 threads a workgroup: no scratch, nothing spilled, at most 128 VGPRs (1024 threads are four waves a SIMD of 512
registers) and at most 163 840 B of static LDS, what a workgroup may hold on gfx950. The file holds those nine kernels and no others.
Read out of the kernel metadata of the gfx950 assembly, built with the Makefile's compiler and flags. It needs hipcc, no GPU."""
import re

import pytest

import codegen_lib as cg

KERNELS = tuple(kind + boundary for kind in ("vn64", "moore64", "clustered64") for boundary in ("", "_torus", "_closed"))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of ca_damage.hip."""
    assert re.search(r"^OBJS\s*:=.*\bca_damage\.o\b", cg.makefile(), re.M)
    lst = cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_damage"])
    return cg.kernel_metadata(lst["ca_damage"])


def test_the_nine_kernels_and_no_others(kernels):
    for name in KERNELS:
        cg.one_kernel(kernels, r"\d+ca_ensemble_damage_%sE" % name)
    assert len(kernels) == len(KERNELS) == 9, sorted(kernels)


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_resources(kernels, name):
    k = cg.one_kernel(kernels, r"\d+ca_ensemble_damage_%sE" % name)
    print("ca_ensemble_damage_" + name, k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] <= 163840
