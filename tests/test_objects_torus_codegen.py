"""ca_ensemble_census64_torus and ca_ensemble_isolate64_torus (csrc/ca_objects_torus.hip) hold a universe and the object being filled
in registers, 1024 threads a workgroup, as the closed kernels do: the unit is built into the library, it holds exactly those two
kernels, and each has no scratch, nothing spilled, at most 128 VGPRs and at most 64 KiB of LDS. Read out of the kernel metadata of the
gfx950 assembly, built with the Makefile's compiler and flags. It needs hipcc, no GPU."""
import re

import pytest

import codegen_lib as cg


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of ca_objects_torus.hip."""
    assert re.search(r"^OBJS\s*:=.*\bca_objects_torus\.o\b", cg.makefile(), re.M)
    return cg.kernel_metadata(cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_objects_torus"])["ca_objects_torus"])


def test_the_unit_holds_the_two_kernels(kernels):
    names = sorted(re.search(r"\d+(ca_ensemble_\w+?64_torus)E", n).group(1) for n in kernels)
    assert names == ["ca_ensemble_census64_torus", "ca_ensemble_isolate64_torus"], sorted(kernels)


@pytest.mark.parametrize("name", ["ca_ensemble_census64_torus", "ca_ensemble_isolate64_torus"])
def test_kernel_resources(kernels, name):
    hits = [n for n in kernels if re.search(r"\d+" + name + "E", n)]
    assert len(hits) == 1, sorted(kernels)
    k = kernels[hits[0]]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] <= 65536
