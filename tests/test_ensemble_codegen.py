"""The three *_moving ensemble kernels (ca_ensemble.hip) are launched with 1024 threads and four waves a SIMD: 128 vector registers at
most, none spilled, no scratch — what a check point adds must not stay in registers across the steps. Read out of the metadata of the
gfx950 assembly, built with the Makefile's compiler and flags. It needs hipcc, no GPU."""
import pytest

import codegen_lib as cg

KERNELS = ["ca_ensemble_vn64_moving", "ca_ensemble_moore64_moving", "ca_ensemble_clustered64_moving"]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of ca_ensemble.hip."""
    return cg.kernel_metadata(cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_ensemble"])["ca_ensemble"])


@pytest.mark.parametrize("kernel", KERNELS)
def test_moving_kernels_fit_four_waves_a_simd(kernels, kernel):
    k = cg.one_kernel(kernels, r"\d+%sE" % kernel)
    print(kernel, "vgpr_count", k["vgpr_count"], "sgpr_count", k["sgpr_count"])
    assert k["vgpr_count"] <= 128
    assert k["vgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
