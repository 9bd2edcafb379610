"""ca_ensemble_compose64 (csrc/ca_compose.hip) holds the destination being built and the piece being staged in registers, 1024 threads
a workgroup: no scratch, nothing spilled, at most 128 VGPRs (1024 threads are four waves a SIMD of 512 registers) and at most 64 KiB of
static LDS — the image of one piece, padded to 65 words a plane of rows, and the waves' partials. Read out of the kernel metadata of
the gfx950 assembly, built with the Makefile's compiler and flags. It needs hipcc, no GPU."""
import re

import pytest

import codegen_lib as cg


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of ca_compose.hip."""
    assert re.search(r"^OBJS\s*:=.*\bca_compose\.o\b", cg.makefile(), re.M)
    return cg.kernel_metadata(cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_compose"])["ca_compose"])


def test_compose_kernel_resources(kernels):
    hits = [n for n in kernels if re.search(r"\d+ca_ensemble_compose64E", n)]
    assert len(hits) == 1 and len(kernels) == 1, sorted(kernels)
    k = kernels[hits[0]]
    print("ca_ensemble_compose64", k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] <= 65536
