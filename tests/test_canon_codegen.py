"""ca_ensemble_canon64 (csrc/ca_canon.hip) holds the universe's rows of T_0 and of the orientation under way in registers, 1024
threads a workgroup: no scratch, nothing spilled, at most 128 VGPRs (1024 threads are four waves a SIMD of 512 registers) and at most
64 KiB of static LDS — compose's image of the universe, the waves' shares of the 48 digests and the partials. ca_canon.hip holds that
one kernel, and ca_compose.hip keeps its one. Read out of the kernel metadata of the gfx950 assembly, built with the Makefile's
compiler and flags. It needs hipcc, no GPU."""
import re

import pytest

import codegen_lib as cg


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{stem: {symbol: {field: value}}} of every kernel of ca_canon.hip and ca_compose.hip."""
    assert re.search(r"^OBJS\s*:=.*\bca_canon\.o\b", cg.makefile(), re.M)
    lst = cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_canon", "ca_compose"])
    return {stem: cg.kernel_metadata(text) for stem, text in lst.items()}


def test_canon_kernel_resources(kernels):
    ks = kernels["ca_canon"]
    hits = [n for n in ks if re.search(r"\d+ca_ensemble_canon64E", n)]
    assert len(hits) == 1 and len(ks) == 1, sorted(ks)
    k = ks[hits[0]]
    print("ca_ensemble_canon64", k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] <= 65536


def test_compose_keeps_its_one_kernel(kernels):
    ks = kernels["ca_compose"]
    assert len(ks) == 1 and re.search(r"\d+ca_ensemble_compose64E", next(iter(ks))), sorted(ks)
