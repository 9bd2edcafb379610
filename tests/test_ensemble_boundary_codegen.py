"""The 24 ensemble kernels of the torus and the closed cube (ca_ensemble_boundary.hip) are launched like their reference siblings of
ca_ensemble.hip, with 1024 threads and four waves a SIMD: 128 vector registers at most, none spilled, no scratch, and the LDS of the
sibling — a boundary changes operands of a step, not what a workgroup holds. Read out of the metadata of the gfx950 assembly, built
with the Makefile's compiler and flags. It needs hipcc, no GPU."""
import pytest

import codegen_lib as cg

SIBLINGS = ["ca_ensemble_%s64%s" % (kind, form) for kind in ("vn", "moore", "clustered") for form in ("", "_cycle", "_trace", "_moving")]
BOUNDARIES = ("torus", "closed")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{unit: {symbol: {field: value}}} of the two units, compiled side by side."""
    units = ["ca_ensemble", "ca_ensemble_boundary"]
    got = cg.listings(tmp_path_factory.mktemp("codegen"), units)
    return {u: cg.kernel_metadata(got[u]) for u in units}


def test_the_unit_holds_the_24_kernels_and_nothing_else(kernels):
    assert len(kernels["ca_ensemble_boundary"]) == len(SIBLINGS) * len(BOUNDARIES) == 24
    assert len(kernels["ca_ensemble"]) == 12


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("sibling", SIBLINGS)
def test_boundary_kernels_fit_four_waves_a_simd(kernels, sibling, boundary):
    k = cg.one_kernel(kernels["ca_ensemble_boundary"], r"\d+%s_%sE" % (sibling, boundary))
    ref = cg.one_kernel(kernels["ca_ensemble"], r"\d+%sE" % sibling)
    print(sibling, boundary, "vgpr_count", k["vgpr_count"], "sgpr_count", k["sgpr_count"], "lds", k["group_segment_fixed_size"], "| reference vgpr_count",
          ref["vgpr_count"])
    assert k["vgpr_count"] <= 128
    assert k["vgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] == ref["group_segment_fixed_size"]
