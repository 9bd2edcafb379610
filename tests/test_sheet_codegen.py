"""ca_render_sheet64 (csrc/render_sheet.hip) keeps one 64^3 universe in LDS and must leave room for four workgroups on a CU: between
32 768 (the universe) and 40 960 bytes of LDS, and — it drops the legacy, skip and indirect branches of the plain kernel — no more
spilled registers and no more scratch than ca_render_packed<false> (csrc/render.hip) in the same run. Read out of the metadata of the
gfx950 assembly, built with the Makefile's compiler and flags plus the renderer's -ffp-contract=off. It needs hipcc, no GPU."""
import re

import pytest

import codegen_lib as cg


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of render_sheet.hip and render.hip."""
    mk = cg.makefile()
    assert re.search(r"^render_sheet\.o:.*\n\t.*-ffp-contract=off", mk, re.M), "render_sheet.o is built without -ffp-contract=off"
    assert re.search(r"^OBJS\s*:=.*\brender_sheet\.o\b", mk, re.M)
    found = {}
    for listing in cg.listings(tmp_path_factory.mktemp("codegen"), ["render_sheet", "render"], ["-ffp-contract=off"]).values():
        found.update(cg.kernel_metadata(listing))
    return found


def test_sheet_kernel_fits_four_workgroups_a_cu(kernels):
    sheet = cg.one_kernel(kernels, r"\d+ca_render_sheet64E")
    plain = cg.one_kernel(kernels, r"\d+ca_render_packedILb0EE")  # ca_render_packed<false>
    print("ca_render_sheet64", sheet)
    print("ca_render_packed<false>", plain)
    assert 32768 <= sheet["group_segment_fixed_size"] <= 40960
    assert sheet["vgpr_spill_count"] <= plain["vgpr_spill_count"]
    assert sheet["private_segment_fixed_size"] <= plain["private_segment_fixed_size"]
