"""The nine kernels of csrc/ca_usage.hip — ca_ensemble_usage_{vn,moore,clustered}64 and their _torus and _closed forms — hold a
universe in LDS, both step parities, and one packed accumulator register a bin beside a step body of their own, 1024 threads a
workgroup: no scratch, nothing spilled, at most 128 VGPRs (1024 threads are four waves a SIMD of 512 registers) and at most 163 840 B
of static LDS, what a workgroup may hold on gfx950. The file holds those nine kernels and no others. The measured numbers are pinned:
README and DESIGN 12.17 quote them. Read out of the kernel metadata of the gfx950 assembly, built with the Makefile's compiler and
flags. It needs hipcc, no GPU."""
import os
import re

import pytest

import codegen_lib as cg

KERNELS = tuple(kind + boundary for kind in ("vn64", "moore64", "clustered64") for boundary in ("", "_torus", "_closed"))
# vector registers (the largest of a kind's three kernels) and static LDS bytes, as README and DESIGN 12.17 quote them
PINNED = {"vn64": (38, 66824), "moore64": (76, 69384), "clustered64": (128, 72200)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of ca_usage.hip."""
    assert re.search(r"^OBJS\s*:=.*\bca_usage\.o\b", cg.makefile(), re.M)
    lst = cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_usage"])
    return cg.kernel_metadata(lst["ca_usage"])


def test_the_nine_kernels_and_no_others(kernels):
    for name in KERNELS:
        cg.one_kernel(kernels, r"\d+ca_ensemble_usage_%sE" % name)
    assert len(kernels) == len(KERNELS) == 9, sorted(kernels)


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_resources(kernels, name):
    k = cg.one_kernel(kernels, r"\d+ca_ensemble_usage_%sE" % name)
    print("ca_ensemble_usage_" + name, k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] <= 163840


@pytest.mark.parametrize("kind", sorted(PINNED))
def test_the_numbers_the_documents_quote(kernels, kind):
    three = [cg.one_kernel(kernels, r"\d+ca_ensemble_usage_%s%sE" % (kind, b)) for b in ("", "_torus", "_closed")]
    vgprs, lds = max(k["vgpr_count"] for k in three), {k["group_segment_fixed_size"] for k in three}
    assert (vgprs, lds) == (PINNED[kind][0], {PINNED[kind][1]})
    quoted = "%d VGPRs, %s B" % (vgprs, format(PINNED[kind][1], ",").replace(",", " "))
    for doc in ("README.md", "DESIGN.md"):
        lines = [line for line in open(os.path.join(cg.ROOT, doc)).read().splitlines() if "ca_ensemble_usage_" + kind in line]
        assert any(quoted in line for line in lines), (doc, kind, quoted)
