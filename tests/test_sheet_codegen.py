"""ca_render_sheet64 (csrc/render_sheet.hip) keeps one 64^3 universe in LDS and must leave room for four workgroups on a CU: between
32 768 (the universe) and 40 960 bytes of LDS, and — it drops the legacy, skip and indirect branches of the plain kernel — no more
spilled registers and no more scratch than ca_render_packed<false> (csrc/render.hip) in the same run. Read out of the metadata of the
gfx950 assembly, built with the Makefile's compiler and flags plus the renderer's -ffp-contract=off. It needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellularautomatons3d_amd", "csrc")
FIELDS = ["group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count"]


def _make_var(text, name):
    m = re.search(r"^%s\s*\?=\s*(.*)$" % name, text, re.M)
    assert m, f"{name} not found in csrc/Makefile"
    return m.group(1).strip()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: {field: value}} of every kernel of render_sheet.hip and render.hip."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or _make_var(mk, "HIPCC")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is not installed")
    assert re.search(r"^render_sheet\.o:.*\n\t.*-ffp-contract=off", mk, re.M), "render_sheet.o is built without -ffp-contract=off"
    assert re.search(r"^OBJS\s*:=.*\brender_sheet\.o\b", mk, re.M)
    arch = _make_var(mk, "ARCH")
    flags = _make_var(mk, "CXXFLAGS").split() + ["-ffp-contract=off"]
    tmp = tmp_path_factory.mktemp("codegen")
    procs = []
    for stem in ("render_sheet", "render"):
        cmd = [hipcc, f"--offload-arch={arch}"] + flags + ["--cuda-device-only", "-S", stem + ".hip", "-o", str(tmp / (stem + ".s"))]
        procs.append(subprocess.Popen(cmd, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL))
    assert [p.wait() for p in procs] == [0, 0]
    found = {}
    for stem in ("render_sheet", "render"):
        listing = (tmp / (stem + ".s")).read_text()
        meta = listing[listing.index("amdhsa.kernels"):]
        for e in ("." + e for e in meta.split("  - .")):
            m = re.search(r"\.name:\s+(\w+)", e)
            if m and re.search(r"\.vgpr_count:", e):
                found[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, e).group(1)) for f in FIELDS}
    return found


def _one(kernels, pattern):
    hits = [n for n in kernels if re.search(pattern, n)]
    assert len(hits) == 1, (pattern, sorted(kernels))
    return kernels[hits[0]]


def test_sheet_kernel_fits_four_workgroups_a_cu(kernels):
    sheet = _one(kernels, r"\d+ca_render_sheet64E")
    plain = _one(kernels, r"\d+ca_render_packedILb0EE")  # ca_render_packed<false>
    print("ca_render_sheet64", sheet)
    print("ca_render_packed<false>", plain)
    assert 32768 <= sheet["group_segment_fixed_size"] <= 40960
    assert sheet["vgpr_spill_count"] <= plain["vgpr_spill_count"]
    assert sheet["private_segment_fixed_size"] <= plain["private_segment_fixed_size"]
