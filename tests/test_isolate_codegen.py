"""ca_ensemble_isolate64 (csrc/ca_isolate.hip) holds a universe and the object being filled in registers, 1024 threads a workgroup: no
scratch, nothing spilled, at most 128 VGPRs (1024 threads are four waves a SIMD of 512 registers) and at most 64 KiB of static LDS —
the image of the object reuses the flood's exchange buffer. Read out of the kernel metadata of the gfx950 assembly, built with the
Makefile's compiler and flags. It needs hipcc, no GPU."""
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
    """{symbol: {field: value}} of every kernel of ca_isolate.hip."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or _make_var(mk, "HIPCC")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is not installed")
    assert re.search(r"^OBJS\s*:=.*\bca_isolate\.o\b", mk, re.M)
    arch = _make_var(mk, "ARCH")
    out = tmp_path_factory.mktemp("codegen") / "ca_isolate.s"
    cmd = [hipcc, f"--offload-arch={arch}"] + _make_var(mk, "CXXFLAGS").split() + ["--cuda-device-only", "-S", "ca_isolate.hip", "-o", str(out)]
    subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    listing = out.read_text()
    meta = listing[listing.index("amdhsa.kernels"):]
    found = {}
    for e in ("." + e for e in meta.split("  - .")):
        m = re.search(r"\.name:\s+(\w+)", e)
        if m and re.search(r"\.vgpr_count:", e):
            found[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, e).group(1)) for f in FIELDS}
    return found


def test_isolate_kernel_resources(kernels):
    hits = [n for n in kernels if re.search(r"\d+ca_ensemble_isolate64E", n)]
    assert len(hits) == 1 and len(kernels) == 1, sorted(kernels)
    k = kernels[hits[0]]
    print("ca_ensemble_isolate64", k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128
    assert k["group_segment_fixed_size"] <= 65536
