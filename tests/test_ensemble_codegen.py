"""The three *_moving ensemble kernels (ca_ensemble.hip) are launched with 1024 threads and four waves a SIMD: 128 vector registers at
most, none spilled, no scratch — what a check point adds must not stay in registers across the steps. Read out of the metadata of the
gfx950 assembly, built with the Makefile's compiler and flags. It needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellularautomatons3d_amd", "csrc")
KERNELS = ["ca_ensemble_vn64_moving", "ca_ensemble_moore64_moving", "ca_ensemble_clustered64_moving"]


def _make_var(text, name):
    m = re.search(r"^%s\s*\?=\s*(.*)$" % name, text, re.M)
    assert m, f"{name} not found in csrc/Makefile"
    return m.group(1).strip()


@pytest.fixture(scope="module")
def entries(tmp_path_factory):
    """The metadata entry of every kernel of ca_ensemble.hip, by the name in its symbol."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or _make_var(mk, "HIPCC")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is not installed")
    arch = _make_var(mk, "ARCH")
    flags = _make_var(mk, "CXXFLAGS").split()
    out = tmp_path_factory.mktemp("codegen") / "ca_ensemble.s"
    cmd = [hipcc, f"--offload-arch={arch}"] + flags + ["--cuda-device-only", "-S", "ca_ensemble.hip", "-o", str(out)]
    subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    listing = out.read_text()
    meta = listing[listing.index(".name:", listing.index("amdhsa.kernels")):]
    found = {}
    for e in meta.split("  - ."):
        m = re.search(r"\.name:\s+_ZN\w*?\d+(ca_ensemble_\w+?)ENS", e)
        if m:
            found[m.group(1)] = e
    return found


@pytest.mark.parametrize("kernel", KERNELS)
def test_moving_kernels_fit_four_waves_a_simd(entries, kernel):
    assert kernel in entries, sorted(entries)
    e = entries[kernel]
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", e).group(1))
    print(kernel, "vgpr_count", vgprs, "sgpr_count", re.search(r"\.sgpr_count:\s+(\d+)", e).group(1))
    assert vgprs <= 128
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
