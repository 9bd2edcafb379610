"""What the *_codegen tests share: the variables of csrc/Makefile, the gfx950 assembly of a .hip file of csrc built with the Makefile's
compiler and flags, and the kernel metadata at its end. It needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellularautomatons3d_amd", "csrc")
FIELDS = ["group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count"]


def makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def make_var(name, text=None):
    """The value csrc/Makefile gives `name` with ?=."""
    m = re.search(r"^%s\s*\?=\s*(.*)$" % name, makefile() if text is None else text, re.M)
    assert m, f"{name} not found in csrc/Makefile"
    return m.group(1).strip()


def listings(tmp, stems, extra_flags=()):
    """{stem: assembly of csrc/<stem>.hip for the Makefile's ARCH}, compiled side by side into the directory `tmp`. Skips the test
    without hipcc."""
    mk = makefile()
    hipcc = os.environ.get("HIPCC") or make_var("HIPCC", mk)
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is not installed")
    head = [hipcc, "--offload-arch=" + make_var("ARCH", mk)] + make_var("CXXFLAGS", mk).split() + list(extra_flags) + ["--cuda-device-only", "-S"]
    procs = [subprocess.Popen(head + [stem + ".hip", "-o", str(tmp / (stem + ".s"))], cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
             for stem in stems]
    assert [p.wait() for p in procs] == [0] * len(stems), stems
    return {stem: (tmp / (stem + ".s")).read_text() for stem in stems}


def kernel_metadata(listing):
    """{symbol: {field: value}} of every kernel in the amdhsa.kernels metadata of a listing, FIELDS as integers."""
    meta = listing[listing.index("amdhsa.kernels"):]
    found = {}
    for e in ("." + e for e in meta.split("  - .")):
        m = re.search(r"\.name:\s+(\w+)", e)
        if m and re.search(r"\.vgpr_count:", e):
            found[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, e).group(1)) for f in FIELDS}
    return found


def one_kernel(kernels, pattern):
    """The fields of the one kernel whose symbol matches `pattern`."""
    hits = [n for n in kernels if re.search(pattern, n)]
    assert len(hits) == 1, (pattern, sorted(kernels))
    return kernels[hits[0]]
