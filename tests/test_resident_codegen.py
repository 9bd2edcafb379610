"""Where the resident 512^3 row-pair kernel (ca_resident_kernel.inc, resident_pair_run) asks for its neighbours' faces of the next
state is part of its design: after plane CA3D_RES_PAIR_PRE of the main pass. The source can say so and the compiled kernel still do
something else — the arithmetic in front of the request is pure, and once nothing but the image write read its results it sank behind
the request's branch, which then left at the head of the pass. This test reads the order out of the gfx950 assembly of the
ahead-of-time kernel, built with the Makefile's compiler and flags. It needs hipcc, no GPU."""
import os
import re

import pytest

import codegen_lib as cg


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    return cg.listings(tmp_path_factory.mktemp("codegen"), ["ca_resident"])["ca_resident"]


def _kernel(listing, fragment):
    """(mnemonics of the kernel whose symbol contains `fragment`, its metadata entry)."""
    lines = listing.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % fragment, l))
    symbol = lines[start].split(":")[0]
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    ops = [l.split()[0] for l in (x.strip() for x in lines[start + 1:end]) if l and re.match(r"^[a-z]\w+(\s|$)", l)]
    meta = listing[listing.index(".name:", listing.index("amdhsa.kernels")):]
    entry = next(e for e in meta.split("  - .") if re.search(r"\.name:\s+%s\s" % re.escape(symbol), e))
    return ops, entry


def _pair_pre():
    src = open(os.path.join(cg.CSRC, "ca_resident_kernel.inc")).read()
    return int(re.search(r"^#define CA3D_RES_PAIR_PRE (\d+)", src, re.M).group(1))


def _lookahead_requests(ops):
    """For every look-ahead request of the step loop — four face loads in a row with the image write behind them and no barrier in
    between (the poll's four loads have the barrier behind them) — the number of v_bitop3_b32 between the z-face stores and the request."""
    found = []
    i = 0
    while i < len(ops):
        if ops[i] != "global_load_dwordx2":
            i += 1
            continue
        j = i
        while j < len(ops) and ops[j] == "global_load_dwordx2":
            j += 1
        if j - i == 4:
            after = next((o for o in ops[j:] if o in ("s_barrier", "ds_write_b128")), None)
            if after == "ds_write_b128":
                n, k = 0, i - 1
                while k >= 0 and ops[k] not in ("global_store_dwordx2", "s_barrier", "ds_write_b128"):
                    n += ops[k] == "v_bitop3_b32"
                    k -= 1
                assert k >= 0 and ops[k] == "global_store_dwordx2", "the z-face stores come before the request"
                found.append(n)
        i = j
    return found


def test_pair_kernel_asks_for_the_next_faces_where_the_source_says(listing):
    ops, _ = _kernel(listing, "ca_resident_vn_pair")
    pre = min(_pair_pre(), 15)  # 15 and up: behind the pass (planes 1 .. 14)
    # 2 rows x 5 v_bitop3_b32 per word-plane, planes 1 .. pre of the main pass in front of the request; one plane of slack
    need = 2 * 5 * (pre - 1)
    found = _lookahead_requests(ops)
    assert len(found) >= 2, f"both halves of the unrolled step loop ask ahead: {found}"
    assert all(n >= need for n in found), f"v_bitop3_b32 between the z-face stores and the request: {found}, expected at least {need}"


def test_pair_kernel_spills_nothing(listing):
    _, entry = _kernel(listing, "ca_resident_vn_pair")
    assert re.search(r"\.vgpr_spill_count:\s+0\s", entry), entry
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)) <= 256
