"""The device texts that the ensemble's object kernels share exist ONCE under csrc/: the pass over the 48 orientations
(ca_canon_pass.inc), the flood loop (ca_flood_loop.inc) and the turn image's constants (ca_turn_image.inc). The first two are fragments:
text included inside the function whose body they are, so they carry no include guard, and only the files named here include them
(DESIGN.md 12.15). The sources are read as text: no GPU, no compiler."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellularautomatons3d_amd", "csrc")

FRAGMENTS = {"ca_canon_pass.inc": ["ca_canon.hip", "ca_canon_period.hip"], "ca_flood_loop.inc": ["ca_census.hip", "ca_flood.inc"]}
HEADERS = {"ca_turn_image.inc": ["ca_canon.hip", "ca_canon_period.hip", "ca_compose.hip"]}


def _sources():
    """{file name: text} of every source file of csrc/."""
    return {n: open(os.path.join(CSRC, n), encoding="utf-8").read() for n in sorted(os.listdir(CSRC))
            if n.endswith((".hip", ".inc", ".h", ".cpp"))}


def _holders(needle):
    """[(file, occurrences)] of the files of csrc/ whose text holds `needle`."""
    return [(n, t.count(needle)) for n, t in _sources().items() if needle in t]


def test_orientation_loop_exists_once():
    assert _holders("for (u32 o = 0; o < kOrientations; o++)") == [("ca_canon_pass.inc", 1)]


def test_flood_loop_exists_once():
    assert _holders("F[p][h] = f;") == [("ca_flood_loop.inc", 1)]


def test_image_constants_exist_once():
    assert _holders("constexpr u32 kImgPlane") == [("ca_turn_image.inc", 1)]


def test_fragments_have_no_include_guard():
    src = _sources()
    for name in FRAGMENTS:
        assert "#pragma once" not in src[name], name
        assert not re.search(r"^\s*#\s*(ifndef|if\s+!defined)", src[name], re.M), name
    for name in HEADERS:
        assert src[name].count("#pragma once") == 1, name


def test_shared_files_are_included_by_their_users_alone():
    src = _sources()
    for name, users in {**FRAGMENTS, **HEADERS}.items():
        found = {n: len(re.findall(r'^\s*#\s*include\s+"%s"' % re.escape(name), t, re.M)) for n, t in src.items()}
        assert {n: c for n, c in found.items() if c} == {u: 1 for u in users}, name


def test_makefile_rebuilds_the_users_of_a_shared_file():
    rule = re.search(r"^%\.o:\s*%\.hip\s+(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    assert rule, "the %.o: %.hip rule of csrc/Makefile"
    prerequisites = rule.group(1).split()
    for name in list(FRAGMENTS) + list(HEADERS):
        assert name in prerequisites, name
