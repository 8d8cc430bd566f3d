"""The interval guard of csrc/neighbour_pick.h on the host (no GPU): the header compiles as plain C++, and whenever the guard passes
for offsets within E of the exact pick's, its integers are neighbour_pick_exact's.

tests/neighbour_pick_guard_check.cpp is the program: 400 000 seeded (rv0, rv1, x, yi) per radius 1, 30 and 86 (1.2 million picks, x up
to 3839 and yi up to 2159), each moved by 0, +-E, +-E (1 - 2^-20) and by the offsets that land the sum on the nearest integer and one
unit in the last place to either side; rv0 = 0 and non-finite input must fail the guard. It runs twice: as built by g++ -O2, and as
a stand-alone binary built with -fsanitize=address,undefined."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "neighbour_pick_guard_check.cpp")
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")
CASES = 400000  # per radius: 1.2 million picks


def _build_and_run(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, *flags, "-o", exe, SRC], check=True)
    p = subprocess.run([exe, str(CASES)], capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    m = re.search(r"^ok (.*)$", p.stdout, re.M)
    assert m, p.stdout[-500:]
    f = m.group(1).split()
    return dict(zip(f[0::2], (int(v) for v in f[1::2])))


def test_guard_passes_only_with_the_exact_integers(tmp_path):
    got = _build_and_run(tmp_path, "guard_check", ["-O2"])
    assert got["cases_per_radius"] == CASES and got["unmoved"] == 3 * CASES >= 10 ** 6
    # the offsets bite: a guard told E / 8 is caught; and the real one is no refusal of everything: with the exact offsets
    # themselves it clears more than 98 % of the picks at every radius (the cap of the GPU test, here for the guard alone)
    assert got["control_caught"] > 0
    for r in ("r1", "r30", "r86"):
        assert got["unmoved_passed_" + r] >= 0.98 * CASES, got


def test_guard_check_under_address_and_undefined_sanitizers(tmp_path):
    """the same program as a stand-alone host binary under -fsanitize=address,undefined (any report is fatal; the runtimes are linked into the
    binary, so it needs nothing of its environment)"""
    got = _build_and_run(tmp_path, "guard_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    assert got["unmoved"] == 3 * CASES
