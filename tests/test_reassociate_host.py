"""CPU: the deciding half of the re-association (eventcalib_amd/csrc/board_nearest.hpp: nearest landmark with ties to the lower
index, d = sqrt(best) - radius, the gate |d| < ring_tol — the functions both board-frame kernels call) compiled for the host —
tests/cpp/check_board_nearest.cpp: 10 000 random cases, exact ties, repeated landmarks, no landmark, NaN points and points exactly
on the gate among them, equal to a straightforward loop bit for bit — once plainly and once under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded).  And the C ABI's new names: declared
in include/ecal.h, listed in capi.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_board_nearest.cpp")
# no FMA contraction: these functions decide (the device translation units compile them the same way)
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall"]
NEW_SYMBOLS = ("ecal_solver_reassociate_dev", "ecal_solver_reassociate", "ecal_solver_create_reassociated")


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_nearest_landmark_and_gate_match_a_plain_loop(tmp_path, name, extra):
    exe = str(tmp_path / ("check_board_nearest_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "10000 cases equal" in out.stdout


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    assert "typedef struct ecal_reassociate_totals" in header
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays
