"""CPU: the radial camera / quaternion spline path of eventcalib_amd/csrc/spline_residual.hpp (spline_residual with its 33-column
row, spline_residual_px, spline_pose_quat + spline_board_point) compiled for the host — tests/cpp/residual_frozen.cpp: 64 cases bit
for bit against tests/golden/residual_frozen_radial_quat.bin, the values of the header as it stood before these functions shared
their arithmetic.  test_board_point_host.py and test_residual_px_host.py hold the functions to each other; this one holds them to
what they computed.  Once plainly and once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with its
own main: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "residual_frozen.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "residual_frozen_radial_quat.bin")
# no FMA contraction: + - * / sqrt, each rounded once, give the same bits with any optimisation level
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall"]


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_residual_header_matches_the_frozen_values(tmp_path, name, extra):
    exe = str(tmp_path / ("residual_frozen_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "64 cases bit-equal" in out.stdout
