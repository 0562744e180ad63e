"""CPU: the board-point functions of eventcalib_amd/csrc/spline_residual.hpp (spline_board_point, spline_pose_quat,
spline_pose_so3: the first half of the residual behind the board-frame event image; the residual functions are built on the same
residual_ray and pose code) compiled for the host — tests/cpp/check_board_point.cpp: 10 000 random cases over pinhole / fisheye
and quaternion / SO3, the residual's tail reconstructed from the board point bit-equal to spline_residual*, the `false` verdicts
exactly the non-finite and non-positive depths (against a depth computed by another route) — once plainly and once under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded).  The device code
of every kernel that uses these functions was compared with the code from before they shared (design/08_solver.md, "One copy of
the residual's pieces"); that the values are the earlier ones is test_residual_frozen_host.py's part."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_board_point.cpp")
# no FMA contraction in either half of the comparison: one set of flags for the whole translation unit
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall"]


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_board_point_header_matches_the_residual(tmp_path, name, extra):
    exe = str(tmp_path / ("check_board_point_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "10000 cases bit-equal" in out.stdout
