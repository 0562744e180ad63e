"""CPU: the pixel-gradient functions of eventcalib_amd/csrc/spline_residual.hpp (spline_residual_px, spline_residual_px_so3,
residual_px_distance: the residual with its gradient by the event's own pixel, behind the report in pixels) compiled for the
host — tests/cpp/check_residual_px.cpp: 10 000 random cases over radial / fisheye and quaternion / SO3, r bit-equal to
spline_residual*, (gu, gv) bit-equal to (-J[2], -J[3]) of the same call with a Jacobian row, the degenerate verdicts exactly the
non-finite and non-positive cases (a board point exactly on its landmark among them) — once plainly and once under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded).  Both sides are
built on the same helpers of the header (ray, distance, way back, d c / d r2, pose), so the check is of what each side adds to
them; the device code was compared with the code from before they shared (design/08_solver.md, "One copy of the residual's
pieces": moving gx, gy into a helper changes a rounding in the solver), and that the values are the earlier ones is
test_residual_frozen_host.py's part."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_residual_px.cpp")
# no FMA contraction in either half of the comparison: one set of flags for the whole translation unit
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall"]


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_residual_px_header_matches_the_residual(tmp_path, name, extra):
    exe = str(tmp_path / ("check_residual_px_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "10000 cases bit-equal" in out.stdout
