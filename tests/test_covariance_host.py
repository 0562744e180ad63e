"""CPU: the covariance of the intrinsics from the banded-arrow system (eventcalib_amd/csrc/arrow_covariance.hpp) without a GPU —
tests/cpp/check_covariance.cpp builds random positive definite arrow systems (n_cp = 4, 5, 9, 40) in the kernel's accumulation
layout and compares Sigma_ii, P = (H^-1)[intr, :] and cov_robust with a dense long double inverse, to 100 n eps kappa_2 of the scaled
system (the program's header derives the bar of each quantity); a control point without rows must report positive_definite = 0 and
NaN, one cluster robust_valid = 0.  Built plainly and under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with
its own main: nothing is preloaded); any failed check or sanitizer report fails the test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_covariance.cpp")
# the flags the host half is compiled with in the product (the solver's translation unit contracts to FMA)
FLAGS = ["-std=c++17", "-ffp-contract=fast", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "eventcalib_amd", "csrc"),
         "-I" + os.path.join(ROOT, "include")]


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("address_undefined", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_covariance_against_a_dense_inverse(tmp_path, name, extra):
    exe = str(tmp_path / ("check_covariance_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC, "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_covariance: ok" in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
