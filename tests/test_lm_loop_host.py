"""CPU: the solver's Levenberg-Marquardt loop (eventcalib_amd/csrc/lm_loop.hpp) without a GPU — tests/cpp/check_lm_loop.cpp supplies
a host implementation of the loop's seam to the device and runs it single-rank (sequential and on a worker pool), as time shards of
one spline (W = 2, 3: ranks are threads, the collectives a barrier-and-add that gives up after a bounded wait), as distributed
segments (W = 2) and against a dense restatement of tests/ref_lm.py, for the quaternion and the SO3 spline.  Built plainly, under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer (a stand-alone program with its own main: nothing is
preloaded); any failed check or sanitizer report fails the test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_lm_loop.cpp")
# the flags the loop is compiled with in the product (the solver's translation unit contracts to FMA)
FLAGS = ["-std=c++17", "-ffp-contract=fast", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "eventcalib_amd", "csrc"),
         "-I" + os.path.join(ROOT, "include")]


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("address_undefined", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
    ("thread", ["-O1", "-g", "-fsanitize=thread", "-fno-omit-frame-pointer"]),
])
def test_lm_loop_variants_give_the_same_iterates(tmp_path, name, extra):
    exe = str(tmp_path / ("check_lm_loop_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC, "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_lm_loop: ok" in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
