"""CPU: the decoders of the raw ingest (eventcalib_amd/csrc/raw_events.hpp — the word step, the summary monoid and the filter that
the kernels of ecal_raw.hip and EventStream::raw2bin call) compiled for the host — tests/cpp/check_raw_decode.cpp: per format 2 000
seeded random word streams decoded by a plain decoder of the test's own, sequentially through the step, and block-wise through
summary / combine / per-block decode with blocks of 1, 2, 7, 64 words and of the kernels' block; records, drop counts and wrap
counts identical across all of them — once plainly and once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone
program with its own main: nothing is preloaded).  And the C ABI's new names: declared in include/ecal.h, listed in capi.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_raw_decode.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
# no FMA contraction, as the device translation unit: t is one conversion and one multiplication
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]
NEW_INT_SYMBOLS = ("ecal_raw_count_events_dev", "ecal_events_from_raw_dev", "ecal_stream_create_from_raw_file", "ecal_raw_to_bin_file")


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_blockwise_decode_equals_sequential_decode(tmp_path, name, extra):
    exe = str(tmp_path / ("check_raw_decode_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "EVT3: 2000 streams equal" in out.stdout and "EVT2: 2000 streams equal" in out.stdout and "headers: 11 cases" in out.stdout


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_INT_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    assert re.search(r"^void ecal_raw_default_options\(", header, re.M) and '"ecal_raw_default_options"' in listed
    assert re.search(r"^uint32_t ecal_raw_block_words\(", header, re.M) and '"ecal_raw_block_words"' in listed
    assert "typedef struct ecal_raw_options" in header and "typedef struct ecal_raw_info" in header
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays
