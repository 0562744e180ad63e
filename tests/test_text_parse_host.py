"""CPU: the line parser of the text ingest (eventcalib_amd/csrc/text_events.hpp — the functions the parse kernel and the host
fallback call) compiled for the host — tests/cpp/check_text_parse.cpp: 200 000 seeded random lines of the fast class equal to
strtoll / strtod bit for bit, 20 000 lines built to leave the fast class handed to the host and never given a value, the malformed
and the blank lines — once plainly and once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with its own
main: nothing is preloaded).  And the C ABI's new names: declared in include/ecal.h, listed in capi.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_text_parse.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
# no FMA contraction, as the device translation unit: a decimal is ONE rounded operation
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]
NEW_SYMBOLS = ("ecal_events_from_text_dev", "ecal_text_count_lines_dev", "ecal_stream_create_from_text_file", "ecal_text_to_bin_file")


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_line_parser_matches_strtoll_and_strtod(tmp_path, name, extra):
    exe = str(tmp_path / ("check_text_parse_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "200000 lines equal, 20000 lines for the host" in out.stdout


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    assert re.search(r"^void ecal_text_default_options\(", header, re.M) and '"ecal_text_default_options"' in listed
    assert "typedef struct ecal_text_options" in header and "typedef struct ecal_text_info" in header
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays
