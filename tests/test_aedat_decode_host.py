"""CPU: the decoders of the AEDAT ingest (eventcalib_amd/csrc/aedat_events.hpp — the field extraction, the wrap flag, the filter,
the header parser and the packet indexer that the kernels of ecal_aedat.hip and EventStream::aedat2bin call) compiled for the host —
tests/cpp/check_aedat_decode.cpp: per format 2 000 seeded random payloads decoded by a plain decoder of the test's own, by the
header's sequential decoder, and block-wise with blocks of 1, 2, 7, 64 events and of the kernels' block; records and every counter
identical across all of them; then the header and indexer cases — once plainly and once under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded).  And the C ABI's new names: declared in
include/ecal.h, listed in capi.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_aedat_decode.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
# no FMA contraction, as the device translation unit: t is one conversion and one multiplication
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]
NEW_INT_SYMBOLS = ("ecal_aedat_parse_header", "ecal_aedat_index_packets", "ecal_aedat_count_events_dev", "ecal_events_from_aedat_dev",
                   "ecal_stream_create_from_aedat_file", "ecal_aedat_to_bin_file")


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_blockwise_decode_equals_sequential_decode(tmp_path, name, extra):
    exe = str(tmp_path / ("check_aedat_decode_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "AEDAT 3.1: 2000 payloads equal" in out.stdout and "AEDAT 2.0: 2000 payloads equal" in out.stdout
    assert "headers: 18 cases, 0 wrong" in out.stdout and "indexer: 16 cases, 0 wrong" in out.stdout


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_INT_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    assert re.search(r"^void ecal_aedat_default_options\(", header, re.M) and '"ecal_aedat_default_options"' in listed
    assert re.search(r"^uint32_t ecal_aedat_block_events\(", header, re.M) and '"ecal_aedat_block_events"' in listed
    for struct in ("ecal_aedat_options", "ecal_aedat_info", "ecal_aedat_packet"):
        assert "typedef struct %s" % struct in header, struct
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays


def test_the_ctypes_structures_follow_the_header():
    """field names and order of the ctypes mirrors against the C declarations (sizes are checked on the GPU against the library)"""
    from eventcalib_amd import capi
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    for cname, cls in (("ecal_aedat_options", capi.AedatOptions), ("ecal_aedat_info", capi.AedatInfo), ("ecal_aedat_packet", capi.AedatPacket)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names.append(first.split()[-1])
                names.extend(r.strip() for r in rest)
        assert names == [n for n, _ in cls._fields_], cname
