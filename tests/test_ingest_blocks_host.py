"""CPU: the host/device pieces the ingest kernels share (eventcalib_amd/csrc/ingest_blocks.hpp — the clipped load, the table
bisection, the table check — and event_record.hpp's packed record) compiled for the host — tests/cpp/check_ingest_blocks.cpp: the load at every
distance from the end of a heap buffer of exactly n_bytes against a bytewise reference, the bisection against a linear search on
tables with empty entries in front, in the middle and at the end, the table check on entries around the file's end and around 2^64
against 128-bit arithmetic, the record against '<dddB' — once plainly
and once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded), which is
what holds "nothing behind n_bytes is read"."""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_ingest_blocks.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
])
def test_shared_ingest_pieces_on_the_host(tmp_path, name, extra):
    exe = str(tmp_path / ("check_ingest_blocks_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    loads = re.search(r"loads: (\d+) cases, 0 wrong", out.stdout)
    tables = re.search(r"tables: (\d+) cases, 0 wrong", out.stdout)
    assert loads and int(loads.group(1)) >= 48 * 3
    assert tables and int(tables.group(1)) >= 128 * 200
    outside = re.search(r"outside: (\d+) cases, 0 wrong", out.stdout)
    assert outside and int(outside.group(1)) >= 6 * 4
    assert "pack_record: 0 wrong" in out.stdout
    record = bytes(int(b, 16) for b in re.search(r"record:((?: [0-9a-f]{2}){25})", out.stdout).group(1).split())
    assert record == struct.pack("<dddB", 0.123456789012345678, 345.0, 259.0, 0)
