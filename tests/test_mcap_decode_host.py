"""CPU: the mcap ingest without a device.

eventcalib_amd/csrc/mcap_events.hpp — the ros2msg parser, the STRUCT layouts derived from a schema (dvs_msgs/Event must give
lead 14, stride 16 and the two offset sets of the contract), the CDR walk, the chain of records, the host decoder and every refusal —
compiled for the host: tests/cpp/check_mcap_events.cpp, once plainly and once under AddressSanitizer + UndefinedBehaviorSanitizer (a
stand-alone program with its own main: nothing is preloaded).

The writer of tests/mcap_writer.py against itself: its event-by-event CDR serialiser and its numpy one give the same bytes, and its
reader finds the events the writer put in."""
import os
import subprocess

import numpy as np
import pytest

import mcap_writer as mw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_mcap_events.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]   # (no FMA contraction, as the device translation unit)


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_header_on_the_host(tmp_path, name, extra):
    exe = str(tmp_path / ("check_mcap_events_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "layouts: 4 cases" in out.stdout
    assert "parser: 3 cases" in out.stdout
    assert "decode: 11 cases" in out.stdout
    assert "refusals: 40 cases" in out.stdout
    assert "wrong: 0" in out.stdout


def test_the_writer_serialises_events_the_same_both_ways_and_the_reader_finds_them():
    rng = np.random.default_rng(3)
    for text in (mw.DVS_EVENT_ARRAY, mw.DVS_EVENT_ARRAY.replace("uint16 x\nuint16 y", "uint8 x\nuint8 y"),
                 mw.DVS_EVENT_ARRAY.replace("uint16 x\nuint16 y\nbuiltin_interfaces/Time ts\nbool polarity", "bool p\nbuiltin_interfaces/Time t\nuint32 y\nuint16 x")):
        for n in (0, 1, 2, 3, 70):
            ev = mw.events_array(rng.integers(0, 200, n), rng.integers(0, 200, n), rng.integers(-5, 2 ** 31 - 1, n), rng.integers(0, 2 ** 32, n), rng.integers(0, 256, n))
            one = mw.event_array_message(ev, frame_id=b"ab", text=text, vectorized=False)
            assert one == mw.event_array_message(ev, frame_id=b"ab", text=text, vectorized=True)
            data = mw.write_mcap([(1, "E", "ros2msg", text)], [(1, 1, "/e")], [(1, one)], per_chunk=n % 2)
            table, info = mw.index_messages(data)
            t_ns, x, y, p = mw.table_events(data, table, info["layout"])
            assert info["n_raw_events"] == n and np.array_equal(x, ev["x"]) and np.array_equal(y, ev["y"]) and np.array_equal(p, ev["pol"] != 0)
            assert np.array_equal(t_ns, ev["sec"].astype(np.int64) * 10 ** 9 + ev["nsec"])
    assert mw.struct_layout(mw.event_struct(mw.DVS_EVENT_ARRAY)) == dict(kind=1, lead=14, stride=16, span=[13, 15], x=[0, 0], y=[2, 2], sec=[4, 6], nsec=[8, 10],
                                                                         pol=[12, 14], x_bytes=2, y_bytes=2)
