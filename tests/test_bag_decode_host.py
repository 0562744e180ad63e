"""CPU: the decoders of the bag ingest (eventcalib_amd/csrc/bag_events.hpp — the field-list parser, the record walker with its choice
of topic and type, the 13-byte field extraction, the filter, that the kernels of ecal_bag.hip and EventStream::bag2bin call) compiled
for the host — tests/cpp/check_bag_decode.cpp: 2 000 seeded random bags decoded from the generator's own book-keeping, by the header's
sequential decoder, and block-wise with blocks of 1, 2, 7, 64 events and of the kernels' block; records and every counter identical
across all of them; then the indexer's and the field parser's cases — once plainly and once under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded).  The library's host indexer against the
Python oracle of tests/bag_writer.py on bags of that writer.  And the C ABI's new names: declared in include/ecal.h, listed in capi.py."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bag_writer as bw  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "check_bag_decode.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
# no FMA contraction, as the device translation unit: t is one conversion and one multiplication
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]
NEW_INT_SYMBOLS = ("ecal_bag_index_messages", "ecal_bag_count_events_dev", "ecal_events_from_bag_dev", "ecal_stream_create_from_bag_file",
                   "ecal_bag_to_bin_file")


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_blockwise_decode_equals_sequential_decode(tmp_path, name, extra):
    exe = str(tmp_path / ("check_bag_decode_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bags: 2000 bags equal" in out.stdout
    assert "indexer: 56 cases, 0 wrong" in out.stdout


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_INT_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    assert re.search(r"^void ecal_bag_default_options\(", header, re.M) and '"ecal_bag_default_options"' in listed
    assert re.search(r"^uint32_t ecal_bag_block_events\(", header, re.M) and '"ecal_bag_block_events"' in listed
    for struct_name in ("ecal_bag_options", "ecal_bag_info", "ecal_bag_message"):
        assert "typedef struct %s" % struct_name in header, struct_name
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays
    assert "ROS bags are not read" not in header
    assert "16_bag_ingest" in open(os.path.join(ROOT, "design", "15_aedat_ingest.md")).read()


def test_the_ctypes_structures_follow_the_header():
    """field names and order of the ctypes mirrors against the C declarations (sizes are checked on the GPU against the library)"""
    from eventcalib_amd import capi
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    for cname, cls in (("ecal_bag_options", capi.BagOptions), ("ecal_bag_info", capi.BagInfo), ("ecal_bag_message", capi.BagMessage)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names.append(first.split()[-1].lstrip("*"))
                names.extend(r.strip() for r in rest)
        assert names == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(capi.BagMessage) == 16 == capi.BAG_MESSAGE_DTYPE.itemsize == bw.MESSAGE_DTYPE.itemsize
    assert ctypes.sizeof(capi.BagInfo) == 14 * 8


# ---- the library's host indexer (no device, no context) against the oracle ----------------------------------------------------------------
def _library():
    import eventcalib_amd
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(eventcalib_amd.lib_path())


def _index(L, data, topic=None, type_=None):
    from eventcalib_amd import capi
    L.ecal_bag_default_options.argtypes, L.ecal_bag_default_options.restype = [ctypes.POINTER(capi.BagOptions)], None
    L.ecal_bag_index_messages.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(capi.BagOptions), ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(capi.BagInfo)]
    L.ecal_bag_index_messages.restype = ctypes.c_int
    o = capi.BagOptions()
    L.ecal_bag_default_options(ctypes.byref(o))
    assert o.auto_time_base == 1 and o.time_base == 0 and not o.topic and not o.type and o.start_time == -float("inf") and o.has_end_time == 0
    o.topic, o.type = (topic.encode() if topic else None), (type_.encode() if type_ else None)
    n, info = ctypes.c_uint64(), capi.BagInfo()
    st = L.ecal_bag_index_messages(None, data, len(data), ctypes.byref(o), None, 0, ctypes.byref(n), ctypes.byref(info))
    if st not in (0, -6):
        return st, None, None
    table = np.zeros(int(n.value), capi.BAG_MESSAGE_DTYPE)
    st = L.ecal_bag_index_messages(None, data, len(data), ctypes.byref(o), table.ctypes.data if table.size else None, table.size, ctypes.byref(n),
                                   ctypes.byref(info))
    return st, table, info.as_dict()


def _random_bag(seed):
    rng = np.random.default_rng(seed)
    conns = [(0, "/dvs/events", bw.DVS), (3, "/dvs/image_raw", "sensor_msgs/Image"), (7, "/dvs/imu", "sensor_msgs/Imu")]
    msgs = []
    for k in range(int(rng.integers(1, 30))):
        if rng.integers(0, 3) == 0:
            msgs.append((int(rng.choice([3, 7])), bytes(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8))))
        else:
            n = int(rng.integers(0, 50))
            ev = bw.events_array(rng.integers(0, 346, n), rng.integers(0, 260, n), 1600000000 + rng.integers(0, 3, n), rng.integers(0, 10 ** 9, n),
                                 rng.integers(0, 2, n))
            msgs.append((0, bw.event_array_message(ev, seq=k, frame_id=b"davis"[: int(rng.integers(0, 6))])))
    return bw.write_bag(conns, msgs, per_chunk=[int(v) for v in rng.integers(0, 5, 3)], closed=bool(seed & 1))


def test_the_host_indexer_equals_the_oracle_on_written_bags():
    L = _library()
    for seed in range(60):
        data = _random_bag(seed)
        for cut in (len(data), 4109 + (seed * 7919) % (len(data) - 4109)):
            part = data[:cut]
            try:
                want_table, want = bw.index_messages(part)
            except bw.BagError:
                assert _index(L, part)[0] == -1, (seed, cut)
                continue
            st, table, info = _index(L, part)
            assert st == 0, (seed, cut)
            assert table.tobytes() == want_table.tobytes(), (seed, cut)
            assert {k: info[k] for k in want} == want, (seed, cut)


def test_the_host_indexer_refuses_what_the_contract_refuses():
    L = _library()
    conns = [(0, "/dvs/events", bw.DVS)]
    ev = bw.events_array([1, 2], [3, 4], [1600000000] * 2, [5, 6], [0, 1])
    msgs = [(0, bw.event_array_message(ev))]
    assert _index(L, bw.write_bag(conns, msgs))[0] == 0
    for bad in (bw.write_bag(conns, msgs, magic=b"#ROSBAG V1.2\n"), b"SQLite format 3\0" + bytes(100), b"\x89MCAP0\r\n" + bytes(100), b"", bytes(50),
                bw.write_bag(conns, msgs, compression="bz2"), bw.write_bag(conns, msgs, compression="lz4"),
                bw.write_bag([(0, "/a", bw.DVS), (1, "/b", bw.PROPHESEE)], [(0, msgs[0][1]), (1, msgs[0][1])]),
                bw.write_bag([(0, "/image", "sensor_msgs/Image")], [(0, b"abc")]),
                bw.write_bag(conns, [(0, msgs[0][1] + b"\0")])):
        with pytest.raises(bw.BagError):
            bw.index_messages(bad)
        assert _index(L, bad)[0] == -1
    stereo = bw.write_bag([(0, "/a", bw.DVS), (1, "/b", bw.PROPHESEE)], [(0, msgs[0][1]), (1, msgs[0][1]), (1, msgs[0][1])])
    assert _index(L, stereo, topic="/b")[2]["n_messages"] == 2 == bw.index_messages(stereo, topic="/b")[1]["n_messages"]
    assert _index(L, stereo, topic="/a")[2]["n_other_messages"] == 2
    assert _index(L, stereo, type_=bw.PROPHESEE)[2]["n_messages"] == 2
    assert struct.unpack_from("<I", stereo, 13)[0] + 8 + struct.unpack_from("<I", stereo, 13 + 4 + struct.unpack_from("<I", stereo, 13)[0])[0] == 4096
