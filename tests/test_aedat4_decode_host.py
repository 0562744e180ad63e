"""CPU: the decoders of the AEDAT 4 ingest (eventcalib_amd/csrc/aedat4_events.hpp — the header parser, the packet indexer, the LZ4
frame walker and inflater, the FlatBuffer locator, the 16-byte event, the filter that the kernels of ecal_aedat4.hip and
EventStream::aedat42bin call) compiled for the host — tests/cpp/check_aedat4_decode.cpp: 2 000 seeded random files decoded by the
test's own book-keeping, by the header's sequential decoder, and block-wise with blocks of 1, 2, 7, 64 events and of the kernels'
block; records and every counter identical; then the header, indexer, frame and locator case tables, and frames made by liblz4
(loaded at run time where it exists) through the header's inflater — once plainly and once under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded).  The writer of the other tests
(tests/aedat4_writer.py) against liblz4 and against the Python oracle.  And the C ABI's new names: declared in include/ecal.h, listed
in capi.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aedat4_oracle as AO  # noqa: E402
import aedat4_writer as AW  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "check_aedat4_decode.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
# no FMA contraction, as the device translation unit: t is one conversion and one multiplication
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]
NEW_INT_SYMBOLS = ("ecal_aedat4_parse_header", "ecal_aedat4_index_packets", "ecal_aedat4_count_events_dev", "ecal_events_from_aedat4_dev",
                   "ecal_stream_create_from_aedat4_file", "ecal_aedat4_to_bin_file")


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_blockwise_decode_equals_sequential_decode(tmp_path, name, extra):
    exe = str(tmp_path / ("check_aedat4_decode_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC, "-ldl"])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "AEDAT 4: 2000 files equal" in out.stdout
    m = re.search(r"(\d+) frames of several blocks, (\d+) files cut short, (\d+) refused", out.stdout)
    assert int(m.group(1)) > 0 and int(m.group(2)) == 500 and int(m.group(3)) > 0
    assert "headers: 18 cases, 0 wrong" in out.stdout and "indexer: 13 cases, 0 wrong" in out.stdout
    assert "frames: 38 cases, 0 wrong" in out.stdout and "locator: 44 cases, 0 wrong" in out.stdout
    assert "liblz4: 200 frames, 0 wrong" in out.stdout or "liblz4: skipped" in out.stdout


def _random_events(rng, n):
    t = 1_700_000_000_000_000 + np.cumsum(rng.integers(0, 40, n))
    return AW.make_events(t, rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n))


def _liblz4():
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.LZ4F_createDecompressionContext.argtypes, lib.LZ4F_createDecompressionContext.restype = [ctypes.POINTER(vp), ctypes.c_uint], sz
    lib.LZ4F_freeDecompressionContext.argtypes, lib.LZ4F_freeDecompressionContext.restype = [vp], sz
    lib.LZ4F_decompress.argtypes = [vp, vp, ctypes.POINTER(sz), vp, ctypes.POINTER(sz), vp]
    lib.LZ4F_decompress.restype = sz
    lib.LZ4F_isError.argtypes, lib.LZ4F_isError.restype = [sz], ctypes.c_uint
    return lib


def _lz4f_decompress(lib, frame, room):
    """(what LZ4F_decompress returns at the end: 0 = the frame is complete and its checksums hold, the bytes)"""
    ctx = ctypes.c_void_p()
    assert not lib.LZ4F_isError(lib.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    src = ctypes.create_string_buffer(bytes(frame), len(frame))
    dst = ctypes.create_string_buffer(room + 16)
    done_in, done_out, rc = 0, 0, 1
    while done_in < len(frame):
        n_out, n_in = ctypes.c_size_t(room + 16 - done_out), ctypes.c_size_t(len(frame) - done_in)
        rc = lib.LZ4F_decompress(ctx, ctypes.byref(dst, done_out), ctypes.byref(n_out), ctypes.byref(src, done_in), ctypes.byref(n_in), None)
        assert not lib.LZ4F_isError(rc), "LZ4F_decompress refuses the writer's frame"
        done_in += n_in.value
        done_out += n_out.value
        if n_in.value == 0 and n_out.value == 0:
            break
    lib.LZ4F_freeDecompressionContext(ctx)
    return rc, dst.raw[:done_out]


def _writer_frames(rng):
    """frames of every kind the writer makes, with what they inflate to"""
    data = AW.event_packet(_random_events(rng, 300))
    big = AW.event_packet(_random_events(rng, 9000))
    yield AW.lz4_stored_frame(data), data
    yield AW.lz4_compressed_frame(data), data
    yield AW.lz4_compressed_frame(big), big                       # three linked blocks
    yield AW.lz4_compressed_frame(big, independent=True), big
    yield AW.lz4_compressed_frame(big, block_max=7), big
    for flags in range(16):
        kw = dict(independent=bool(flags & 1), block_checksum=bool(flags & 2), content_size=bool(flags & 4), content_checksum=bool(flags & 8))
        yield AW.lz4_compressed_frame(data, **kw), data
    f = AW.Lz4Frame()
    lit = bytes(rng.integers(0, 256, 700, dtype=np.uint8))
    f.block([(lit[:271], 1, 19), (b"", 270, 274), (lit[271:285], 13, 4), (lit[285:300], None, 0)])
    f.stored(lit[300:400])
    f.block([(b"", 65, 18), (lit[400:], 3, 20), (b"12345", None, 0)])
    yield f.finish(), bytes(f.out)


def test_the_writers_frames_inflate_through_liblz4():
    """the writer's header checksum, flags, block and content checksums: LZ4F_decompress takes its frames and gives the input back"""
    lib = _liblz4()
    if lib is None:
        print("liblz4.so.1 cannot be loaded: nothing to hold the writer against")
        return
    rng = np.random.default_rng(3)
    n = 0
    for frame, data in _writer_frames(rng):
        rc, out = _lz4f_decompress(lib, frame, len(data))
        assert rc == 0 and out == data
        n += 1
    assert n == 22


def test_the_oracle_inflates_the_writers_frames_and_reads_its_packets():
    rng = np.random.default_rng(4)
    for frame, data in _writer_frames(rng):
        assert AO.lz4_frame(frame) == data
    ev = _random_events(rng, 50)
    for knobs in (dict(), dict(vtable_after=True), dict(extra_fields=2), dict(vector_mod=7), dict(vtable_after=True, vector_mod=0)):
        got = AO.packet_events(AW.event_packet(ev, **knobs))
        assert got.tobytes() == ev.tobytes()
    assert len(AO.packet_events(AW.event_packet(ev[:0], absent=True))) == 0
    assert len(AO.packet_events(AW.event_packet(ev[:0], short_vtable=True))) == 0
    assert AW.xxh32(b"") == 0x02CC5D05 and AW.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_INT_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    assert re.search(r"^void ecal_aedat4_default_options\(", header, re.M) and '"ecal_aedat4_default_options"' in listed
    assert re.search(r"^uint32_t ecal_aedat4_block_events\(", header, re.M) and '"ecal_aedat4_block_events"' in listed
    for struct in ("ecal_aedat4_options", "ecal_aedat4_info", "ecal_aedat4_packet"):
        assert "typedef struct %s" % struct in header, struct
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays


def test_the_ctypes_structures_follow_the_header():
    """field names and order of the ctypes mirrors against the C declarations (sizes are checked on the GPU against the library)"""
    from eventcalib_amd import capi
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    for cname, cls in (("ecal_aedat4_options", capi.Aedat4Options), ("ecal_aedat4_info", capi.Aedat4Info), ("ecal_aedat4_packet", capi.Aedat4Packet)):
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
    assert ctypes.sizeof(capi.Aedat4Packet) == 16 and capi.AEDAT4_PACKET_DTYPE.itemsize == 16
