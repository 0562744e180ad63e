"""GPU: the text ingest (include/ecal.h "text ingest"; eventcalib_amd/csrc/ecal_text.hip) — text event files parsed in HBM into
packed 25-byte records — against two independent oracles, byte for byte (no tolerance anywhere):
  1. `py_oracle`: the contract restated in Python (int(), float(), struct.pack("<dddB"), the filter, the duplicated last record);
  2. the repo's host converter opengv2::EventStream::txt2bin (eventcalib_amd/csrc/host/event.hpp: the reference's iostream loop),
     compiled here with g++ from a small driver written into the temporary directory.
Where the two oracles cannot agree the test says so: a text without any record line makes the host loop write one record of zeros
(its failed read — difference 2 of the contract; this library returns no record), the host converter has no start / end time (the
reading rule is applied to its records here) and always repeats the last record (duplicate_last=0 is compared with its output
minus that record)."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest
import torch

import eventcalib_amd
from eventcalib_amd import calibrate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

DRIVER_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "event.hpp"
// usage: drv host|device|load text.txt magnitude base|none end|none
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const long long none = std::numeric_limits<long long>::min();
    const double mag = std::atof(argv[3]);
    const long long base = std::strcmp(argv[4], "none") ? std::atoll(argv[4]) : none;
    const long long end = std::strcmp(argv[5], "none") ? std::atoll(argv[5]) : none;
    try {
        if (!std::strcmp(argv[1], "load")) {
            opengv2::EventContainer c;
            c.loadTextFile(argv[2], mag, base, end);
            std::printf("size %zu first %.17g last %.17g lines %llu\n", c.size(), c.firstTime(), c.lastTime(),
                        (unsigned long long) c.textInfo.n_lines);
            return 0;
        }
        const long long n = std::strcmp(argv[1], "host") ? opengv2::EventStream::txt2binDevice(argv[2], mag, base, end)
                                                         : opengv2::EventStream::txt2bin(argv[2], mag, base, end);
        std::printf("count %lld\n", n);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
"""


def py_oracle(text, time_magnitude=1e-6, time_base=None, end_stamp=None, start_time=-INF, end_time=None, duplicate_last=True):
    """The contract of include/ecal.h, restated: the records' bytes."""
    out, base, last = [], time_base, None
    for line in text.split(b"\n"):
        f = line.split()
        if not f:
            continue
        stamp, x, y, p = int(f[0]), float(f[1]), float(f[2]), int(f[3])
        base = stamp if base is None else base
        last = None
        if end_stamp is not None and stamp > end_stamp:
            break
        t = float(stamp - base) * time_magnitude
        if t < 0:
            continue
        if end_time is not None and t >= end_time:
            break
        if t >= start_time:
            last = struct.pack("<dddB", t, x, y, p)
            out.append(last)
    else:
        if duplicate_last and last is not None and text[-1:] in (b" ", b"\t", b"\r", b"\n"):
            out.append(last)
    return b"".join(out)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("text_driver")
    src, exe = str(d / "drv.cpp"), str(d / "drv")
    open(src, "w").write(DRIVER_SRC)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", exe, src,
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    return exe


def run_driver(driver, mode, path, time_magnitude=1e-6, time_base=None, end_stamp=None):
    out = subprocess.run([driver, mode, path, repr(float(time_magnitude)), "none" if time_base is None else str(time_base),
                          "none" if end_stamp is None else str(end_stamp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def host_txt2bin(driver, workdir, text, **kw):
    """bytes of the .bin the host converter writes from `text` (txt2bin's own arguments only)"""
    path = os.path.join(str(workdir), "host_oracle.txt")
    open(path, "wb").write(text)
    out = run_driver(driver, "host", path, **kw)
    data = open(path[:-4] + ".bin", "rb").read()
    assert out.split() == ["count", str(len(data) // 25)]
    return data


def reading_rule(records, start_time=-INF, end_time=None):
    """eventCameraCalib.cpp:154-163 over packed records: keep t >= start_time, stop at the first t >= end_time"""
    out = []
    for i in range(0, len(records), 25):
        t = struct.unpack_from("<d", records, i)[0]
        if end_time is not None and t >= end_time:
            break
        if t >= start_time:
            out.append(records[i:i + 25])
    return b"".join(out)


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


def ingest(ctx, text, **opts):
    ev, info = ctx.events_from_text(text, **opts)
    torch.cuda.synchronize()
    data = ev.cpu().numpy().tobytes()
    assert len(data) == 25 * info["n_events"]
    return data, info


THREE = b"5 1 2 1\n7 3.5 4 0\n9 10 11 1\n"
FIVE = b"100 1 2 1\n200 3 4 0\n300 5 6 1\n400 7 8 0\n500 9 10 1\n"
EDGE_CASES = [
    ("empty", b"", {}),
    ("blanks_only", b"  \n\t\n \r\n   ", {}),
    ("one_line_with_newline", b"5 1 2 1\n", {}),
    ("one_line_without_newline", b"5 1 2 1", {}),
    ("one_newline", b"\n", {}),
    ("three_lines", THREE, {}),
    ("three_lines_no_final_newline", THREE[:-1], {}),
    ("three_lines_no_duplicate", THREE, {"duplicate_last": False}),
    ("three_lines_trailing_blank_no_newline", THREE[:-1] + b" ", {}),
    ("crlf_tabs_blank_lines", b"\r\n5 1 2 1\r\n\r\n  \t\n7\t3.5  \t4 0\r\n\t9 10 11 1 \r\n\n\n", {}),
    ("minus_zero_and_point_five", b"5 -0 .5 1\n6 -0.0 -.5 0\n7 0 5. 1\n8 +.25 1e2 0", {}),
    ("negative_stamps_explicit_base", b"-5 1 2 1\n-3 3.5 4 0\n9 10 11 1\n", {"time_base": -4}),
    ("explicit_base_first_dropped", b"5 1 2 1\n7 3.5 4 0\n9 10 11 1\n3 1 1 1\n", {"time_base": 6}),
    ("explicit_base_last_dropped_no_duplicate_of_it", b"5 1 2 1\n7 3.5 4 0\n3 10 11 1\n", {"time_base": 4}),
    ("end_stamp_on_first_line", FIVE, {"end_stamp": 99}),
    ("end_stamp_in_the_middle", FIVE, {"end_stamp": 300}),
    ("end_stamp_between_lines", FIVE, {"end_stamp": 350}),
    ("end_stamp_on_last_line", FIVE, {"end_stamp": 499}),
    ("end_stamp_behind_last_line", FIVE, {"end_stamp": 500}),
    ("end_stamp_with_base", FIVE, {"end_stamp": 300, "time_base": 150}),
    ("start_time_seconds", FIVE, {"time_magnitude": 1e-2, "start_time": 1.5}),
    ("end_time_seconds", FIVE, {"time_magnitude": 1e-2, "end_time": 3.0}),
    ("start_and_end_time", FIVE, {"time_magnitude": 1e-2, "start_time": 1.0, "end_time": 4.0}),
    ("end_time_on_first_record", FIVE, {"time_magnitude": 1e-2, "end_time": 0.0}),
    ("start_time_behind_everything", FIVE, {"time_magnitude": 1e-2, "start_time": 9.0}),
    ("magnitude_one", FIVE, {"time_magnitude": 1.0, "time_base": 0}),
]


@pytest.mark.parametrize("name,text,opts", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_edge_files_against_both_oracles(ctx, driver, tmp_path, name, text, opts):
    got, info = ingest(ctx, text, **opts)
    want = py_oracle(text, **opts)
    print(name, "records", len(got) // 25, info)
    assert got == want
    assert info["n_host_lines"] == 0 and info["first_bad_line"] == 0
    assert info["n_lines"] == (text.count(b"\n") + (0 if text.endswith(b"\n") or not text else 1))
    assert info["n_blank"] == sum(1 for ln in text.split(b"\n")[:info["n_lines"]] if not ln.split())
    # every record line is kept, or dropped for exactly one reason
    dup = (len(want) - len(py_oracle(text, **dict(opts, duplicate_last=False)))) // 25
    assert info["n_events"] - dup + info["n_negative"] + info["n_after_end"] + info["n_before_start"] == info["n_lines"] - info["n_blank"]
    # the host converter (its own arguments: magnitude, base, end stamp), then what it cannot do itself
    host_kw = {k: v for k, v in opts.items() if k in ("time_magnitude", "time_base", "end_stamp")}
    host = host_txt2bin(driver, tmp_path, text, **host_kw)
    if not any(ln.split() for ln in text.split(b"\n")):
        assert host == bytes(25) and got == b""     # the host loop's failed read writes one record of zeros; no record here
        return
    host = reading_rule(host, opts.get("start_time", -INF), opts.get("end_time"))
    if opts.get("duplicate_last", True):
        assert got == host
    else:
        assert got + got[-25:] == host


# ---- boundaries: 300 000 lines that straddle every 16-byte load and every workgroup span -----------------------------------------
def _coordinate(rng):
    r = rng.random()
    if r < 0.5:
        return str(rng.randrange(1280))
    if r < 0.9:
        k = rng.randint(1, 14)
        j = rng.randint(1, 15 - k)
        return "%s%d.%0*d" % (rng.choice(["", "", "-", "+"]), rng.randrange(10 ** k), j, rng.randrange(10 ** j))
    if r < 0.95:
        return "%d.%de%s%d" % (rng.randrange(1, 1000), rng.randrange(1000), rng.choice(["", "+", "-"]), rng.randrange(8))
    return rng.choice(["-0", ".5", "5.", "-.125", "0.0", "007", "1E2"])


def _blank(rng, lo, hi):
    return "".join(rng.choice(" \t") for _ in range(rng.randint(lo, hi)))


@pytest.fixture(scope="module")
def big_lines():
    """300 000 record lines, stamps of 1 - 18 digits ascending, blank lines sprinkled in (a list of str, no line breaks).  The
    fields come from seeded pools (20 000 coordinates, the blank runs), so that building the text takes a second."""
    rng = random.Random(20240611)
    n = 300000
    stamps = sorted(rng.randrange(10 ** (d - 1), 10 ** d) for d in (rng.randint(1, 18) for _ in range(n)))
    coords = [_coordinate(rng) for _ in range(20000)]
    seps = [_blank(rng, 1, 3) for _ in range(512)]
    edges = [_blank(rng, 0, 2) for _ in range(256)] + [_blank(rng, 0, 5) for _ in range(256)]
    picks = np.random.default_rng(20240611).integers(0, 1 << 30, size=(n, 8)).tolist()
    lines = []
    for s, q in zip(stamps, picks):
        if q[7] % 20 == 0:      # the shortest form
            lines.append("%d %d %d %d" % (s, q[1] % 10, q[2] % 10, q[3] & 1))
        else:
            lines.append(edges[q[0] % 256] + str(s) + seps[q[1] % 512] + coords[q[2] % 20000] + seps[q[3] % 512] + coords[q[4] % 20000] +
                         seps[q[5] % 512] + "01"[q[6] & 1] + edges[(q[6] >> 1) % 256] + ("\r" if (q[6] >> 10) % 5 == 0 else ""))
        if q[7] % 50 == 1:
            lines.append(edges[256 + (q[0] >> 8) % 256])
    return lines


@pytest.fixture(scope="module")
def big_text(big_lines):
    text = ("\n".join(big_lines) + "\n").encode()
    if len(text) % 16 == 0:
        text += b"\n"
    return text


def test_boundaries_300k_lines_no_host_help(ctx, big_text):
    widths = [len(ln) for ln in big_text.split(b"\n")]
    print("line widths", min(w for w in widths if w > 6), "to", max(widths), "bytes;", len(big_text), "bytes of text")
    assert min(w for w in widths if w > 6) <= 8 and max(widths) >= 55
    assert len(big_text) > 1024 * 4096 and len(widths) > 1024 * 256      # both block scans (1024 counts a round) take more than one round
    want = py_oracle(big_text)
    got, info = ingest(ctx, big_text)
    print(info)
    assert info["n_host_lines"] == 0          # every line of this class is converted on the device: the host did none of the work
    assert got == want
    assert info["n_lines"] == len(widths) - 1 and info["n_events"] == 300001
    # the same text once more from a device tensor whose byte count is no multiple of 16 and which sits in front of other bytes
    # (record lines: a read behind n_bytes would show as records)
    assert len(big_text) % 16 != 0
    poison = b"\n999999999999999999 7 7 1\n" * 4
    whole = torch.from_numpy(np.frombuffer(big_text + poison, np.uint8).copy()).cuda()
    view = whole[: len(big_text)]
    assert view.data_ptr() % 16 == 0
    ev, info2 = ctx.events_from_text(view)
    assert ev.cpu().numpy().tobytes() == want and info2 == info
    assert ctx.text_count_lines(view) == info["n_lines"]
    # and half of it, without a final line break
    cut = big_text[: len(big_text) // 2]
    cut = cut[: cut.rfind(b"\n")]
    got3, info3 = ingest(ctx, cut)
    assert got3 == py_oracle(cut) and info3["n_host_lines"] == 0


# ---- host fallback -----------------------------------------------------------------------------------------------------------------
def test_host_fallback_counts_exactly_its_lines(ctx, driver, tmp_path):
    rng = random.Random(77)
    lines, n_slow = [], 0
    for i in range(2000):
        stamp = 1000 + 3 * i
        if rng.random() < 0.1:
            n_slow += 1
            kind = rng.randrange(3)
            if kind == 0:      # 17 - 19 significant digits
                d = rng.randint(17, 19)
                k = rng.randint(1, 4)
                digits = str(rng.randrange(10 ** (d - 1), 10 ** d))
                lines.append("%d %s.%s %d %d" % (stamp, digits[:k], digits[k:], rng.randrange(260), i & 1))
            elif kind == 1:    # the same in y, with an exponent
                d = rng.randint(17, 19)
                lines.append("%d %d %se-%d %d" % (stamp, rng.randrange(346), str(rng.randrange(10 ** (d - 1), 10 ** d)), d - 2, i & 1))
            else:              # longer than the device parser looks at
                lines.append("%d %d%s%d %d" % (stamp, rng.randrange(346), " " * rng.randint(130, 200), rng.randrange(260), i & 1))
        else:
            lines.append("%d %d %d.5 %d" % (stamp, rng.randrange(346), rng.randrange(260), i & 1))
    text = ("\n".join(lines) + "\n").encode()
    got, info = ingest(ctx, text)
    assert info["n_host_lines"] == n_slow and n_slow > 100
    assert got == py_oracle(text)
    assert got == host_txt2bin(driver, tmp_path, text)
    # the filter runs again behind the patch: a break that only a host-parsed line decides
    slow_at = next(i for i, ln in enumerate(lines) if len(ln) > 128)
    end = 1000 + 3 * slow_at - 1
    got2, info2 = ingest(ctx, text, end_stamp=end)
    assert got2 == py_oracle(text, end_stamp=end) and info2["n_events"] == slow_at and info2["n_after_end"] == 2000 - slow_at


# ---- errors ------------------------------------------------------------------------------------------------------------------------
MALFORMED = ["1 2 3", "1 2 3 1 5", "1 2 3 2", "12.5 1 2 1", "9223372036854775808 1 2 1", "1 1e 2 1", "1 - 2 1",
             "1 2 3 1" + " " * 140 + "x"]


@pytest.mark.parametrize("bad", MALFORMED, ids=["three_fields", "five_fields", "polarity_2", "stamp_12p5", "stamp_beyond_int64",
                                                "empty_exponent", "lone_minus", "overlong_five_fields"])
def test_malformed_line_is_an_error_and_names_the_line(ctx, tmp_path, bad):
    pos = 100 + 611 * MALFORMED.index(bad)     # (0-based line index; different workgroups of the parse pass)
    lines = ["%d %d %d %d" % (10 + i, i % 346, i % 260, i & 1) for i in range(5000)]
    good = ("\n".join(lines) + "\n").encode()
    lines[pos] = bad
    lines[4700] = "again not a record"         # a later offender: the FIRST one is reported
    text = ("\n".join(lines) + "\n").encode()
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_text(text)
    assert e.value.status == -1 and e.value.info["first_bad_line"] == pos + 1 and ("line %d" % (pos + 1)) in str(e.value)
    path = str(tmp_path / "bad.txt")
    open(path, "wb").write(text)
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.stream_from_text_file(path)         # no stream is created
    assert e.value.status == -1 and e.value.info["first_bad_line"] == pos + 1
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.text_to_bin(path, str(tmp_path / "bad.bin"))
    assert e.value.status == -1
    got, info = ingest(ctx, good)               # the context is usable afterwards
    assert got == py_oracle(good) and info["n_events"] == 5001


def test_too_small_capacity_reports_the_needed_count(ctx):
    text = FIVE * 300
    want = py_oracle(text)
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_text(text, capacity=700)
    assert e.value.status == -6 and e.value.info["n_events"] == len(want) // 25 == 1501
    ev, info = ctx.events_from_text(text, capacity=e.value.info["n_events"])
    assert ev.cpu().numpy().tobytes() == want
    with pytest.raises(eventcalib_amd.EcalError) as e:      # the duplicated record needs its slot too
        ctx.events_from_text(text, capacity=1500)
    assert e.value.status == -6 and e.value.info["n_events"] == 1501
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_text(text, capacity=0)
    assert e.value.status == -6


# ---- file level --------------------------------------------------------------------------------------------------------------------
def test_file_entry_points_against_the_host_converter(ctx, driver, tmp_path, big_lines):
    text = ("\n".join(big_lines[:100000]) + "\n").encode()
    host = host_txt2bin(driver, tmp_path, text)
    path = str(tmp_path / "events.txt")
    open(path, "wb").write(text)
    ev, info, t_first, t_last = ctx.stream_from_text_file(path)
    data = ev.cpu().numpy().tobytes()
    assert data == host and info["n_host_lines"] == 0 and info["n_lines"] == 100000
    assert struct.pack("<dd", t_first, t_last) == host[:8] + host[-25:-17]
    info2 = ctx.text_to_bin(path, str(tmp_path / "by_library.bin"))
    assert open(str(tmp_path / "by_library.bin"), "rb").read() == host and info2 == info
    # the C++ shims: txt2binDevice (same file name rule, same count), EventContainer::loadTextFile
    dev_txt = str(tmp_path / "shim.txt")
    open(dev_txt, "wb").write(text)
    out = run_driver(driver, "device", dev_txt)
    assert out.split() == ["count", str(len(host) // 25)]
    assert open(dev_txt[:-4] + ".bin", "rb").read() == host
    out = run_driver(driver, "load", dev_txt).split()
    assert out[:2] == ["size", str(len(host) // 25)] and out[-1] == "100000"
    assert struct.pack("<dd", float(out[3]), float(out[5])) == host[:8] + host[-25:-17]
    # an empty file is a stream of no events
    open(path, "wb").write(b"")
    ev, info, t_first, t_last = ctx.stream_from_text_file(path)
    assert ev.numel() == 0 and info["n_events"] == 0 and (t_first, t_last) == (0.0, 0.0)


def test_unsorted_text_file_becomes_a_time_ordered_stream(ctx, tmp_path):
    rng = random.Random(5)
    stamps = [rng.randrange(1, 10 ** 6) for _ in range(20000)]
    text = "".join("%d %d %d %d\n" % (s, i % 346, i % 260, i & 1) for i, s in enumerate(stamps)).encode()
    path = str(tmp_path / "unsorted.txt")
    open(path, "wb").write(text)
    ev, info, _, _ = ctx.stream_from_text_file(path, time_base=0)
    want = py_oracle(text, time_base=0)
    recs = [want[i:i + 25] for i in range(0, len(want), 25)]
    recs.sort(key=lambda r: struct.unpack_from("<d", r)[0])      # stable, like the multimap
    assert ev.cpu().numpy().tobytes() == b"".join(recs)
    assert ctx.events_from_text(text, time_base=0)[0].cpu().numpy().tobytes() == want     # the _dev form keeps the file order


def test_text_stream_detects_like_the_same_records(ctx, tmp_path):
    """A 60 000-event synthetic calibration stream written as text with integer microsecond stamps, loaded through
    calibrate.load_events_text: the detection pass sees what it sees on the same records packed directly."""
    import synth_stream as SS
    from eventcalib_amd.pipeline import DetectPipeline
    n = 60000
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cpu", seed=3))
    stamps = torch.round(t * 1e6).to(torch.int64)
    path = str(tmp_path / "synthetic.txt")
    with open(path, "w") as f:
        f.write("\n".join("%d %d %d %d" % (s, x, y, p) for s, (x, y), p in zip(stamps.tolist(), xy.to(torch.int64).tolist(), pol.tolist())))
    direct = SS.pack_records(stamps.to(torch.float64) * 1e-6, xy, pol)       # t = (double)(stamp - 0) * 1e-6
    events, t_first, t_last = calibrate.load_events_text(ctx, path, time_base=0)
    assert events.cpu().numpy().tobytes() == direct.numpy().tobytes()
    assert (t_first, t_last) == (float(stamps[0]) * 1e-6, float(stamps[-1]) * 1e-6)
    t0, t1 = SS.tiled_windows(t_first, t_last)
    infos = []
    pipe = DetectPipeline(ctx)
    pipe.set_windows(t0, t1)
    for buf in (events, direct.cuda()):
        pipe.run(buf)
        torch.cuda.synchronize()
        infos.append(pipe.win_info[: len(t0)].cpu().numpy().copy())
    assert (infos[0] == infos[1]).all() and int(infos[0][:, 1].sum()) > 0
