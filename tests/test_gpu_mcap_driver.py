"""GPU: the C++ shims of the mcap ingest (eventcalib_amd/csrc/host/event.hpp) through a small driver compiled into the temporary
directory: EventStream::mcap2bin (one host thread, the sequential decoder of mcap_events.hpp) and EventStream::mcap2binDevice
(ecal_mcap_to_bin_file) must write identical files for every kind; EventContainer::loadMcapFile must report the size and the first /
last time that loading that .bin reports; a file of compressed chunks raises.  And the product's driver in `batch` mode on the .mcap
of a synthetic calibration stream against the same run on the .bin that EventStream::mcap2bin makes of it, with the settings keys
Mcap_Topic, Mcap_TimeBase, Mcap_FlipX and Mcap_FlipY."""
import os
import subprocess

import numpy as np
import pytest

import mcap_writer as mw
import synth_stream as SS
import test_gpu_raw_ingest as RAW
from test_gpu_mcap_ingest import BASE, SCHEMAS, channels, cut, evt3_file, file_of, image, msg
from test_gpu_shims import SETTINGS_YAML

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "event.hpp"
// usage: drv host|device|loadmcap|loadbin file width height time_base|auto flip_y
int main(int argc, char **argv) {
    if (argc != 7) return 2;
    ecal_mcap_options opt;
    ecal_mcap_default_options(&opt);
    opt.width = (uint32_t) std::atoi(argv[3]);
    opt.height = (uint32_t) std::atoi(argv[4]);
    if (std::strcmp(argv[5], "auto")) {
        opt.auto_time_base = 0;
        opt.time_base = std::atoll(argv[5]);
    }
    opt.flip_y = std::atoi(argv[6]);
    try {
        if (!std::strcmp(argv[1], "loadmcap") || !std::strcmp(argv[1], "loadbin")) {
            opengv2::EventContainer c;
            if (!std::strcmp(argv[1], "loadmcap")) c.loadMcapFile(argv[2], &opt);
            else c.loadFile(argv[2], -std::numeric_limits<double>::infinity());
            std::printf("size %zu first %.17g last %.17g messages %llu base %lld kind %u\n", c.size(), c.firstTime(), c.lastTime(),
                        (unsigned long long) c.mcapInfo.n_messages, (long long) c.mcapInfo.time_base, c.mcapInfo.layout.kind);
            return 0;
        }
        ecal_mcap_info info;
        const long long n = std::strcmp(argv[1], "host") ? opengv2::EventStream::mcap2binDevice(argv[2], &opt, &info)
                                                         : opengv2::EventStream::mcap2bin(argv[2], &opt, &info);
        std::printf("count %lld raw %llu outside %llu negative %llu before %llu after %llu messages %llu other %llu chunks %llu schemas %llu channels %llu "
                    "trailing %llu first %lld base %lld size %u x %u payload %llu nostate %llu otherwords %llu wraps %llu kind %u lead %u stride %u\n", n,
                    (unsigned long long) info.n_raw_events, (unsigned long long) info.n_outside, (unsigned long long) info.n_negative,
                    (unsigned long long) info.n_before_start, (unsigned long long) info.n_after_end, (unsigned long long) info.n_messages,
                    (unsigned long long) info.n_other_messages, (unsigned long long) info.n_chunks, (unsigned long long) info.n_schemas,
                    (unsigned long long) info.n_channels, (unsigned long long) info.n_trailing_bytes, (long long) info.first_stamp_ns,
                    (long long) info.time_base, info.msg_width, info.msg_height, (unsigned long long) info.n_payload_bytes,
                    (unsigned long long) info.n_no_state, (unsigned long long) info.n_other_words, (unsigned long long) info.n_time_wraps,
                    info.layout.kind, info.layout.lead, info.layout.stride);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("mcap_driver")
    src, exe = str(d / "drv.cpp"), str(d / "drv")
    open(src, "w").write(DRIVER_SRC)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", exe, src,
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    return exe


def run(driver, mode, path, width=0, height=0, time_base="auto", flip_y=0, ok=True):
    out = subprocess.run([driver, mode, path, str(width), str(height), str(time_base), str(flip_y)], capture_output=True, text=True, timeout=120)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out.stdout


def random_file(kind, n, seed):
    """n random events — a tenth outside 346 x 260 — in messages of 0 .. 3000, images in between, cut short in the summary section"""
    rng = np.random.default_rng(seed)
    ev = (rng.integers(0, 380, n), rng.integers(0, 290, n), BASE + 400000000 + np.cumsum(rng.integers(0, 20000, n)), rng.integers(0, 2, n))
    messages, a = [], 0
    while a < n:
        b = min(n, a + int(rng.integers(0, 3000)))
        messages += [msg(kind, cut(ev, a, b), frame_id=b"cam0"[: len(messages) % 5]), image(int(rng.integers(0, 200)))]
        a = b
    return file_of(kind, messages, per_chunk=[3, 8, 1])[: -40]


@pytest.mark.parametrize("kind", [mw.STRUCT, mw.MONO])
def test_host_and_device_converters_write_identical_files(driver, tmp_path, kind):
    data = random_file(kind, 60000, 77)
    host, dev = str(tmp_path / "host.mcap"), str(tmp_path / "device.mcap")
    for path in (host, dev):
        open(path, "wb").write(data)
    late = BASE + 500000000        # a time base behind the first events
    for size in ((0, 0, "auto", 0), (346, 260, late, 1)):          # without bounds; with bounds, the flip of y and a time base
        a = run(driver, "host", host, *size)
        b = run(driver, "device", dev, *size)
        print(a)
        assert a == b and int(a.split()[1]) > 30000
        out = open(host[:-5] + ".bin", "rb").read()
        assert out == open(dev[:-5] + ".bin", "rb").read() and len(out) == 25 * int(a.split()[1])
        want, info, _ = mw.decode(data, time_base=None if size[2] == "auto" else late, width=size[0], height=size[1], flip_y=bool(size[3]))
        assert out == want and ("base %d " % info["time_base"]) in a and ("first %d " % BASE) in a and ("kind %d " % kind) in a
    assert " outside 0 " not in a and " negative 0 " not in a and " other 0 " not in a and "size 346 x 260" in a
    # a file of compressed chunks: both refuse, name the compression and say what to do
    open(host, "wb").write(file_of(kind, [msg(kind, cut((np.arange(3), np.arange(3), BASE + np.arange(3), np.arange(3) & 1), 0, 3))], compression="zstd"))
    for mode in ("host", "device", "loadmcap"):
        said = run(driver, mode, host, ok=False)
        assert "exception" in said and "zstd" in said and "uncompressed" in said


def test_evt3_packets_through_both_converters(driver, tmp_path):
    payload = RAW.payload_of(RAW.random_words("EVT3", 40000, 9), "EVT3")
    data, _ = evt3_file(payload, np.random.default_rng(2))
    host, dev = str(tmp_path / "host.mcap"), str(tmp_path / "device.mcap")
    for path in (host, dev):
        open(path, "wb").write(data)
    for size in ((0, 0, "auto"), (1280, 720, 1500)):
        a, b = run(driver, "host", host, *size), run(driver, "device", dev, *size)
        assert a == b and int(a.split()[1]) > 1000 and "kind 3 " in a and ("payload %d " % len(payload)) in a
        assert open(host[:-5] + ".bin", "rb").read() == open(dev[:-5] + ".bin", "rb").read()
    for mode, path in (("host", host), ("device", dev)):          # no flips for evt3 packets
        said = run(driver, mode, path, 1280, 720, "auto", 1, ok=False)
        assert "exception" in said and "evt3" in said and "flip" in said


def stream_events(n=200000, seed=3):
    import torch
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cpu", seed=seed))
    t_ns = torch.round(t * 1e9).to(torch.int64) + BASE + 250000000
    base = int(t_ns[0]) // 10 ** 9 * 10 ** 9
    records = SS.pack_records((t_ns - base).to(torch.float64) * 1e-9, xy, pol).numpy().tobytes()
    return (xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(), t_ns.numpy(), pol.to(torch.int64).numpy()), records, base


def to_messages(kind, ev, per=4096, between=None):
    messages = []
    for i, a in enumerate(range(0, len(ev[0]), per)):
        messages.append(msg(kind, cut(ev, a, a + per), frame_id=b"davis"[: i % 6]))
        if between is not None:
            messages += between(i)
    return messages


@pytest.mark.parametrize("kind", [mw.STRUCT, mw.MONO])
def test_load_mcap_file_reports_what_loading_the_bin_reports(driver, tmp_path, kind):
    ev, records, base = stream_events()
    binf, path = str(tmp_path / "events.bin"), str(tmp_path / "events.mcap")
    open(binf, "wb").write(records)
    open(path, "wb").write(file_of(kind, to_messages(kind, ev, between=lambda i: [image(51 + i % 4)] * (i % 2))))
    b = run(driver, "loadbin", binf).split()
    for time_base in ("auto", base):
        a = run(driver, "loadmcap", path, time_base=time_base).split()
        assert a[:6] == b[:6] and a[1] == "200000" and a[7] == "49" and a[9] == str(base) and a[11] == str(kind)
    assert np.frombuffer(records[:8], "<f8")[0] == float(a[3]) and np.frombuffer(records[-25:-17], "<f8")[0] == float(a[5])


def test_driver_in_batch_mode_reads_an_mcap_file(driver, tmp_path):
    """unit_test_eventCameraCalib <settings> <events> <dir> batch on events.mcap (images between the event messages; epoch stamps,
    Mcap_TimeBase and Mcap_Topic given) and on the .bin that EventStream::mcap2bin — the sequential host decoder — makes of the same
    file.  The records in HBM are the same bytes, so the keyframe and init lines are the same text; the refined line is held to
    test_gpu_shims.py's figure for two runs of the chain (the solve sums with FP64 atomics), and for the same reason the trajectory
    file is held to its stamps."""
    exe = os.path.join(ROOT, "eventcalib_amd", "unit_test_eventCameraCalib")
    if not os.path.exists(exe):      # (it travels to the GPU box prebuilt, like libecal.so)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eventcalib_amd", "csrc"), "driver"])
    SS.TRAJECTORY = "orbit"
    try:
        n = 2_000_000
        buf = SS.make_stream(n, rate=1.0e6, t_start=5.0, device="cpu", seed=21)
    finally:
        SS.TRAJECTORY = "hover"
    import torch
    t, xy, pol = SS.unpack_records(buf)
    base = BASE + 123456789
    ev = (xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(), (torch.round(t * 1e9).to(torch.int64) + base).numpy(), pol.to(torch.int64).numpy())
    path = str(tmp_path / "events.mcap")
    between = lambda i: [image(346 * 260 + 7)] if i % 8 == 0 else [image(51)] * (i % 2)
    open(path, "wb").write(file_of(mw.STRUCT, to_messages(mw.STRUCT, ev, between=between), per_chunk=[6, 3]))
    said = run(driver, "host", path, 346, 0, base)        # the oracle: events.bin beside the file, by the host decoder (no flip)
    assert said.split()[1] == str(n) and ("base %d " % base) in said
    binf = str(tmp_path / "events.bin")
    outs, dirs = {}, {}
    for name, events, extra in (("bin", binf, ""), ("mcap", path, "Mcap_TimeBase: %d\nMcap_Topic: /dvs/events\nMcap_FlipX: 0\nMcap_FlipY: 0\n" % base)):
        d = tmp_path / name
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(SETTINGS_YAML % dict(start=5, end=8) + extra)
        out = subprocess.run([exe, yamlf, events, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = [ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")]
        dirs[name] = d
    assert outs["mcap"][0] == "mcap_time_base %d" % base          # the base in force is printed
    a, b = outs["mcap"][1:], outs["bin"]
    print("\n".join(a))
    assert [ln.split()[0] for ln in a] == ["keyframes", "init", "refined"] == [ln.split()[0] for ln in b]
    assert a[0] == b[0] and a[1] == b[1] and int(a[0].split()[1]) > 20
    ra, rb = a[2].split(), b[2].split()
    assert np.abs(np.array([float(v) for v in ra[1:10]]) - np.array([float(v) for v in rb[1:10]])).max() < 1e-9 * 400 and ra[10:] == rb[10:]
    files = lambda d: sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)
    assert files(dirs["mcap"]) == files(dirs["bin"]) and "TrajectoryByEvent.txt" in files(dirs["mcap"])
    ta, tb = (open(str(dirs[k] / "TrajectoryByEvent.txt")).read().split("\n") for k in ("mcap", "bin"))
    assert len(ta) == len(tb) > 20 and [ln.split()[:1] for ln in ta] == [ln.split()[:1] for ln in tb]
    # the settings keys are read: another topic finds no channel
    settings = open(str(dirs["mcap"] / "settings.yaml")).read()
    open(str(tmp_path / "other.yaml"), "w").write(settings.replace("Mcap_Topic: /dvs/events", "Mcap_Topic: /other/events"))
    out = subprocess.run([exe, str(tmp_path / "other.yaml"), path, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "/other/events" in out.stderr and "no channel" in out.stderr
    # a file of compressed chunks ends the driver with the library's text and exit code 4
    open(path, "wb").write(file_of(mw.STRUCT, to_messages(mw.STRUCT, cut(ev, 0, 10)), compression="lz4"))
    out = subprocess.run([exe, str(dirs["mcap"] / "settings.yaml"), path, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "lz4" in out.stderr and "uncompressed" in out.stderr
    # ... and so does a ROS 1 bag under the name .mcap
    open(path, "wb").write(b"#ROSBAG V2.0\n" + bytes(4096))
    out = subprocess.run([exe, str(dirs["mcap"] / "settings.yaml"), path, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "ROS 1 bag" in out.stderr
