"""GPU: the C++ shims of the bag ingest (eventcalib_amd/csrc/host/event.hpp) through a small driver compiled into the temporary
directory: EventStream::bag2bin (one host thread, the sequential decoder of bag_events.hpp) and EventStream::bag2binDevice
(ecal_bag_to_bin_file) must write identical files; EventContainer::loadBagFile must report the size and the first / last time that
loading that .bin reports; a bag of compressed chunks raises.  And the product's driver in `batch` mode on the .bag of a synthetic
calibration stream against the same run on the .bin that EventStream::bag2bin makes of it."""
import os
import subprocess

import numpy as np
import pytest

import bag_writer as bw
import synth_stream as SS
from test_gpu_bag_ingest import CONNS, S0, image, msg, synthetic  # noqa: F401  (synthetic: a fixture)
from test_gpu_shims import SETTINGS_YAML

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "event.hpp"
// usage: drv host|device|loadbag|loadbin file width height time_base|auto
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    ecal_bag_options opt;
    ecal_bag_default_options(&opt);
    opt.width = (uint32_t) std::atoi(argv[3]);
    opt.height = (uint32_t) std::atoi(argv[4]);
    if (std::strcmp(argv[5], "auto")) {
        opt.auto_time_base = 0;
        opt.time_base = std::atoll(argv[5]);
    }
    opt.flip_y = opt.height ? 1 : 0;
    try {
        if (!std::strcmp(argv[1], "loadbag") || !std::strcmp(argv[1], "loadbin")) {
            opengv2::EventContainer c;
            if (!std::strcmp(argv[1], "loadbag")) c.loadBagFile(argv[2], &opt);
            else c.loadFile(argv[2], -std::numeric_limits<double>::infinity());
            std::printf("size %zu first %.17g last %.17g messages %llu base %lld\n", c.size(), c.firstTime(), c.lastTime(),
                        (unsigned long long) c.bagInfo.n_messages, (long long) c.bagInfo.time_base);
            return 0;
        }
        ecal_bag_info info;
        const long long n = std::strcmp(argv[1], "host") ? opengv2::EventStream::bag2binDevice(argv[2], &opt, &info)
                                                         : opengv2::EventStream::bag2bin(argv[2], &opt, &info);
        std::printf("count %lld raw %llu outside %llu negative %llu before %llu after %llu messages %llu other %llu chunks %llu connections %llu "
                    "trailing %llu first %lld base %lld size %u x %u\n", n, (unsigned long long) info.n_raw_events, (unsigned long long) info.n_outside,
                    (unsigned long long) info.n_negative, (unsigned long long) info.n_before_start, (unsigned long long) info.n_after_end,
                    (unsigned long long) info.n_messages, (unsigned long long) info.n_other_messages, (unsigned long long) info.n_chunks,
                    (unsigned long long) info.n_connections, (unsigned long long) info.n_trailing_bytes, (long long) info.first_stamp_ns,
                    (long long) info.time_base, info.msg_width, info.msg_height);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("bag_driver")
    src, exe = str(d / "drv.cpp"), str(d / "drv")
    open(src, "w").write(DRIVER_SRC)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", exe, src,
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    return exe


def run(driver, mode, path, width=0, height=0, time_base="auto", ok=True):
    out = subprocess.run([driver, mode, path, str(width), str(height), str(time_base)], capture_output=True, text=True, timeout=120)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out.stdout


def events_to_messages(t_ns, x, y, p, per=4096, between=None):
    messages = []
    for i, a in enumerate(range(0, len(t_ns), per)):
        s = slice(a, a + per)
        messages.append(msg(bw.events_array(x[s], y[s], t_ns[s] // 10 ** 9, t_ns[s] % 10 ** 9, p[s]), frame_id=b"davis"[: i % 6], seq=i))
        if between is not None:
            messages += between(i)
    return messages


def random_bag(n, seed):
    """a bag of n random events — a tenth outside 346 x 260, polarity bytes of every value, images and IMU samples in between"""
    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, 380, n), rng.integers(0, 290, n)
    p = np.where(rng.integers(0, 8, n) == 0, rng.integers(0, 256, n), rng.integers(0, 2, n))
    t_ns = S0 * 10 ** 9 + 400000000 + np.cumsum(rng.integers(0, 20000, n))
    messages, a = [], 0
    while a < n:
        b = min(n, a + int(rng.integers(0, 3000)))
        messages.append(msg(bw.events_array(x[a:b], y[a:b], t_ns[a:b] // 10 ** 9, t_ns[a:b] % 10 ** 9, p[a:b]), frame_id=b"cam0"[: len(messages) % 5]))
        messages.append(image(int(rng.integers(0, 200)), conn=1 + len(messages) % 2))
        a = b
    return bw.write_bag(CONNS, messages, per_chunk=[3, 8, 1]) [: -7]       # (cut short in the last chunk info record)


def test_host_and_device_converters_write_identical_files(driver, tmp_path):
    data = random_bag(100000, 77)
    host, dev = str(tmp_path / "host.bag"), str(tmp_path / "device.bag")
    for path in (host, dev):
        open(path, "wb").write(data)
    late = S0 * 10 ** 9 + 500000000        # a time base behind the first events
    for size in ((0, 0, "auto"), (346, 260, late)):          # without bounds; with bounds, the flip of y and a time base
        a = run(driver, "host", host, *size)
        b = run(driver, "device", dev, *size)
        print(a)
        assert a == b and int(a.split()[1]) > 50000
        out = open(host[:-4] + ".bin", "rb").read()
        assert out == open(dev[:-4] + ".bin", "rb").read() and len(out) == 25 * int(a.split()[1])
        want, info, _ = bw.decode(data, time_base=None if size[2] == "auto" else late, width=size[0], height=size[1], flip_y=bool(size[1]))
        assert out == want and ("base %d " % info["time_base"]) in a and ("first %d " % (S0 * 10 ** 9)) in a
    assert " outside 0 " not in a and " negative 0 " not in a and " other 0 " not in a and " trailing 0 " not in a and "size 346 x 260" in a
    # a bag of compressed chunks: both refuse, name the compression and say what to do
    open(host, "wb").write(bw.write_bag(CONNS, [msg(bw.events_array([1], [2], [S0], [3], [1]))], compression="bz2"))
    for mode in ("host", "device", "loadbag"):
        said = run(driver, mode, host, ok=False)
        assert "exception" in said and "bz2" in said and "rosbag decompress" in said


def test_load_bag_file_reports_what_loading_the_bin_reports(driver, tmp_path, synthetic):  # noqa: F811
    t_ns, x, y, p, records, base = synthetic
    binf, path = str(tmp_path / "events.bin"), str(tmp_path / "events.bag")
    open(binf, "wb").write(records)
    open(path, "wb").write(bw.write_bag(CONNS, events_to_messages(t_ns, x, y, p, between=lambda i: [image(51 + i % 4, conn=2)] * (i % 2))))
    b = run(driver, "loadbin", binf).split()
    for time_base in ("auto", base):
        a = run(driver, "loadbag", path, time_base=time_base).split()
        assert a[:6] == b[:6] and a[1] == "200000" and a[7] == "49" and a[9] == str(base)
    assert np.frombuffer(records[:8], "<f8")[0] == float(a[3]) and np.frombuffer(records[-25:-17], "<f8")[0] == float(a[5])


def test_driver_in_batch_mode_reads_a_bag(driver, tmp_path):
    """unit_test_eventCameraCalib <settings> <events> <dir> batch on events.bag (images between the event messages; epoch stamps,
    Bag_TimeBase given) and on the .bin that EventStream::bag2bin — the sequential host decoder — makes of the same bag.  The records
    in HBM are the same bytes, so the keyframe and init lines are the same text; the refined line is held to test_gpu_shims.py's figure
    for two runs of the chain (the solve sums with FP64 atomics), and for the same reason the trajectory file is held to its stamps."""
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
    base = S0 * 10 ** 9 + 123456789
    t_ns = (torch.round(t * 1e9).to(torch.int64) + base).numpy()
    bag = str(tmp_path / "events.bag")
    between = lambda i: [image(346 * 260 + 7)] if i % 8 == 0 else [image(51, conn=2)] * (i % 2)
    open(bag, "wb").write(bw.write_bag(CONNS, events_to_messages(t_ns, xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(),
                                                                 pol.to(torch.int64).numpy(), between=between), per_chunk=[6, 3]))
    said = run(driver, "host", bag, 346, 0, base)        # the oracle: events.bin beside the bag, by the host decoder (no flip)
    assert said.split()[1] == str(n) and ("base %d " % base) in said
    binf = str(tmp_path / "events.bin")
    outs, dirs = {}, {}
    for name, path, extra in (("bin", binf, ""), ("bag", bag, "Bag_TimeBase: %d\nBag_Topic: /dvs/events\n" % base)):
        d = tmp_path / name
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(SETTINGS_YAML % dict(start=5, end=8) + extra)
        out = subprocess.run([exe, yamlf, path, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = [ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")]
        dirs[name] = d
    assert outs["bag"][0] == "bag_time_base %d" % base          # the base in force is printed
    a, b = outs["bag"][1:], outs["bin"]
    print("\n".join(a))
    assert [ln.split()[0] for ln in a] == ["keyframes", "init", "refined"] == [ln.split()[0] for ln in b]
    assert a[0] == b[0] and a[1] == b[1] and int(a[0].split()[1]) > 20
    ra, rb = a[2].split(), b[2].split()
    assert np.abs(np.array([float(v) for v in ra[1:10]]) - np.array([float(v) for v in rb[1:10]])).max() < 1e-9 * 400 and ra[10:] == rb[10:]
    files = lambda d: sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)
    assert files(dirs["bag"]) == files(dirs["bin"]) and "TrajectoryByEvent.txt" in files(dirs["bag"])
    ta, tb = (open(str(dirs[k] / "TrajectoryByEvent.txt")).read().split("\n") for k in ("bag", "bin"))
    assert len(ta) == len(tb) > 20 and [ln.split()[:1] for ln in ta] == [ln.split()[:1] for ln in tb]
    # a bag of compressed chunks ends the driver with the library's text and exit code 4
    open(bag, "wb").write(bw.write_bag(CONNS, [msg(bw.events_array([1], [2], [S0], [3], [1]))], compression="lz4"))
    out = subprocess.run([exe, str(tmp_path / "bag" / "settings.yaml"), bag, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "lz4" in out.stderr and "rosbag decompress" in out.stderr
    # ... and so does a ROS 2 file under the name .bag
    open(bag, "wb").write(b"SQLite format 3\0" + bytes(4096))
    out = subprocess.run([exe, str(tmp_path / "bag" / "settings.yaml"), bag, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "ROS 2" in out.stderr
