"""GPU: the C++ shims of the AEDAT 4 ingest (eventcalib_amd/csrc/host/event.hpp) through a small driver compiled into the temporary
directory: EventStream::aedat42bin (one host thread, the sequential decoder of aedat4_events.hpp) and EventStream::aedat42binDevice
(ecal_aedat4_to_bin_file) must write identical files, which are also the Python oracle's; EventContainer::loadAedat4File must report
the size and the first / last time that loading that .bin reports.  And the product's driver in `batch` mode on the .aedat4 of a
synthetic calibration stream against the same run on the .bin of the same events."""
import os
import subprocess

import numpy as np
import pytest

import aedat4_oracle as AO
import aedat4_writer as AW
import synth_stream as SS
from test_gpu_shims import SETTINGS_YAML

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "event.hpp"
// usage: drv host|device|loadaedat4|loadbin file width height time_base   (time_base < 0: automatic)
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    ecal_aedat4_options opt;
    ecal_aedat4_default_options(&opt);
    opt.width = (uint32_t) std::atoi(argv[3]);
    opt.height = (uint32_t) std::atoi(argv[4]);
    if (std::atoll(argv[5]) >= 0) {
        opt.auto_time_base = 0;
        opt.time_base = std::atoll(argv[5]);
    }
    opt.flip_y = opt.height ? 1 : 0;
    try {
        if (!std::strcmp(argv[1], "loadaedat4") || !std::strcmp(argv[1], "loadbin")) {
            opengv2::EventContainer c;
            if (!std::strcmp(argv[1], "loadaedat4")) c.loadAedat4File(argv[2], &opt);
            else c.loadFile(argv[2], -std::numeric_limits<double>::infinity());
            std::printf("size %zu first %.17g last %.17g packets %llu stream %d\n", c.size(), c.firstTime(), c.lastTime(),
                        (unsigned long long) c.aedat4Info.n_packets, c.aedat4Info.stream_id);
            return 0;
        }
        ecal_aedat4_info info;
        const long long n = std::strcmp(argv[1], "host") ? opengv2::EventStream::aedat42binDevice(argv[2], &opt, &info)
                                                         : opengv2::EventStream::aedat42bin(argv[2], &opt, &info);
        std::printf("count %lld raw %llu outside %llu negative %llu before %llu after %llu packets %llu other_packets %llu trailing %llu "
                    "compressed %llu inflated %llu first_stamp %lld time_base %lld compression %d stream %d\n", n,
                    (unsigned long long) info.n_raw_events, (unsigned long long) info.n_outside, (unsigned long long) info.n_negative,
                    (unsigned long long) info.n_before_start, (unsigned long long) info.n_after_end, (unsigned long long) info.n_packets,
                    (unsigned long long) info.n_other_packets, (unsigned long long) info.n_trailing_bytes,
                    (unsigned long long) info.n_compressed_bytes, (unsigned long long) info.n_inflated_bytes, (long long) info.first_stamp_us,
                    (long long) info.time_base, info.compression, info.stream_id);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("aedat4_driver")
    src, exe = str(d / "drv.cpp"), str(d / "drv")
    open(src, "w").write(DRIVER_SRC)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", exe, src,
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    return exe


def run(driver, mode, path, width=0, height=0, time_base=-1, ok=True):
    out = subprocess.run([driver, mode, path, str(width), str(height), str(time_base)], capture_output=True, text=True, timeout=120)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out.stdout


def encode4(t_us, x, y, on, per=4096, compress_every=0, between=None, stream=1, **build):
    """the events in packets of `per` as an AEDAT 4 file (LZ4): stored blocks, every compress_every-th packet truly compressed;
    between(k): a foreign packet's (stream id, FlatBuffer) in front of packet k, or None"""
    ev = AW.make_events(t_us, x, y, on)
    chain = []
    for k, a in enumerate(range(0, len(ev), per)):
        extra = between(k) if between else None
        if extra is not None:
            chain.append((extra[0], AW.lz4_stored_frame(extra[1])))
        fb = AW.event_packet(ev[a:a + per])
        chain.append((stream, AW.lz4_compressed_frame(fb) if compress_every and k % compress_every == 0 else AW.lz4_stored_frame(fb)))
    return AW.build_file(chain, AW.LZ4, **build)


def test_host_and_device_converters_write_identical_files(driver, tmp_path):
    rng = np.random.default_rng(77)
    n = 100000
    x, y, on = rng.integers(-5, 380, n), rng.integers(-5, 290, n), rng.integers(0, 2, n)       # a tenth outside 346 x 260
    t_us = 1_700_000_000_400_000 + np.cumsum(rng.integers(0, 20, n))
    # a recording that was never closed (dataTablePosition -1), cut inside a packet's header
    data = encode4(t_us, x, y, on, per=3000, compress_every=9, data_table=False,
                   between=lambda k: (2 + k % 2, AW.foreign_packet(64 + 977 * (k % 5), seed=k)) if k % 3 == 0 else None) + b"\x01\x00\x00\x00\x10"
    host, dev = str(tmp_path / "host.aedat4"), str(tmp_path / "device.aedat4")
    for path in (host, dev):
        open(path, "wb").write(data)
    late = int(t_us[0]) + 6000                       # a time base behind the first events
    for size, opts in (((0, 0, -1), dict()), ((346, 260, late), dict(width=346, height=260, flip_y=True, time_base=late))):
        a = run(driver, "host", host, *size)
        b = run(driver, "device", dev, *size)
        print(a)
        assert a == b and int(a.split()[1]) > 50000
        out = open(host[:-7] + ".bin", "rb").read()
        assert out == open(dev[:-7] + ".bin", "rb").read() and len(out) == 25 * int(a.split()[1])
        want, info = AO.decode(data, **opts)
        assert out == want.tobytes()
        w = a.split()
        said = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
        assert said == dict(count=info["n_events"], raw=info["n_raw_events"], outside=info["n_outside"], negative=info["n_negative"],
                            before=info["n_before_start"], after=info["n_after_end"], packets=info["n_packets"],
                            other_packets=info["n_other_packets"], trailing=info["n_trailing_bytes"], compressed=info["n_compressed_bytes"],
                            inflated=info["n_inflated_bytes"], first_stamp=info["first_stamp_us"], time_base=info["time_base"],
                            compression=1, stream=1)
    assert "outside 0 " not in a and "negative 0 " not in a and "other_packets 12 " in a and "trailing 5 " in a
    # a ZSTD file, and one cut short before its header: both refuse, and say AEDAT 4
    for bad, word in ((AW.build_file([(1, AW.event_packet(AW.make_events([1], [1], [1], [1])))], AW.ZSTD), "ZSTD"), (AW.VERSION_LINE, "cut short")):
        open(host, "wb").write(bad)
        for mode in ("host", "device", "loadaedat4"):
            said = run(driver, mode, host, ok=False)
            assert "exception" in said and "AEDAT 4" in said and word in said


def test_load_aedat4_file_reports_what_loading_the_bin_reports(driver, tmp_path):
    rng = np.random.default_rng(5)
    n = 200000
    base = 1_700_000_123_000_000
    t_us = base + 5_000_000 + np.sort(rng.integers(0, 3_000_000, n))
    x, y, on = rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n)
    path, binf = str(tmp_path / "events.aedat4"), str(tmp_path / "plain.bin")
    data = encode4(t_us, x, y, on, compress_every=16)
    open(path, "wb").write(data)
    want, info = AO.decode(data, time_base=base)
    open(binf, "wb").write(want.tobytes())
    a = run(driver, "loadaedat4", path, time_base=base).split()
    b = run(driver, "loadbin", binf).split()
    assert a[:6] == b[:6] and a[1] == "200000" and a[7] == str((n + 4095) // 4096) and a[9] == "1"
    rec = want.tobytes()
    assert np.frombuffer(rec[:8], "<f8")[0] == float(a[3]) and np.frombuffer(rec[-25:-17], "<f8")[0] == float(a[5])


def test_driver_in_batch_mode_reads_an_aedat4_file(tmp_path):
    """unit_test_eventCameraCalib <settings> <events> <dir> batch on events.aedat4 (LZ4: stored blocks for most packets, a few packets
    truly compressed, frames between the event packets; the file's clock is set by Aedat4_TimeBase) and on the .bin of the same
    events.  The records in HBM are the same bytes, so the keyframe and init lines are the same text; the refined line is held to
    test_gpu_aedat_driver.py's figure for two runs of the chain (the solve sums with FP64 atomics)."""
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
    t_us = torch.round(t * 1e6).to(torch.int64)
    base = 1_700_000_000_000_000 + 123456789
    binf, aedat4 = str(tmp_path / "events.bin"), str(tmp_path / "events.aedat4")
    SS.pack_records(t_us.to(torch.float64) * 1e-6, xy, pol).numpy().tofile(binf)
    frame = AW.foreign_packet(36 + 346 * 260 * 2, seed=1)
    imu = AW.foreign_packet(12 + 51 * 2, identifier=b"IMUS", seed=2)
    between = lambda k: (0, frame) if k % 8 == 0 else (2, imu) if k % 2 else None
    data = encode4(t_us.numpy() + base, xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(), pol.to(torch.int64).numpy(),
                   compress_every=97, between=between)
    open(aedat4, "wb").write(data)
    outs = {}
    for name, path, extra in (("bin", binf, ""), ("aedat4", aedat4, "Aedat4_TimeBase: %d\n" % base)):
        d = tmp_path / name
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(SETTINGS_YAML % dict(start=5, end=8) + extra)
        out = subprocess.run([exe, yamlf, path, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = [ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")]
    a, b = outs["aedat4"], outs["bin"]
    print("\n".join(a))
    assert a[0] == "aedat4_time_base %d" % base
    a = a[1:]
    assert [ln.split()[0] for ln in a] == ["keyframes", "init", "refined"] == [ln.split()[0] for ln in b]
    assert a[0] == b[0] and a[1] == b[1] and int(a[0].split()[1]) > 20
    ra, rb = a[2].split(), b[2].split()
    assert np.abs(np.array([float(v) for v in ra[1:10]]) - np.array([float(v) for v in rb[1:10]])).max() < 1e-9 * 400 and ra[10:] == rb[10:]
    # a file the driver cannot read ends it with the library's text and exit code 4
    open(aedat4, "wb").write(AW.build_file([(1, AW.event_packet(AW.make_events([1], [1], [1], [1])))], AW.ZSTD_HIGH))
    out = subprocess.run([exe, str(tmp_path / "aedat4" / "settings.yaml"), aedat4, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "AEDAT 4" in out.stderr and "ZSTD_HIGH" in out.stderr
