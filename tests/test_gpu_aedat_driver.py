"""GPU: the C++ shims of the AEDAT ingest (eventcalib_amd/csrc/host/event.hpp) through a small driver compiled into the temporary
directory: EventStream::aedat2bin (one host thread, the sequential decoder of aedat_events.hpp) and EventStream::aedat2binDevice
(ecal_aedat_to_bin_file) must write identical files; EventContainer::loadAedatFile must report the size and the first / last time
that loading that .bin reports; a file of version 4.0 raises.  And the product's driver in `batch` mode on the .aedat of a synthetic
calibration stream against the same run on the .bin of the same events."""
import os
import subprocess

import numpy as np
import pytest

import synth_stream as SS
from test_gpu_aedat_ingest import HEADER20, HEADER31, encode20, encode31, ev, foreign, polarity, synthetic  # noqa: F401  (synthetic: a fixture)
from test_gpu_shims import SETTINGS_YAML

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "event.hpp"
// usage: drv host|device|loadaedat|loadbin file width height time_base
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    ecal_aedat_options opt;
    ecal_aedat_default_options(&opt);
    opt.width = (uint32_t) std::atoi(argv[3]);
    opt.height = (uint32_t) std::atoi(argv[4]);
    opt.time_base = std::atoll(argv[5]);
    opt.flip_y = opt.height ? 1 : 0;
    try {
        if (!std::strcmp(argv[1], "loadaedat") || !std::strcmp(argv[1], "loadbin")) {
            opengv2::EventContainer c;
            if (!std::strcmp(argv[1], "loadaedat")) c.loadAedatFile(argv[2], &opt);
            else c.loadFile(argv[2], -std::numeric_limits<double>::infinity());
            std::printf("size %zu first %.17g last %.17g packets %llu records %llu\n", c.size(), c.firstTime(), c.lastTime(),
                        (unsigned long long) c.aedatInfo.n_packets, (unsigned long long) c.aedatInfo.n_records);
            return 0;
        }
        ecal_aedat_info info;
        const long long n = std::strcmp(argv[1], "host") ? opengv2::EventStream::aedat2binDevice(argv[2], &opt, &info)
                                                         : opengv2::EventStream::aedat2bin(argv[2], &opt, &info);
        std::printf("count %lld raw %llu invalid %llu outside %llu negative %llu packets %llu other_packets %llu records %llu other_records %llu "
                    "trailing %llu wraps %llu format %d header %llu\n", n, (unsigned long long) info.n_raw_events,
                    (unsigned long long) info.n_invalid, (unsigned long long) info.n_outside, (unsigned long long) info.n_negative,
                    (unsigned long long) info.n_packets, (unsigned long long) info.n_other_packets, (unsigned long long) info.n_records,
                    (unsigned long long) info.n_other_records, (unsigned long long) info.n_trailing_bytes,
                    (unsigned long long) info.n_time_wraps, info.format, (unsigned long long) info.header_bytes);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("aedat_driver")
    src, exe = str(d / "drv.cpp"), str(d / "drv")
    open(src, "w").write(DRIVER_SRC)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", exe, src,
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    return exe


def run(driver, mode, path, width=0, height=0, time_base=0, ok=True):
    out = subprocess.run([driver, mode, path, str(width), str(height), str(time_base)], capture_output=True, text=True, timeout=120)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out.stdout


def random_file(fmt, n, seed):
    """a file of n random events — a tenth outside 346 x 260, a tenth invalid (3.1), foreign packets / records in between"""
    rng = np.random.default_rng(seed)
    x, y, p = rng.integers(0, 380, n), rng.integers(0, 290, n), rng.integers(0, 2, n)
    ts = 5000 + np.cumsum(rng.integers(0, 20, n))
    if fmt == "3.1":
        valid = rng.integers(0, 10, n) > 0
        parts, a = [], 0
        while a < n:
            b = min(n, a + int(rng.integers(0, 3000)))
            parts.append(polarity([ev(int(x[k]), int(y[k]), int(p[k]), int(ts[k]), int(valid[k])) for k in range(a, b)], overflow=a // 40000))
            parts.append(foreign(int(rng.integers(1, 60)), int(rng.integers(0, 5)), etype=int(rng.integers(2, 5))))
            a = b
        return HEADER31 + b"".join(parts) + b"\x01\x00\x01"
    addr = (y << 22) | (x << 12) | (p << 11) | rng.integers(0, 1024, n)
    kind = rng.integers(0, 10, n)
    addr = np.where(kind == 0, addr | 0x80000000, np.where(kind == 1, addr | 0x400, addr & ~0x400))
    return HEADER20 + np.stack([addr, (0xFFFF0000 + ts) & 0xFFFFFFFF], axis=1).astype(">u4").tobytes() + b"\x01"


@pytest.mark.parametrize("fmt", ["3.1", "2.0"])
def test_host_and_device_converters_write_identical_files(driver, tmp_path, fmt):
    data = random_file(fmt, 100000, 77)
    host, dev = str(tmp_path / "host.aedat"), str(tmp_path / "device.aedat")
    for path in (host, dev):
        open(path, "wb").write(data)
    late = 6000 if fmt == "3.1" else 0xFFFF0000 + 6000        # a time base behind the first events
    for size in ((0, 0, 0), (346, 260, late)):          # without bounds; with bounds, the flip of y and a time base
        a = run(driver, "host", host, *size)
        b = run(driver, "device", dev, *size)
        print(a)
        assert a == b and int(a.split()[1]) > 50000
        out = open(host[:-6] + ".bin", "rb").read()
        assert out == open(dev[:-6] + ".bin", "rb").read() and len(out) == 25 * int(a.split()[1])
    assert "outside 0 " not in a and "negative 0 " not in a and ("header %d" % len(HEADER31 if fmt == "3.1" else HEADER20)) in a
    assert ("invalid 0 " not in a and "other_packets 0 " not in a and "trailing 3 " in a) if fmt == "3.1" else ("wraps 1 " in a and "other_records 0 " not in a)
    # a file of version 4.0: both refuse, and name the version
    open(host, "wb").write(b"#!AER-DAT4.0\r\n" + data[14:])
    for mode in ("host", "device", "loadaedat"):
        said = run(driver, mode, host, ok=False)
        assert "exception" in said and "4.0" in said


def test_load_aedat_file_reports_what_loading_the_bin_reports(driver, tmp_path, synthetic):  # noqa: F811
    t_us, x, y, p, records, base = synthetic
    binf = str(tmp_path / "events.bin")
    open(binf, "wb").write(records)
    b = run(driver, "loadbin", binf).split()
    for fmt in ("3.1", "2.0"):
        path = str(tmp_path / ("events%s.aedat" % fmt[0]))
        payload, n_packets = encode31(t_us, x, y, p) if fmt == "3.1" else (encode20(t_us, x, y, p), 0)
        open(path, "wb").write((HEADER31 if fmt == "3.1" else HEADER20) + payload)
        a = run(driver, "loadaedat", path, time_base=base).split()
        assert a[:6] == b[:6] and a[1] == "200000" and a[7] == str(n_packets) and a[9] == ("0" if fmt == "3.1" else "200000")
        assert np.frombuffer(records[:8], "<f8")[0] == float(a[3]) and np.frombuffer(records[-25:-17], "<f8")[0] == float(a[5])


def test_driver_in_batch_mode_reads_an_aedat_file(tmp_path):
    """unit_test_eventCameraCalib <settings> <events> <dir> batch on events.aedat (3.1, frames between the event packets; the file's
    clock starts at Aedat_TimeBase) and on the .bin of the same events.  The records in HBM are the same bytes, so the keyframe and
    init lines are the same text; the refined line is held to test_gpu_shims.py's figure for two runs of the chain (the solve sums
    with FP64 atomics)."""
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
    base = 123456789
    binf, aedat = str(tmp_path / "events.bin"), str(tmp_path / "events.aedat")
    SS.pack_records(t_us.to(torch.float64) * 1e-6, xy, pol).numpy().tofile(binf)
    between = lambda k: foreign(36 + 346 * 260 * 2, 1) if k % 8 == 0 else foreign(51, 2, etype=3) if k % 2 else b""
    payload, _ = encode31(t_us.numpy() + base, xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(), pol.to(torch.int64).numpy(),
                          between=between)
    open(aedat, "wb").write(HEADER31 + payload)
    outs = {}
    for name, path, extra in (("bin", binf, ""), ("aedat", aedat, "Aedat_TimeBase: %d\n" % base)):
        d = tmp_path / name
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(SETTINGS_YAML % dict(start=5, end=8) + extra)
        out = subprocess.run([exe, yamlf, path, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = [ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")]
    a, b = outs["aedat"], outs["bin"]
    print("\n".join(a))
    assert [ln.split()[0] for ln in a] == ["keyframes", "init", "refined"] == [ln.split()[0] for ln in b]
    assert a[0] == b[0] and a[1] == b[1] and int(a[0].split()[1]) > 20
    ra, rb = a[2].split(), b[2].split()
    assert np.abs(np.array([float(v) for v in ra[1:10]]) - np.array([float(v) for v in rb[1:10]])).max() < 1e-9 * 400 and ra[10:] == rb[10:]
    # AEDAT 4 is refused by its name, before anything is read
    aedat4 = str(tmp_path / "events.aedat4")
    open(aedat4, "wb").write(b"#!AER-DAT4.0\r\n")
    out = subprocess.run([exe, str(tmp_path / "bin" / "settings.yaml"), aedat4, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "AEDAT 4" in out.stderr
    # ... and a file of that version under the name .aedat by its first line
    open(aedat, "wb").write(b"#!AER-DAT4.0\r\n" + payload[:1000])
    out = subprocess.run([exe, str(tmp_path / "aedat" / "settings.yaml"), aedat, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "4.0" in out.stderr
