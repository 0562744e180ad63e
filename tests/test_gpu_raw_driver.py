"""GPU: the C++ shims of the raw ingest (eventcalib_amd/csrc/host/event.hpp) through a small driver compiled into the temporary
directory: EventStream::raw2bin (one host thread, the sequential decoder of raw_events.hpp) and EventStream::raw2binDevice
(ecal_raw_to_bin_file) must write identical files; EventContainer::loadRawFile must report the size and the first / last time that
loading that .bin reports."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_raw_ingest import encode, payload_of, random_words, synthetic  # noqa: F401  (synthetic: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "event.hpp"
// usage: drv host|device|loadraw|loadbin file width height
int main(int argc, char **argv) {
    if (argc != 5) return 2;
    ecal_raw_options opt;
    ecal_raw_default_options(&opt);
    opt.width = (uint32_t) std::atoi(argv[3]);
    opt.height = (uint32_t) std::atoi(argv[4]);
    try {
        if (!std::strcmp(argv[1], "loadraw") || !std::strcmp(argv[1], "loadbin")) {
            opengv2::EventContainer c;
            if (!std::strcmp(argv[1], "loadraw")) c.loadRawFile(argv[2], &opt);
            else c.loadFile(argv[2], -std::numeric_limits<double>::infinity());
            std::printf("size %zu first %.17g last %.17g words %llu\n", c.size(), c.firstTime(), c.lastTime(),
                        (unsigned long long) c.rawInfo.n_words);
            return 0;
        }
        ecal_raw_info info;
        const long long n = std::strcmp(argv[1], "host") ? opengv2::EventStream::raw2binDevice(argv[2], &opt, &info)
                                                         : opengv2::EventStream::raw2bin(argv[2], &opt, &info);
        std::printf("count %lld words %llu no_state %llu outside %llu other %llu wraps %llu format %d header %llu\n", n,
                    (unsigned long long) info.n_words, (unsigned long long) info.n_no_state, (unsigned long long) info.n_outside,
                    (unsigned long long) info.n_other_words, (unsigned long long) info.n_time_wraps, info.format,
                    (unsigned long long) info.header_bytes);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("raw_driver")
    src, exe = str(d / "drv.cpp"), str(d / "drv")
    open(src, "w").write(DRIVER_SRC)
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(lib_dir, "csrc", "host"), "-o", exe, src,
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    return exe


def run(driver, mode, path, width=0, height=0, ok=True):
    out = subprocess.run([driver, mode, path, str(width), str(height)], capture_output=True, text=True, timeout=120)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out.stdout


@pytest.mark.parametrize("fmt,header", [("EVT3", b"% evt 3.0\n% end\n"), ("EVT2", b"% format EVT2;width=1280\n")])
def test_host_and_device_converters_write_identical_files(driver, tmp_path, fmt, header):
    payload = payload_of(random_words(fmt, 100000, 77), fmt, b"\x01")
    host_raw, dev_raw = str(tmp_path / "host.raw"), str(tmp_path / "device.raw")
    for path in (host_raw, dev_raw):
        open(path, "wb").write(header + payload)
    for size in ((0, 0), (640, 480)):
        a = run(driver, "host", host_raw, *size)
        b = run(driver, "device", dev_raw, *size)
        print(a)
        assert a == b and int(a.split()[1]) > 5000
        data = open(host_raw[:-4] + ".bin", "rb").read()
        assert data == open(dev_raw[:-4] + ".bin", "rb").read() and len(data) == 25 * int(a.split()[1])
    assert "outside 0" not in a and ("header %d" % len(header)) in a
    # no format anywhere: both refuse
    open(host_raw, "wb").write(payload)
    assert "exception" in run(driver, "host", host_raw, ok=False) and "exception" in run(driver, "device", host_raw, ok=False)


def test_load_raw_file_reports_what_loading_the_bin_reports(driver, tmp_path, synthetic):  # noqa: F811
    t_us, x, y, p, records = synthetic
    raw, binf = str(tmp_path / "events.raw"), str(tmp_path / "events.bin")
    payload = encode("EVT3", t_us, x, y, p)
    open(raw, "wb").write(b"% evt 3.0\n% end\n" + payload)
    open(binf, "wb").write(records)
    a, b = run(driver, "loadraw", raw).split(), run(driver, "loadbin", binf).split()
    assert a[:6] == b[:6] and a[1] == "200000" and a[7] == str(len(payload) // 2)
    assert np.frombuffer(records[:8], "<f8")[0] == float(a[3]) and np.frombuffer(records[-25:-17], "<f8")[0] == float(a[5])
