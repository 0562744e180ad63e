"""GPU: the C++ shims of the array ingest (eventcalib_amd/csrc/host/event.hpp) through a small driver compiled into the temporary
directory: EventStream::npy2bin (one host thread, the plain walk of fields_events.hpp) and EventStream::npy2binDevice
(ecal_npy_to_bin_file) must write identical files; EventContainer::loadNpyFile and ::loadArrays must report the size and the first /
last time that loading that .bin reports; a big-endian file raises.  And the product's driver in `batch` mode on the .npy of the
synthetic calibration stream the other driver tests use, against the same run on the .bin that EventStream::npy2bin makes of it."""
import os
import subprocess

import numpy as np
import pytest

import synth_stream as SS
from test_gpu_shims import SETTINGS_YAML

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED = np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")])

DRIVER_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "event.hpp"
// usage: drv host|device|loadnpy|loadarrays|loadbin file width height time_base
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    ecal_npy_options opt;
    ecal_npy_default_options(&opt);
    opt.fields.width = (uint32_t) std::atoi(argv[3]);
    opt.fields.height = (uint32_t) std::atoi(argv[4]);
    opt.fields.time_base = std::atoll(argv[5]);
    opt.fields.flip_y = opt.fields.height ? 1 : 0;
    try {
        if (!std::strncmp(argv[1], "load", 4)) {
            opengv2::EventContainer c;
            if (!std::strcmp(argv[1], "loadnpy")) {
                c.loadNpyFile(argv[2], &opt);
            } else if (!std::strcmp(argv[1], "loadarrays")) {   // the packed 13-byte items of the file, as columns in host memory
                std::FILE *fp = std::fopen(argv[2], "rb");
                if (!fp) return 5;
                std::vector<uint8_t> bytes;
                uint8_t buf[65536];
                for (size_t got; (got = std::fread(buf, 1, sizeof(buf), fp)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
                std::fclose(fp);
                ecal_npy_layout L;
                char err[256] = "";
                if (ecal_npy_parse_header(nullptr, bytes.data(), bytes.size(), 0, &opt, &L, err, sizeof(err)) != ECAL_OK) throw std::invalid_argument(err);
                ecal_field f[4];
                for (int k = 0; k < 4; k++) f[k] = ecal_field{bytes.data() + L.data_offset + L.field[k].offset, (int64_t) L.item_stride, L.field[k].type, 0u};
                c.loadArrays(f, L.n_events, &opt.fields);
            } else {
                c.loadFile(argv[2], -std::numeric_limits<double>::infinity());
            }
            std::printf("size %zu first %.17g last %.17g base %lld\n", c.size(), c.firstTime(), c.lastTime(), (long long) c.fieldsInfo.time_base);
            return 0;
        }
        ecal_fields_info info;
        const long long n = std::strcmp(argv[1], "host") ? opengv2::EventStream::npy2binDevice(argv[2], &opt, &info)
                                                         : opengv2::EventStream::npy2bin(argv[2], &opt, &info);
        std::printf("count %lld raw %llu outside %llu negative %llu before %llu after %llu base %lld\n", n, (unsigned long long) info.n_raw_events,
                    (unsigned long long) info.n_outside, (unsigned long long) info.n_negative, (unsigned long long) info.n_before_start,
                    (unsigned long long) info.n_after_end, (long long) info.time_base);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("npy_driver")
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


def test_host_and_device_converters_write_identical_files(driver, tmp_path):
    import fields_oracle as FO
    rng = np.random.default_rng(77)
    n = 100000
    arr = np.zeros(n, PACKED)
    arr["t"] = 400000 + np.cumsum(rng.integers(0, 20, n))
    arr["x"], arr["y"], arr["p"] = rng.integers(0, 380, n), rng.integers(0, 290, n), rng.integers(0, 2, n)       # a tenth outside 346 x 260
    host, dev = str(tmp_path / "host.npy"), str(tmp_path / "device.npy")
    for path in (host, dev):
        np.save(path, arr)
    for size in ((0, 0, 0), (346, 260, 500000)):          # without bounds; with bounds, the flip of y and a time base behind the first events
        a = run(driver, "host", host, *size)
        b = run(driver, "device", dev, *size)
        print(a)
        assert a == b and int(a.split()[1]) > 50000
        out = open(host[:-4] + ".bin", "rb").read()
        assert out == open(dev[:-4] + ".bin", "rb").read() and len(out) == 25 * int(a.split()[1])
        want, counts = FO.from_fields(arr["t"], arr["x"], arr["y"], arr["p"], time_base=size[2], width=size[0], height=size[1], flip_y=bool(size[1]))
        assert out == want.tobytes() and ("outside %d negative %d " % (counts["n_outside"], counts["n_negative"])) in a
    assert " outside 0 " not in a and " negative 0 " not in a and ("base 500000") in a
    # a big-endian file: both refuse and say so
    np.save(host, arr.astype(PACKED.newbyteorder(">")))
    for mode in ("host", "device", "loadnpy", "loadarrays"):
        said = run(driver, mode, host, ok=False)
        assert "exception" in said and "big-endian" in said


def test_load_npy_file_and_load_arrays_report_what_loading_the_bin_reports(driver, tmp_path):
    n = 200000
    import torch
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cpu", seed=3))
    arr = np.zeros(n, PACKED)
    arr["t"] = torch.round(t * 1e6).to(torch.int64).numpy() + 1_600_000_000_000_000
    arr["x"], arr["y"], arr["p"] = xy[:, 0].numpy(), xy[:, 1].numpy(), pol.numpy()
    base = int(arr["t"][0]) // 10 ** 6 * 10 ** 6
    npy = str(tmp_path / "events.npy")
    np.save(npy, arr)
    assert run(driver, "host", npy, time_base=base).split()[1] == str(n)
    b = run(driver, "loadbin", str(tmp_path / "events.bin")).split()
    for mode in ("loadnpy", "loadarrays"):
        a = run(driver, mode, npy, time_base=base).split()
        assert a[:6] == b[:6] and a[1] == str(n) and a[7] == str(base), mode


def test_driver_in_batch_mode_reads_an_npy_file(driver, tmp_path):
    """unit_test_eventCameraCalib <settings> <events> <dir> batch on events.npy (packed 13-byte items, microsecond stamps of epoch time,
    Npy_TimeBase given) and on the .bin that EventStream::npy2bin — the plain host walk — makes of the same file.  The records in HBM
    are the same bytes: every line the driver prints and every file it writes must be identical (the settings files lie outside
    the output directories).  Each figure is printed before it is asserted."""
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
    base = 1_600_000_000_123_456
    arr = np.zeros(n, PACKED)
    arr["t"] = torch.round(t * 1e6).to(torch.int64).numpy() + base
    arr["x"], arr["y"], arr["p"] = xy[:, 0].numpy(), xy[:, 1].numpy(), pol.numpy()
    npy = str(tmp_path / "events.npy")
    np.save(npy, arr)
    said = run(driver, "host", npy, 346, 0, base)        # the oracle: events.bin beside the file, by the host walk (no flip)
    assert said.split()[1] == str(n) and ("base %d" % base) in said
    binf = str(tmp_path / "events.bin")
    outs, dirs = {}, {}
    for name, path, extra in (("bin", binf, ""), ("npy", npy, "Npy_TimeBase: %d\nNpy_TimeMagnitude: 1e-6\n" % base)):
        d = tmp_path / name
        d.mkdir()
        yamlf = str(tmp_path / (name + "_settings.yaml"))
        open(yamlf, "w").write(SETTINGS_YAML % dict(start=5, end=8) + extra)
        out = subprocess.run([exe, yamlf, path, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = [ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")]
        dirs[name] = d
    a, b = outs["npy"], outs["bin"]
    print("\n".join(a))
    assert [ln.split()[0] for ln in a] == ["keyframes", "init", "refined"] == [ln.split()[0] for ln in b]
    assert a[0] == b[0] and a[1] == b[1] and int(a[0].split()[1]) > 20
    ra, rb = a[2].split(), b[2].split()
    print("refined, largest difference of the nine figures:", np.abs(np.array([float(v) for v in ra[1:10]]) - np.array([float(v) for v in rb[1:10]])).max())
    files = lambda d: sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)
    differing = []
    for name in files(dirs["npy"]):
        same = os.path.exists(str(dirs["bin"] / name)) and open(str(dirs["npy"] / name), "rb").read() == open(str(dirs["bin"] / name), "rb").read()
        print("output file %s: %s" % (name, "identical" if same else "differs"))
        differing += [] if same else [name]
    assert a[2] == b[2]
    assert files(dirs["npy"]) == files(dirs["bin"]) and "TrajectoryByEvent.txt" in files(dirs["npy"])
    assert not differing, differing
    assert len(open(str(dirs["npy"] / "TrajectoryByEvent.txt")).read().split("\n")) > 20
    # a file the header parser refuses ends the driver with the library's text and exit code 4
    np.save(npy, np.zeros(10, [("t", "<i8"), ("x", "<u2"), ("p", "u1")]))
    out = subprocess.run([exe, str(tmp_path / "npy_settings.yaml"), npy, str(tmp_path), "batch"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 4 and "missing field y" in out.stderr
