"""CPU: the hot-pixel filter without a device.

eventcalib_amd/csrc/pixel_activity.hpp — the pixel of a record, the rule that calls a pixel hot, the sequential and the block-wise
compaction that the kernels of ecal_activity.hip and ecal_hot_pixel_mask share — compiled for the host: tests/cpp/check_hot_pixels.cpp
(the classification on its edge values; the rule against a brute-force restatement on seeded random count maps and the special ones;
the block-wise compaction with blocks of 1, 2, 7, 64 and 4096 events against the sequential one on 1000 seeded random streams), once
plainly and once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is preloaded).

ecal_hot_pixel_mask through ctypes (no context, no device) against the numpy oracle of tests/hot_pixel_oracle.py: with the default
options the project's clean synthetic streams mask no pixel, and with hot pixels injected exactly the injected pixels are masked.
And the C ABI's new names: declared in include/ecal.h, listed in capi.py, the ctypes structures as the header has them."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hot_pixel_oracle as HP  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "check_hot_pixels.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]   # (no FMA contraction, as the device translation unit)
NEW_INT_SYMBOLS = ("ecal_pixel_activity_dev", "ecal_hot_pixel_mask", "ecal_filter_events_dev", "ecal_stream_remove_hot_pixels")
W, H = 346, 260


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_header_on_the_host(tmp_path, name, extra):
    exe = str(tmp_path / ("check_hot_pixels_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pixels: 29 cases" in out.stdout
    assert "rule: 421 maps" in out.stdout
    assert "streams: 1000 streams equal" in out.stdout
    assert "wrong: 0" in out.stdout


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_INT_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    assert re.search(r"^void ecal_hot_pixel_default_options\(", header, re.M) and '"ecal_hot_pixel_default_options"' in listed
    for struct_name in ("ecal_activity_totals", "ecal_filter_totals", "ecal_hot_pixel_options", "ecal_hot_pixel_info"):
        assert "typedef struct %s" % struct_name in header, struct_name
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays
    assert "pixel activity / hot pixels" in header
    makefile = open(os.path.join(ROOT, "eventcalib_amd", "csrc", "Makefile")).read()
    assert "build/ecal_activity.o" in makefile


def _header_fields(header, cname):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names.append(first.split()[-1].lstrip("*"))
            names.extend(r.strip() for r in rest)
    return names


def test_the_ctypes_structures_follow_the_header():
    from eventcalib_amd import capi
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    for cname, cls in (("ecal_hot_pixel_options", capi.HotPixelOptions), ("ecal_hot_pixel_info", capi.HotPixelInfo)):
        assert _header_fields(header, cname) == [n for n, _ in cls._fields_], cname
    for cname, dtype in (("ecal_activity_totals", capi.ACTIVITY_TOTALS), ("ecal_filter_totals", capi.FILTER_TOTALS)):
        assert _header_fields(header, cname) == list(dtype.names), cname
        assert dtype.itemsize == 8 * len(dtype.names)
    assert ctypes.sizeof(capi.HotPixelOptions) == 24 and ctypes.sizeof(capi.HotPixelInfo) == 56


# ---- ecal_hot_pixel_mask (no device, no context) against the oracle ------------------------------------------------------------------
def _library():
    import eventcalib_amd
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(eventcalib_amd.lib_path())


def _same_mask(counts, extra_mask=None, **options):
    """capi.hot_pixel_mask against the oracle on one map; returns the mask and the info"""
    from eventcalib_amd import capi
    mask, info = capi.hot_pixel_mask(counts, extra_mask=extra_mask, **options)
    want, want_info = HP.hot_mask(counts, extra_mask=extra_mask, **options)
    assert mask.dtype == bool and mask.shape == counts.shape[1:]
    assert (mask == want).all()
    assert info == want_info
    return mask, info


def test_default_options_and_refusals():
    from eventcalib_amd import capi
    _library()
    o = capi.hot_pixel_options()
    assert (o.width, o.height, o.quantile_permille, o.min_count, o.factor) == (346, 260, 990, 64, 8.0)
    assert (HP.DEFAULTS["quantile_permille"], HP.DEFAULTS["min_count"], HP.DEFAULTS["factor"]) == (990, 64, 8.0)
    counts = np.zeros((2, 3, 5), np.uint32)
    for bad in (dict(quantile_permille=1001), dict(factor=-1.0), dict(factor=float("nan")), dict(factor=float("inf"))):
        with pytest.raises(capi.EcalError) as e:
            capi.hot_pixel_mask(counts, **bad)
        assert e.value.status == -1
    with pytest.raises(capi.EcalError):
        capi.hot_pixel_mask(np.zeros((2, 1, 4097), np.uint32))
    mask, info = _same_mask(counts)
    assert not mask.any() and info["n_active_pixels"] == 0 and info["quantile_count"] == 0


def test_rule_equals_the_oracle_on_random_maps():
    _library()
    rng = np.random.default_rng(5)
    for it in range(60):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 60))
        counts = (rng.integers(0, 30, (2, h, w)) * (rng.random((2, h, w)) < rng.random())).astype(np.uint32)
        for _ in range(int(rng.integers(0, 4))):
            counts[rng.integers(0, 2), rng.integers(0, h), rng.integers(0, w)] = rng.integers(0, 100000)
        extra = (rng.random((h, w)) < 0.1) if it % 2 else None
        _same_mask(counts, extra_mask=extra, quantile_permille=int(rng.choice([0, 500, 990, 1000, int(rng.integers(0, 1001))])),
                   min_count=int(rng.integers(0, 100)), factor=float(rng.choice([0.0, 1.0, 2.0, 8.0, 7.9])))
    # exact ties at factor * Q: 80 is not above 8 * 10
    counts = np.zeros((2, 4, 8), np.uint32)
    counts[0].ravel()[:28] = 10
    counts[0].ravel()[28:32] = (80, 40, 0, 81)
    counts[1].ravel()[28:32] = (0, 40, 80, 0)
    mask, info = _same_mask(counts, quantile_permille=500)
    assert info["quantile_count"] == 10 and info["n_hot_pixels"] == 1 and mask.ravel()[31] and mask.sum() == 1


@pytest.fixture(scope="module")
def clean_streams():
    import synth_stream as SS
    SS.TRAJECTORY = "orbit"
    try:
        orbit = SS.make_stream(2_000_000, rate=1.0e6, t_start=5.0, device="cpu", seed=21).numpy()
    finally:
        SS.TRAJECTORY = "hover"
    hover = SS.make_stream(60000, device="cpu", seed=3).numpy()
    return orbit, hover


def test_clean_streams_mask_no_pixel(clean_streams):
    """where the default factor comes from: the largest count is below 4 x the 99 % quantile of the non-zero counts on these streams
    (3.90 on the orbit stream, 1.76 on the hover stream), so a factor of 8 masks nothing"""
    _library()
    for name, rec, bound in (("orbit", clean_streams[0], 4.0), ("hover", clean_streams[1], 4.0)):
        counts, tot = HP.count_events(rec, W, H)
        assert tot["n_off_grid"] == 0 and tot["n_on_grid"] == rec.size // 25
        ratio = HP.ratio_max_to_quantile(counts)
        print("%s: %d events, largest count %d, ratio to the 99 %% quantile %.3f" % (name, rec.size // 25, int((counts[0] + counts[1]).max()), ratio))
        assert ratio < bound
        mask, info = _same_mask(counts)
        assert not mask.any() and info["n_hot_pixels"] == 0 and info["n_removed"] == 0 and info["n_kept"] == rec.size // 25


def test_injected_pixels_are_exactly_the_masked_ones(clean_streams):
    _library()
    clean = clean_streams[0]
    dirty, where, per = HP.inject_hot_pixels(clean, W, H)
    assert dirty.size == clean.size + 5 * 10000 * 25 and per == [(5000, 5000)] * 5
    t = HP.fields(dirty)[0]
    assert (np.diff(t) >= 0).all()
    counts, _ = HP.count_events(dirty, W, H)
    mask, info = _same_mask(counts)
    ys, xs = np.nonzero(mask)
    assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(where)
    assert info["n_hot_pixels"] == 5 == info["n_masked_pixels"] and info["n_removed"] == 50000 and info["max_count"] == 10000
    assert [(int(counts[0, y, x]), int(counts[1, y, x])) for x, y in where] == per
    # the oracle chain gives the clean stream back byte for byte
    out, chain_info = HP.remove_hot_pixels(dirty, W, H)
    assert out.tobytes() == clean.tobytes() and chain_info["n_removed"] == 50000 and chain_info["n_kept"] == clean.size // 25
