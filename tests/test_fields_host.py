"""CPU: the array ingest's walk (ecal_events_from_fields_host — eventcalib_amd/csrc/fields_events.hpp compiled into the library, no
device) and its reverse (ecal_events_to_fields_host) against the numpy statement of the rule (tests/fields_oracle.py), byte for byte:
every allowed type for every field, the three polarity conventions, packed items of 13, 14 and 16 bytes, each drop class and the stop
rule with the counter identity, the refusals by their text, and the round trip of integer stamps.  tests/cpp/check_fields.cpp runs the
same header stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer.  And the C ABI's new names: declared, listed, mirrored."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fields_oracle as FO  # noqa: E402

NEW_INT_SYMBOLS = ("ecal_events_from_fields_host", "ecal_events_from_fields_dev", "ecal_stream_create_from_fields", "ecal_events_to_fields_host",
                   "ecal_events_to_fields_dev", "ecal_npy_parse_header", "ecal_stream_create_from_npy_file", "ecal_npy_to_bin_file",
                   "ecal_stream_to_npy_file")


@pytest.fixture(scope="module")
def capi():
    import eventcalib_amd
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    from eventcalib_amd import capi
    return capi


def _check(capi, cols, **options):
    """the host walk against the oracle on the same columns and options; -> the info dict"""
    got, info = capi.events_from_fields_host(*cols, **options)
    want_opt = dict(options)
    want_opt.setdefault("time_magnitude", FO.default_magnitude(cols[0]))
    want, counts = FO.from_fields(*cols, **want_opt)
    assert {k: info[k] for k in FO.COUNTERS} == counts
    assert got.tobytes() == want.tobytes()
    assert sum(info[k] for k in FO.COUNTERS[1:]) == info["n_raw_events"]
    return info


CASES = [("t", dt) for dt in FO.STAMP_DTYPES] + [(f, dt) for f in "xyp" for dt in FO.ALL_DTYPES + (np.bool_,)]


@pytest.mark.parametrize("field,dtype", CASES, ids=["%s-%s" % (f, np.dtype(d).name) for f, d in CASES])
def test_every_allowed_type_of_every_field(capi, field, dtype):
    rng = np.random.default_rng(11)
    cols = FO.random_columns(rng, 777, **{field: dtype})
    info = _check(capi, cols)
    assert info["n_events"] == 777
    # with a size, a start and an end: the same
    _check(capi, cols, width=200, height=200, start_time=1.5, end_time=4.2, flip_x=True, flip_y=True)


def test_the_three_polarity_conventions_and_nan(capi):
    rng = np.random.default_rng(5)
    t, x, y, _ = FO.random_columns(rng, 300)
    bits = rng.integers(0, 2, 300)
    want = None
    for p in (bits.astype(np.uint8), bits.astype(bool), (2 * bits - 1).astype(np.int8), (2 * bits - 1).astype(np.float32), bits.astype(np.float64)):
        got, _ = capi.events_from_fields_host(t, x, y, p)
        _check(capi, (t, x, y, p))
        assert FO.records(got)["p"].tolist() == bits.tolist()
        want = got if want is None else want
        assert got.tobytes() == want.tobytes()
    p = np.where(bits == 1, np.nan, 1.0)
    got, _ = capi.events_from_fields_host(t, x, y, p)
    assert FO.records(got)["p"].tolist() == (1 - bits).tolist()      # NaN gives 0


ITEMS = {
    13: np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")]),
    14: np.dtype([("ts", "<i8"), ("X", "<u2"), ("Y", "<u2"), ("pol", "<i2")]),
    16: np.dtype([("timestamp", "<i8"), ("x", "<u2"), ("y", "<u2"), ("polarity", "?")], align=True),
}


@pytest.mark.parametrize("item", sorted(ITEMS))
def test_packed_items_of_13_14_and_16_bytes(capi, item):
    dt = ITEMS[item]
    assert dt.itemsize == item
    rng = np.random.default_rng(item)
    t, x, y, p = FO.random_columns(rng, 501)
    arr = np.zeros(501, dt)
    names = dt.names
    for name, col in zip(names, (t, x, y, p)):
        arr[name] = col
    cols = tuple(arr[name] for name in names)
    assert all(c.strides[0] == item for c in cols)          # taken where they lie
    for shift in range(4):                                   # ... at every byte offset of the item array
        raw = np.zeros(arr.nbytes + 8, np.uint8)
        raw[shift: shift + arr.nbytes] = arr.view(np.uint8)
        moved = raw[shift: shift + arr.nbytes].view(dt)
        info = _check(capi, tuple(moved[name] for name in names), width=346, height=260, end_time=4.0)
        assert info["n_after_end"] > 0 and info["n_events"] > 0


def _filter_case():
    rng = np.random.default_rng(23)
    n = 4000
    t, x, y, p = FO.random_columns(rng, n, t=np.int64, x=np.int16, y=np.float32)
    x[::17] = -1
    y[5::29] = np.nan
    y[7::31] = 260.0
    return (t, x, y, p), dict(width=346, height=260, time_base=1_300_000, start_time=0.4, end_time=2.9)


def test_each_drop_class_the_stop_rule_and_the_counter_identity(capi):
    cols, opt = _filter_case()
    info = _check(capi, cols, **opt)
    assert all(info[k] > 0 for k in FO.COUNTERS), info                 # a condition on the input
    assert 2 * info["n_events"] >= info["n_raw_events"], info
    assert info["time_base"] == 1_300_000
    # the stop event is the first that reaches end_time in INPUT order: an early late event ends the stream there
    t = cols[0].copy()
    t[101] = t[-1]                                            # (event 101 is inside the sensor)
    info = _check(capi, (t,) + cols[1:], **opt)
    assert info["n_after_end"] == len(t) - 101
    # flips behind the bounds test, a float stamp in seconds, sub-pixel coordinates kept
    ts = cols[0].astype(np.float64) * 1e-6
    _check(capi, (ts,) + cols[1:], width=346, height=260, flip_x=True, flip_y=True, start_time=1.2, end_time=3.9)
    got, _ = capi.events_from_fields_host(ts, cols[1], cols[2], cols[3], time_magnitude=1.0)
    keep = np.ones(len(ts), bool)
    assert FO.records(got)["t"].tobytes() == ts[keep].tobytes()         # an F64 stamp passes bit for bit
    # the automatic base: element 0's stamp
    got, info = capi.events_from_fields_host(*cols, auto_time_base=True)
    assert info["time_base"] == int(cols[0][0]) and FO.records(got)["t"][0] == 0.0
    want, _ = FO.from_fields(*cols, time_base=int(cols[0][0]))
    assert got.tobytes() == want.tobytes()
    assert capi.events_from_fields_host(ts, cols[1], cols[2], cols[3], auto_time_base=True)[1]["time_base"] == 0
    # no events
    e = np.zeros(0, np.int64)
    got, info = capi.events_from_fields_host(e, e, e, e)
    assert got.size == 0 and all(info[k] == 0 for k in FO.COUNTERS)


def test_a_capacity_too_small_reports_the_count_needed(capi):
    cols = FO.random_columns(np.random.default_rng(2), 100)
    with pytest.raises(capi.EcalError) as e:
        capi.events_from_fields_host(*cols, capacity=40)
    assert e.value.status == -6 and e.value.info["n_events"] == 100


def test_refusals_name_the_field(capi):
    t, x, y, p = FO.random_columns(np.random.default_rng(3), 50)
    for bad_t in (t.astype(np.uint8), t.astype(np.int16), t.astype(np.uint16), t.astype(np.int8)):
        with pytest.raises(capi.EcalError) as e:
            capi.events_from_fields_host(bad_t, x, y, p)
        assert e.value.status == -1 and "field t" in str(e.value) and "stamp type" in str(e.value)
    with pytest.raises(capi.EcalError) as e:
        capi.events_from_fields_host(t.astype(np.float64), x, y, p, time_base=5)
    assert e.value.status == -1 and "float stamp" in str(e.value)
    for flips in (dict(flip_x=True, height=260), dict(flip_y=True, width=346)):
        with pytest.raises(capi.EcalError) as e:
            capi.events_from_fields_host(t, x, y, p, **flips)
        assert e.value.status == -1 and "flip_x / flip_y need width / height" in str(e.value)
    # raw: a type code that does not exist, a stride below the type's size
    L = capi.load_library()
    f = (capi.Field * 4)(*[capi._host_column(a)[1] for a in (t, x, y, p)])
    o, info, err = capi.fields_options(), capi.FieldsInfo(), ctypes.create_string_buffer(256)
    out = np.zeros(50 * 25, np.uint8)
    f[2].type = 9
    assert L.ecal_events_from_fields_host(f, 50, ctypes.byref(o), out.ctypes.data, 50, ctypes.byref(info), err, 256) == -1
    assert b"field y" in err.value and b"unknown type" in err.value
    f[2].type, f[1].stride = 2, 1
    assert L.ecal_events_from_fields_host(f, 50, ctypes.byref(o), out.ctypes.data, 50, ctypes.byref(info), err, 256) == -1
    assert b"field x" in err.value and b"stride" in err.value
    with pytest.raises(ValueError):
        capi.events_from_fields_host(np.full(3, 2 ** 63, np.uint64), x[:3], y[:3], p[:3])
    got, _ = capi.events_from_fields_host(np.arange(3, dtype=np.uint64), x[:3], y[:3], p[:3])       # viewed as int64
    assert FO.records(got)["t"].tolist() == [0.0, 1e-6, 2e-6]


OUT_CASES = [(np.float64, np.float64, np.uint8), (np.float32, np.float32, np.float32), (np.int64, np.uint16, np.bool_), (np.uint32, np.int16, np.int8),
             (np.int32, np.uint8, np.uint16), (np.int64, np.int8, np.int64), (np.int64, np.uint32, np.float64), (np.int64, np.int32, np.int32),
             (np.int64, np.int64, np.uint32)]


@pytest.mark.parametrize("t,xy,p", OUT_CASES, ids=["-".join(np.dtype(d).name for d in c) for c in OUT_CASES])
def test_the_reverse_equals_the_oracle_for_each_output_type(capi, t, xy, p):
    rng = np.random.default_rng(31)
    cols = FO.random_columns(rng, 600, width=100, height=100)
    events, _ = FO.from_fields(*cols)
    signed = np.dtype(p).kind in "if"
    got, info = capi.events_to_fields_host(events, t=t, xy=xy, p=p, polarity_signed=signed)
    want, bad = FO.to_fields(events, t=t, xy=xy, p=p, polarity_signed=signed)
    assert not bad.any() and info == {"n_events": 600, "n_unrepresentable": 0}
    for k in "txyp":
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    # with a base and another tick
    if np.dtype(t).kind != "f":
        got, _ = capi.events_to_fields_host(events, t=t, xy=xy, p=p, polarity_signed=signed, ticks_per_second=1e3, time_base=77)
        want, _ = FO.to_fields(events, t=t, xy=xy, p=p, polarity_signed=signed, ticks_per_second=1e3, time_base=77)
        assert got["t"].tobytes() == want["t"].tobytes()


def test_what_is_not_representable_is_counted(capi):
    rng = np.random.default_rng(41)
    t, x, y, p = FO.random_columns(rng, 500, x=np.float64, y=np.float64)
    x[::7] = np.floor(x[::7])
    y[:] = np.floor(y)
    t = t.astype(np.float64) * 1e-6
    t[3], t[9], t[11] = np.nan, np.inf, 1e300
    events, _ = FO.from_fields(t, x, y, p, time_magnitude=1.0)
    rec = FO.records(events).copy()
    rec["t"][3] = np.nan                                    # (the ingest drops a NaN stamp: put one into the records)
    rec["x"][20], rec["y"][21], rec["y"][22] = 70000.0, -1.0, np.inf
    events = rec.view(np.uint8).reshape(-1)
    want, bad = FO.to_fields(events, t=np.int64, xy=np.uint16)
    assert 0 < bad.sum() < rec.size
    with pytest.raises(capi.EcalError) as e:
        capi.events_to_fields_host(events, t=np.int64, xy=np.uint16)
    assert e.value.status == -6 and e.value.info["n_unrepresentable"] == int(bad.sum())
    with pytest.raises(capi.EcalError) as e:
        capi.events_to_fields_host(events, p=np.uint8, polarity_signed=True)
    assert e.value.status == -1 and "field p" in str(e.value)
    # float outputs hold everything
    got, info = capi.events_to_fields_host(events, t=np.float32, xy=np.float32)
    assert info["n_unrepresentable"] == 0
    want, _ = FO.to_fields(events, t=np.float32, xy=np.float32)
    assert all(got[k].tobytes() == want[k].tobytes() for k in "txyp")


def test_integer_stamps_come_back_exactly(capi):
    """for stamp - base < 2 * 10^15 ticks at 1e-6 / 1e6: to_fields(from_fields(k)) == k"""
    rng = np.random.default_rng(53)
    n = 200_000
    base = 1_600_000_000_000_000
    k = base + rng.integers(0, 2 * 10 ** 15, n)
    k[:4] = base, base + 1, base + 2 * 10 ** 15 - 1, base + 10 ** 15
    _, x, y, p = FO.random_columns(rng, n)
    events, info = capi.events_from_fields_host(k, x, y, p, time_base=base)
    assert info["n_events"] == n
    back, _ = capi.events_to_fields_host(events, t=np.int64, xy=np.uint16, p=np.uint8, time_base=base)
    assert (back["t"] == k).all() and (back["x"] == x).all() and (back["y"] == y).all() and (back["p"] == p).all()


# ---- the stand-alone program under the sanitizers -------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "check_fields.cpp")
INC = os.path.join(ROOT, "eventcalib_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC]


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_header_parser_and_walk_stand_alone(tmp_path, name, extra):
    exe = str(tmp_path / ("check_fields_" + name))
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "walk: 400 inputs equal" in out.stdout
    assert "headers: 0 wrong" in out.stdout


# ---- the ABI's new names --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    capi_src = open(os.path.join(ROOT, "eventcalib_amd", "capi.py")).read()
    listed = re.search(r"EXPORTED_SYMBOLS = \[(.*?)\n\]", capi_src, re.S).group(1)
    for name in NEW_INT_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert '"%s"' % name in listed, name
    for name in ("ecal_fields_default_options", "ecal_to_fields_default_options", "ecal_npy_default_options"):
        assert re.search(r"^void %s\(" % name, header, re.M) and '"%s"' % name in listed
    assert re.search(r"^uint32_t ecal_fields_block_events\(", header, re.M) and '"ecal_fields_block_events"' in listed
    assert re.search(r"#define ECAL_ABI_VERSION 3\b", header)      # additive: the version stays


def test_the_ctypes_structures_follow_the_header(capi):
    header = open(os.path.join(ROOT, "include", "ecal.h")).read()
    for cname, cls in (("ecal_field", capi.Field), ("ecal_fields_options", capi.FieldsOptions), ("ecal_fields_info", capi.FieldsInfo),
                       ("ecal_to_fields_options", capi.ToFieldsOptions), ("ecal_to_fields_info", capi.ToFieldsInfo), ("ecal_npy_field", capi.NpyField),
                       ("ecal_npy_layout", capi.NpyLayout), ("ecal_npy_options", capi.NpyOptions)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names.append(re.sub(r"\[\d+\]", "", first.split()[-1].lstrip("*")))
                names.extend(r.strip() for r in rest)
        assert names == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(capi.Field) == 24 and ctypes.sizeof(capi.FieldsInfo) == 56 and ctypes.sizeof(capi.NpyLayout) == 24 + 4 * 16 + 8
    for code, name in enumerate(capi.FIELD_TYPE_NAMES):
        assert re.search(r"ECAL_FIELD_%s = %d\b" % (name, code), header), name
    o = capi.fields_options()
    assert (o.time_magnitude, o.time_base, o.auto_time_base, o.width, o.height, o.flip_x, o.flip_y, o.start_time, o.has_end_time) == (1e-6, 0, 0, 0, 0, 0, 0, 0.0, 0)
    assert capi.to_fields_options().ticks_per_second == 1e6
