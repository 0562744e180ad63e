"""GPU: the array ingest (include/ecal.h "array ingest"; eventcalib_amd/csrc/ecal_fields.hip) — events held as four columns packed into
25-byte records in HBM — against the host walk (ecal_events_from_fields_host, itself held to the numpy oracle by
tests/test_fields_host.py), byte for byte, the counters included.  No tolerance anywhere.  B = ecal_fields_block_events() places the
cases on the kernels' block boundaries; columns are laid into larger tensors so that every base offset, stride and type meets the
aligned-word loads."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import eventcalib_amd
import fields_oracle as FO
from eventcalib_amd import calibrate, capi
from test_gpu_bag_ingest import load_bin, synthetic  # noqa: F401  (synthetic: a fixture)

pytestmark = pytest.mark.gpu

COMMON = dict(t=np.int64, x=np.uint16, y=np.uint16, p=np.uint8)
FILTER = dict(width=346, height=260, time_base=1_300_000, start_time=0.4, end_time=2.9, flip_x=True)
ITEMS = {
    13: np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")]),
    14: np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "<i2")]),
    16: np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "?")], align=True),
}


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def B(ctx):
    b = ctx.fields_block_events()
    assert b >= 64
    return b


def columns(n, seed=1, dirty=True, **types):
    """random columns; dirty: coordinates outside the sensor and NaNs where the type holds them, so that every counter moves"""
    rng = np.random.default_rng(seed)
    t, x, y, p = FO.random_columns(rng, n, **dict(COMMON, **types))
    if dirty and n:
        x[::17] = 400 if x.dtype.kind == "u" and x.dtype.itemsize > 1 else (255 if x.dtype == np.uint8 else -1)
        y[5::29] = np.nan if y.dtype.kind == "f" else 300 if y.dtype.itemsize > 1 else (255 if y.dtype == np.uint8 else -2)
    return t, x, y, p


def separate(cols, shift=0):
    """every column in a tensor of its own, `shift` bytes behind the tensor's (aligned) start -> (keep-alive, Field * 4)"""
    keep, f = [], (capi.Field * 4)()
    for k, c in enumerate(cols):
        raw = np.full(shift + c.nbytes + 5, 0xEE, np.uint8)
        raw[shift: shift + c.nbytes] = np.ascontiguousarray(c).view(np.uint8)
        d = torch.from_numpy(raw).cuda()
        assert d.data_ptr() % 16 == 0
        keep.append(d)
        f[k] = capi.Field(d.data_ptr() + shift, c.dtype.itemsize, capi.field_type(c.dtype), 0)
    return keep, f


def items(cols, dt, shift=0):
    """the columns as fields of one structured array, `shift` bytes behind a tensor's start -> (keep-alive, Field * 4, host array)"""
    arr = np.zeros(len(cols[0]), dt)
    for name, c in zip("txyp", cols):
        arr[name] = c
    raw = np.full(shift + arr.nbytes + 5, 0xEE, np.uint8)
    raw[shift: shift + arr.nbytes] = arr.view(np.uint8)
    d = torch.from_numpy(raw).cuda()
    f = (capi.Field * 4)()
    for k, name in enumerate("txyp"):
        f[k] = capi.Field(d.data_ptr() + shift + dt.fields[name][1], dt.itemsize, capi.field_type(dt[name]), 0)
    return [d], f, arr


def run_dev(ctx, f, n, capacity=None, **options):
    o = capi.fields_options(**options)
    cap = n if capacity is None else capacity
    out = torch.full((cap * 25 + 128,), 0xCD, dtype=torch.uint8, device="cuda")
    info = ctx.events_from_fields_dev(f, n, o, out.data_ptr() + 64, cap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:64] == 0xCD).all() and (h[64 + info["n_events"] * 25:] == 0xCD).all()      # nothing outside the records is stored
    return h[64: 64 + info["n_events"] * 25], info


def check(ctx, cols, f, **options):
    """the device form on the fields f against the host walk on the same columns"""
    options.setdefault("time_magnitude", FO.default_magnitude(cols[0]))
    want, want_info = capi.events_from_fields_host(*cols, **options)
    got, info = run_dev(ctx, f, len(cols[0]), **options)
    assert info == want_info
    assert got.tobytes() == want.tobytes()
    return info


def test_structures_have_the_library_sizes(ctx):
    """the default-option calls write the whole structure: a ctypes mirror that is too short would lose its guard bytes"""
    for cls, fn, size in ((capi.FieldsOptions, "ecal_fields_default_options", 64), (capi.ToFieldsOptions, "ecal_to_fields_default_options", 24),
                          (capi.NpyOptions, "ecal_npy_default_options", 64 + 40)):
        class Guarded(ctypes.Structure):
            _fields_ = [("o", cls), ("guard", ctypes.c_uint8 * 64)]
        g = Guarded()
        ctypes.memset(ctypes.byref(g), 0x5A, ctypes.sizeof(g))
        raw = ctypes.CDLL(capi.lib_path())      # (a handle of the test's own: the shared one keeps its struct-pointer prototypes)
        getattr(raw, fn).argtypes, getattr(raw, fn).restype = [ctypes.c_void_p], None
        getattr(raw, fn)(ctypes.byref(g))
        assert bytes(g.guard) == b"\x5A" * 64 and ctypes.sizeof(cls) == size, fn
    assert ctypes.sizeof(capi.Field) == 24 and ctypes.sizeof(capi.FieldsInfo) == 56


def test_sizes_around_the_block(ctx, B):
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 7):
        cols = columns(n, seed=n)
        keep, f = separate(cols)
        info = check(ctx, cols, f, **FILTER)
        assert info["n_raw_events"] == n
        check(ctx, cols, f)


CASES = [("t", dt) for dt in FO.STAMP_DTYPES] + [(f, dt) for f in "xyp" for dt in FO.ALL_DTYPES]


@pytest.mark.parametrize("field,dtype", CASES, ids=["%s-%s" % (f, np.dtype(d).name) for f, d in CASES])
def test_each_type_per_field(ctx, B, field, dtype):
    cols = columns(B + 5, seed=7, **{field: dtype})
    base = 0 if np.dtype(cols[0].dtype).kind == "f" else 1_300_000
    flt = dict(FILTER, time_base=base)
    for shift in (0, 1 + len(field + np.dtype(dtype).name) % 3):
        keep, f = separate(cols, shift)
        check(ctx, cols, f, **flt)


@pytest.mark.parametrize("item", sorted(ITEMS))
def test_base_offsets_and_strides(ctx, B, item):
    cols = columns(B + 3, seed=item)
    cols = cols[:3] + (cols[3].astype(ITEMS[item]["p"]),)
    for shift in (1, 2, 3):
        keep, f, arr = items(cols, ITEMS[item], shift)
        assert all(f[k].stride == item for k in range(4))
        check(ctx, tuple(arr[k] for k in "txyp"), f, **FILTER)
    # float columns of 4 and 8 bytes at every residue: one, two and three aligned words per element
    cols = columns(B + 3, seed=item, t=np.float64, x=np.float32, y=np.float64, p=np.float32)
    for shift in (1, 2, 3):
        keep, f = separate(cols, shift)
        check(ctx, cols, f, **dict(FILTER, time_base=0))


def test_the_stop_event_on_either_side_of_a_block_boundary(ctx, B):
    n = 2 * B + 50
    for stop in (B - 1, B, 2 * B - 1, 2 * B, 0, n - 1):
        t, x, y, p = columns(n, seed=3, dirty=False)
        t[:] = 1_000_000 + np.arange(n)
        t[stop] = 9_000_000
        if stop + 7 < n:
            t[stop + 7] = 9_500_000        # a later one that reaches it too
        keep, f = separate((t, x, y, p))
        info = check(ctx, (t, x, y, p), f, end_time=5.0)
        assert info["n_after_end"] == n - stop and info["n_events"] == stop


def test_every_counter_moves_and_half_the_events_stay(ctx, B):
    cols = columns(3 * B + 7, seed=23, x=np.int16, y=np.float32)
    keep, f = separate(cols, 1)
    info = check(ctx, cols, f, **FILTER)
    assert all(info[k] > 0 for k in FO.COUNTERS), info                     # a condition on the input
    assert 2 * info["n_events"] >= info["n_raw_events"], info
    assert sum(info[k] for k in FO.COUNTERS[1:]) == info["n_raw_events"]


def test_capacity_too_small_and_guard_bytes(ctx, B):
    cols = columns(B + 9, seed=5, dirty=False)
    keep, f = separate(cols)
    want, _ = capi.events_from_fields_host(*cols)
    for cap in (0, 1, B, B + 8):
        out = torch.full((cap * 25 + 128,), 0xCD, dtype=torch.uint8, device="cuda")
        with pytest.raises(capi.EcalError) as e:
            ctx.events_from_fields_dev(f, B + 9, capi.fields_options(), out.data_ptr() + 64, cap, 0)
        assert e.value.status == -6 and e.value.info["n_events"] == B + 9
        h = out.cpu().numpy()
        assert (h[:64] == 0xCD).all() and (h[64 + cap * 25:] == 0xCD).all()          # the 64 bytes in front and behind stay
    got, info = run_dev(ctx, f, B + 9, capacity=B + 9)
    assert got.tobytes() == want.tobytes()


def test_refusals_name_the_field(ctx, B):
    cols = columns(100, dirty=False)
    # the columns 8 KiB apart in one tensor: a record buffer laid over one column's end touches no other column
    big = torch.zeros(4 * 8192, dtype=torch.uint8, device="cuda")
    f = (capi.Field * 4)()
    for k, c in enumerate(cols):
        big[4096 + k * 8192: 4096 + k * 8192 + c.nbytes] = torch.from_numpy(c.view(np.uint8).copy()).cuda()
        f[k] = capi.Field(big.data_ptr() + 4096 + k * 8192, c.dtype.itemsize, capi.field_type(c.dtype), 0)
    out = torch.zeros(100 * 25 + 16, dtype=torch.uint8, device="cuda")

    def refused(fields, n, status, text, out_ptr=None, cap=100, **options):
        with pytest.raises(capi.EcalError) as e:
            ctx.events_from_fields_dev(fields, n, capi.fields_options(**options), out.data_ptr() if out_ptr is None else out_ptr, cap, 0)
        assert e.value.status == status and text in str(e.value), str(e.value)

    refused(f, 100, -1, "auto_time_base must be 0", auto_time_base=True)
    refused(f, 100, -1, "flip_x / flip_y need width / height", flip_y=True)
    g = (capi.Field * 4)(*f)
    g[0].type = capi.field_type(np.uint16)
    refused(g, 100, -1, "field t: type U16 is not a stamp type")
    g = (capi.Field * 4)(*f)
    g[3].type = 12
    refused(g, 100, -1, "field p: unknown type 12")
    g = (capi.Field * 4)(*f)
    g[1].stride = 1
    refused(g, 100, -1, "field x: stride 1")
    g = (capi.Field * 4)(*f)
    g[2].ptr = None
    refused(g, 100, -1, "field y: null pointer")
    _, fs = separate((cols[0].astype(np.float64),) + cols[1:])
    refused(fs, 100, -1, "float stamp", time_base=3)
    # an output that overlaps a column's bytes, at its first and at its last byte
    for k, name in enumerate("txyp"):
        span = 99 * f[k].stride + cols[k].dtype.itemsize
        refused(f, 100, -1, "overlaps field " + name, out_ptr=f[k].ptr + span - 1)
        refused(f, 100, -1, "overlaps field " + name, out_ptr=f[k].ptr - 100 * 25 + 1)
    refused(f, 2 ** 32, -6, "more than 2^32-1 events", cap=0)
    with pytest.raises(ValueError):
        ctx.events_from_arrays(cols[0][:5], cols[1], cols[2], cols[3])


def test_a_synthetic_stream_as_columns_equals_its_bin(ctx, tmp_path, synthetic):  # noqa: F811
    t_ns, x, y, p, records, base = synthetic
    binf = str(tmp_path / "events.bin")
    open(binf, "wb").write(records)
    want, w0, w1 = load_bin(ctx, binf)
    x16, y16, p8 = x.astype(np.uint16), y.astype(np.uint16), p.astype(np.uint8)
    opt = dict(time_magnitude=1e-9, time_base=base)
    ev, info = ctx.events_from_arrays(t_ns, x16, y16, p8, **opt)
    assert torch.equal(ev, want) and info["n_events"] == 200000 and info["time_base"] == base
    # torch tensors where they are: 1-D strided views of CUDA tensors, int16 coordinates, bool polarity
    tt = torch.stack([torch.from_numpy(t_ns).cuda(), torch.zeros(200000, dtype=torch.int64, device="cuda")], dim=1)
    xy = torch.stack([torch.from_numpy(x.astype(np.int16)).cuda(), torch.from_numpy(y.astype(np.int16)).cuda()], dim=1)
    ev, _ = ctx.events_from_arrays(tt[:, 0], xy[:, 0], xy[:, 1], torch.from_numpy(p8 != 0).cuda(), **opt)
    assert torch.equal(ev, want)
    # a structured array, uploaded once as it lies
    arr = np.zeros(200000, ITEMS[13])
    arr["t"], arr["x"], arr["y"], arr["p"] = t_ns, x16, y16, p8
    ev, _ = ctx.events_from_structured(arr, **opt)
    assert torch.equal(ev, want)
    # the stream form: HOST columns, and the structured array's fields taken where they lie
    for cols in ((t_ns, x16, y16, p8), tuple(arr[k] for k in "txyp")):
        ev, info, t0, t1 = ctx.stream_from_arrays(*cols, **opt)
        assert torch.equal(ev, want) and (t0, t1) == (w0, w1) and info["n_events"] == 200000
    ev, t0, t1 = calibrate.load_events_arrays(ctx, t_ns, x16, y16, p8, **opt)
    assert torch.equal(ev, want) and (t0, t1) == (w0, w1)
    _, info, _, _ = ctx.stream_from_arrays(t_ns, x16, y16, p8, time_magnitude=1e-9, auto_time_base=True)
    assert info["time_base"] == int(t_ns[0])
    # a shuffled copy: the device form keeps the input order, the stream form sorts (stable)
    idx = np.random.default_rng(4).permutation(200000)
    shuffled = np.frombuffer(records, FO.RECORD)[idx]
    ev, _ = ctx.events_from_arrays(t_ns[idx], x16[idx], y16[idx], p8[idx], **opt)
    assert ev.cpu().numpy().tobytes() == shuffled.tobytes()
    ev, _, _, _ = ctx.stream_from_arrays(t_ns[idx], x16[idx], y16[idx], p8[idx], **opt)
    assert ev.cpu().numpy().tobytes() == shuffled[np.argsort(shuffled["t"], kind="stable")].tobytes()
    # .npy files as numpy writes them: structured and (N, 4), and an .npz through numpy
    npy = str(tmp_path / "events.npy")
    np.save(npy, arr)
    ev, info, t0, t1 = ctx.stream_from_npy_file(npy, **opt)
    assert torch.equal(ev, want) and (t0, t1) == (w0, w1) and info["n_raw_events"] == 200000
    assert ctx.npy_to_bin(npy, str(tmp_path / "by_library.bin"), **opt) == info
    assert open(str(tmp_path / "by_library.bin"), "rb").read() == records
    ev, t0, t1 = calibrate.load_events_npy(ctx, npy, **opt)
    assert torch.equal(ev, want)
    np.save(npy, np.stack([x, y, t_ns, p], axis=1).astype(np.int64))
    ev, _, _, _ = ctx.stream_from_npy_file(npy, columns="xytp", **opt)
    assert torch.equal(ev, want)
    np.savez(str(tmp_path / "events.npz"), ts=t_ns, x=x16, y=y16, pol=p8)
    ev, t0, t1 = calibrate.load_events_npz(ctx, str(tmp_path / "events.npz"), **opt)
    assert torch.equal(ev, want)
    # a file the header parser refuses is refused with its text, a cut payload with both sizes
    np.save(npy, arr.astype(ITEMS[13].newbyteorder(">")))
    with pytest.raises(capi.EcalError) as e:
        ctx.stream_from_npy_file(npy, **opt)
    assert e.value.status == -1 and "big-endian" in str(e.value)
    np.save(npy, arr[:1000])
    data = open(npy, "rb").read()
    open(npy, "wb").write(data[:-3])
    with pytest.raises(capi.EcalError) as e:
        ctx.npy_to_bin(npy, str(tmp_path / "cut.bin"), **opt)
    assert e.value.status == -1 and "12997 bytes there, 13000 needed" in str(e.value)
    # no events
    np.save(npy, arr[:0])
    ev, info, _, _ = ctx.stream_from_npy_file(npy)
    assert ev.numel() == 0 and info["n_events"] == 0
    assert struct.pack("<d", w0) == records[:8]
