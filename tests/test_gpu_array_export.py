"""GPU: the array ingest's reverse (ecal_events_to_fields_dev; eventcalib_amd/csrc/ecal_fields.hip) — packed records unpacked into
columns of the asked types — against the numpy oracle (tests/fields_oracle.py) element for element, and the .npy writer
(ecal_stream_to_npy_file) against numpy's own reader.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import eventcalib_amd
import fields_oracle as FO
from eventcalib_amd import calibrate, capi

pytestmark = pytest.mark.gpu

UNPACK_T = 256      # threads (= records) per workgroup of the unpack kernel


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def events():
    """3 * 256 + 7 records on a 100 x 100 sensor with integral coordinates and microsecond stamps: every output type holds them"""
    cols = FO.random_columns(np.random.default_rng(31), 3 * UNPACK_T + 7, width=100, height=100)
    return FO.from_fields(*cols)[0]


OUT_CASES = [(np.float64, np.float64, np.uint8), (np.float32, np.float32, np.float32), (np.int64, np.uint16, np.bool_), (np.uint32, np.int16, np.int8),
             (np.int32, np.uint8, np.uint16), (np.int64, np.int8, np.int64), (np.int64, np.uint32, np.float64), (np.int64, np.int32, np.int32),
             (np.int64, np.int64, np.uint32)]


@pytest.mark.parametrize("t,xy,p", OUT_CASES, ids=["-".join(np.dtype(d).name for d in c) for c in OUT_CASES])
def test_each_output_type_equals_numpy(ctx, events, t, xy, p):
    signed = np.dtype(p).kind in "if"
    for n in (0, 1, UNPACK_T - 1, UNPACK_T, UNPACK_T + 1, 3 * UNPACK_T + 7):
        ev = events[: n * 25]
        got = ctx.events_to_arrays(ev, t=t, xy=xy, p=p, polarity_signed=signed, ticks_per_second=1e6, time_base=77)
        want, bad = FO.to_fields(ev, t=t, xy=xy, p=p, polarity_signed=signed, time_base=77)
        assert not bad.any()
        for k in "txyp":
            g = got[k].cpu()
            assert got[k].is_cuda and g.numel() == n
            assert g.view(torch.uint8).numpy().tobytes() == want[k].tobytes(), (k, n)
    # records at an odd address: a view one byte into a larger tensor
    shifted = torch.zeros(events.size + 1, dtype=torch.uint8, device="cuda")
    shifted[1:] = torch.from_numpy(events.copy()).cuda()
    got = ctx.events_to_arrays(shifted[1:], t=t, xy=xy, p=p, polarity_signed=signed)
    want, _ = FO.to_fields(events, t=t, xy=xy, p=p, polarity_signed=signed)
    assert all(got[k].cpu().view(torch.uint8).numpy().tobytes() == want[k].tobytes() for k in "txyp")


@pytest.mark.parametrize("item,shift", [(13, 1), (14, 2), (16, 3), (13, 0)])
def test_columns_inside_packed_items_keep_the_bytes_between_them(ctx, events, item, shift):
    dt = {13: np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")]),
          14: np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1"), ("gap", "u1")]),
          16: np.dtype([("t", "<f8"), ("x", "<f4"), ("y", "<u2"), ("p", "i1"), ("gap", "u1")])}[item]
    assert dt.itemsize == item
    n = events.size // 25
    out = torch.full((shift + n * item + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    f = (capi.Field * 4)()
    for k, name in enumerate("txyp"):
        f[k] = capi.Field(out.data_ptr() + shift + dt.fields[name][1], item, capi.field_type(dt[name]), 0)
    rec = torch.from_numpy(events.copy()).cuda()
    info = ctx.events_to_fields_dev(rec.data_ptr(), n, f, capi.to_fields_options(), torch.cuda.current_stream().cuda_stream)
    assert info == {"n_events": n, "n_unrepresentable": 0}
    h = out.cpu().numpy()
    assert (h[:shift] == 0xCD).all() and (h[shift + n * item:] == 0xCD).all()              # nothing outside the items
    arr = h[shift: shift + n * item].view(dt)
    want, _ = FO.to_fields(events, t=dt["t"], xy=np.float64, p=dt["p"])
    assert arr["t"].tobytes() == want["t"].tobytes() and arr["p"].tobytes() == want["p"].tobytes()
    assert (arr["x"] == FO.records(events)["x"]).all() and (arr["y"] == FO.records(events)["y"]).all()
    if "gap" in dt.names:
        assert (arr["gap"] == 0xCD).all()                                                  # ... and nothing between the elements
    # back in through the ingest: the same records
    back, _ = ctx.events_from_structured(arr.copy(), time_magnitude=1.0 if dt["t"].kind == "f" else 1e-6)
    assert back.cpu().numpy().tobytes() == events.tobytes()


def test_what_is_not_representable_is_counted(ctx, events):
    rec = FO.records(events).copy()
    rec["x"][::5] += 0.25                                   # sub-pixel coordinates
    rec["y"][3] = -1.0
    rec["y"][4] = 70000.0
    rec["t"][6], rec["t"][7], rec["t"][8] = np.nan, np.inf, 1e300
    ev = rec.view(np.uint8).reshape(-1)
    _, bad = FO.to_fields(ev, t=np.int64, xy=np.uint16)
    assert 0 < bad.sum() < rec.size
    with pytest.raises(capi.EcalError) as e:
        ctx.events_to_arrays(ev, t=np.int64, xy=np.uint16)
    assert e.value.status == -6 and e.value.info == {"n_events": rec.size, "n_unrepresentable": int(bad.sum())}
    _, bad = FO.to_fields(ev, t=np.float64, xy=np.int32)
    with pytest.raises(capi.EcalError) as e:
        ctx.events_to_arrays(ev, xy=np.int32)
    assert e.value.status == -6 and e.value.info["n_unrepresentable"] == int(bad.sum()) == len(rec["x"][::5]) - 0
    # float outputs hold everything
    got = ctx.events_to_arrays(ev, t=np.float32, xy=np.float32)
    want, _ = FO.to_fields(ev, t=np.float32, xy=np.float32)
    assert all(got[k].cpu().view(torch.uint8).numpy().tobytes() == want[k].tobytes() for k in "txyp")


def test_refusals(ctx, events):
    with pytest.raises(capi.EcalError) as e:
        ctx.events_to_arrays(events, p=np.uint8, polarity_signed=True)
    assert e.value.status == -1 and "field p" in str(e.value) and "unsigned" in str(e.value)
    with pytest.raises(capi.EcalError) as e:
        ctx.events_to_arrays(events, t=np.int16)
    assert e.value.status == -1 and "field t" in str(e.value)
    with pytest.raises(capi.EcalError) as e:
        ctx.events_to_arrays(events, ticks_per_second=0.0)
    assert e.value.status == -1 and "ticks_per_second" in str(e.value)
    # an output column inside the records
    n = events.size // 25
    rec = torch.from_numpy(events.copy()).cuda()
    spare = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    f = (capi.Field * 4)(*[capi.Field(spare.data_ptr(), 8, 8, 0)] * 4)
    f[2] = capi.Field(rec.data_ptr() + n * 25 - 1, 8, 8, 0)
    with pytest.raises(capi.EcalError) as e:
        ctx.events_to_fields_dev(rec.data_ptr(), n, f, capi.to_fields_options(), 0)
    assert e.value.status == -1 and "field y overlaps the records" in str(e.value)


def test_a_stream_as_npy_is_what_numpy_loads_and_reads_back_identical(ctx, tmp_path, events):
    npy = str(tmp_path / "out.npy")
    ctx.stream_to_npy(torch.from_numpy(events.copy()).cuda(), npy)
    loaded = np.load(npy)
    assert loaded.dtype == FO.RECORD and loaded.tobytes() == events.tobytes()
    assert (len(open(npy, "rb").read()) - events.size) % 64 == 0                  # numpy's padding of the header
    back, info, t0, t1 = ctx.stream_from_npy_file(npy)                            # float stamps: time_magnitude 1.0 by the header
    assert back.cpu().numpy().tobytes() == events.tobytes() and info["n_events"] == events.size // 25
    assert (t0, t1) == (loaded["t"][0], loaded["t"][-1])
    # the stream sorts first: a shuffled input comes out in time order (stable)
    rec = FO.records(events)
    idx = np.random.default_rng(2).permutation(rec.size)
    calibrate.save_events_npy(ctx, rec[idx].view(np.uint8).reshape(-1), npy)
    assert np.load(npy).tobytes() == rec[idx][np.argsort(rec[idx]["t"], kind="stable")].tobytes()
    # no records: a file numpy loads as an empty array of the dtype
    ctx.stream_to_npy(np.zeros(0, np.uint8), npy)
    assert np.load(npy).shape == (0,) and np.load(npy).dtype == FO.RECORD
