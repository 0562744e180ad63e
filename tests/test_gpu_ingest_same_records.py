"""GPU: the table ingests decode the same events into the same records.  One list of 2 B + 1 events (B = ecal_bag_block_events(), the
slots of a decode block) is written by the tests' pure-Python writers as a ROS 1 bag, an MCAP file of dvs_msgs/EventArray messages
(STRUCT), an MCAP file of mono packets (MONO), an AEDAT 3.1 payload, an AEDAT 4 file without compression and AEDAT 2.0 records, cut
into the same messages / packets: one boundary between slots B - 1 and B, one message of no events.  Every format goes through its
_dev form with the same filter — a start_time that drops the first two events, a width that puts a few outside, an end_time that first
bites at slot B + 3, inside the second block — and the records' bytes and the counters the formats share must be equal across all six,
and equal to what the list gives by hand.  The verdict and write kernels of the six are one body (slot_kernels.hpp) and their host
side one driver (ingest_driver.hpp): this pins that they cannot drift apart, at the smallest shape that crosses a block, a stop and an
empty table entry.

Stamps: whole microseconds below one AEDAT 2.0 wrap, and only those k at which the nanosecond formats' t = (1000 k) * 1e-9 and the
microsecond formats' t = k * 1e-6 round to the same double (the two products differ in the last bit for about two stamps in three).
Before any GPU work the writers' own readers decode the six inputs, unfiltered, to the same records on the CPU."""
import numpy as np
import pytest
import torch

import aedat4_oracle as AO
import aedat4_writer as AW
import bag_writer as bw
import mcap_writer as mw
import test_gpu_aedat4_ingest as T4
import test_gpu_aedat_ingest as TA
import test_gpu_bag_ingest as TB
import test_gpu_mcap_ingest as TM
import eventcalib_amd
from eventcalib_amd import mcap

pytestmark = pytest.mark.gpu

REC = TA.REC
BASE_US = 5_000_000                              # the time base in microseconds: below 2^31, so no AEDAT 3.1 overflow and no 2.0 wrap
SHARED = ("n_raw_events", "n_events", "n_outside", "n_negative", "n_before_start", "n_after_end")
WIDTH, HEIGHT = 340, 260                         # the events are on 346 x 260: those with x >= 340 are outside
FORMATS = ("bag", "mcap struct", "mcap mono", "aedat 3.1", "aedat4 none", "aedat 2.0")


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


def event_list(B):
    """(k: microseconds behind the base, x, y, p) of 2 B + 1 events, and the cuts of the messages"""
    n = 2 * B + 1
    k = np.array([v for v in range(1000, 1000 + 8 * n) if float(v) * 1e-6 == float(1000 * v) * 1e-9][:n], np.int64)
    assert len(k) == n
    rng = np.random.default_rng(5)
    x, y, p = rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n)
    x[[0, 1, 2, B + 3]] = 10                      # the events the start and the end are placed by are on the sensor
    cuts = [0, 7, 7, 300, B, B + 500, n]          # an empty message; a boundary between slots B - 1 and B
    return k, x, y, p, cuts


def expected(k, x, y, p, B):
    """the filter by hand -> (records' bytes, the shared counters); no filter: B = None"""
    t = k.astype(np.float64) * 1e-6
    n = len(k)
    live = np.arange(n) < (B + 3 if B is not None else n)
    outside = live & (x >= WIDTH) if B is not None else np.zeros(n, bool)
    before = live & ~outside & (np.arange(n) < 2) if B is not None else np.zeros(n, bool)
    keep = live & ~outside & ~before
    rec = np.zeros(int(keep.sum()), REC)
    rec["t"], rec["x"], rec["y"], rec["p"] = t[keep], x[keep], y[keep], p[keep]
    return rec.tobytes(), dict(n_raw_events=n, n_events=int(keep.sum()), n_outside=int(outside.sum()), n_negative=0,
                               n_before_start=int(before.sum()), n_after_end=n - int(live.sum()))


def write_all(k, x, y, p, cuts):
    """the six inputs, cut alike"""
    t_us = BASE_US + k
    t_ns = 1000 * t_us
    parts = list(zip(cuts, cuts[1:]))
    ev_ns = (x, y, t_ns, p)
    out = {}
    out["bag"] = TB.bag([TB.msg(bw.events_array(x[a:b], y[a:b], t_ns[a:b] // 10 ** 9, t_ns[a:b] % 10 ** 9, p[a:b]), frame_id=b"ab"[: i % 3])
                         for i, (a, b) in enumerate(parts)], per_chunk=2)
    for name, kind in (("mcap struct", mw.STRUCT), ("mcap mono", mw.MONO)):
        out[name] = TM.file_of(kind, [TM.msg(kind, TM.cut(ev_ns, a, b), frame_id=b"ab"[: i % 3]) for i, (a, b) in enumerate(parts)], per_chunk=2)
    out["aedat 3.1"] = b"".join(TA.polarity([TA.ev(int(x[i]), int(y[i]), int(p[i]), int(t_us[i])) for i in range(a, b)]) for a, b in parts)
    out["aedat4 none"] = T4.event_file([AW.make_events(t_us[a:b], x[a:b], y[a:b], p[a:b]) for a, b in parts], compression=AW.NONE)
    out["aedat 2.0"] = TA.payload20([TA.dvs(int(x[i]), int(y[i]), int(p[i]), int(t_us[i])) for i in range(len(k))])
    return out


def on_the_cpu(name, data, **flt):
    """the writers' own readers -> the records' bytes"""
    if name == "bag":
        return bw.decode(data, time_base=1000 * BASE_US, **flt)[0]
    if name.startswith("mcap"):
        return mw.decode(data, time_base=1000 * BASE_US, **flt)[0]
    if name.startswith("aedat "):
        return TA.oracle(data, name[6:], time_base=BASE_US, **flt)[0]
    return AO.decode(data, time_base=BASE_US, **flt)[0].tobytes()


def on_the_gpu(ctx, name, data, **flt):
    """index on the host where the format has a table, the _dev form -> (the records' bytes, info)"""
    if name == "bag":
        table, _ = ctx.bag_index_messages(data)
        got, info = ctx.events_from_bag(data, table, time_base=1000 * BASE_US, **flt)
    elif name.startswith("mcap"):
        table, tinfo = ctx.mcap_index_messages(data)
        got, info = ctx.events_from_mcap(data, table, tinfo["layout"], time_base=1000 * BASE_US, **flt)
    elif name == "aedat 3.1":
        table, _ = ctx.aedat_index_packets(data, source=-1)
        got, info = ctx.events_from_aedat(data, "3.1", packets=table, time_base=BASE_US, **flt)
    elif name == "aedat 2.0":
        got, info = ctx.events_from_aedat(data, "2.0", packets=None, time_base=BASE_US, **flt)
    else:
        table, tinfo = ctx.aedat4_index_packets(data)
        got, info = ctx.events_from_aedat4(data, tinfo["compression"], table, time_base=BASE_US, **flt)
    torch.cuda.synchronize()
    return got.cpu().numpy().tobytes(), info


def test_six_formats_one_list_the_same_records_and_counters(ctx):
    B = ctx.bag_block_events()
    assert B == 1024 and ctx.aedat_block_events("3.1") == B and ctx.aedat4_block_events() == B and mcap.mcap_block_events() == B
    k, x, y, p, cuts = event_list(B)
    assert BASE_US + int(k[-1]) < 1 << 31
    inputs = write_all(k, x, y, p, cuts)
    assert tuple(inputs) == FORMATS
    # on the CPU first: the six inputs hold the same list
    plain, _ = expected(k, x, y, p, None)
    for name, data in inputs.items():
        assert on_the_cpu(name, data) == plain, name
    # the same filter for every format
    t = k.astype(np.float64) * 1e-6
    flt = dict(width=WIDTH, height=HEIGHT, start_time=float(t[2]), end_time=float(t[B + 3]))
    want, want_counters = expected(k, x, y, p, B)
    assert want_counters["n_before_start"] == 2 and want_counters["n_after_end"] == B - 2 and 3 <= want_counters["n_outside"] <= 60
    for name, data in inputs.items():
        assert on_the_cpu(name, data, **flt) == want, name
    results = {name: on_the_gpu(ctx, name, data, **flt) for name, data in inputs.items()}
    for name, (records, info) in results.items():
        counters = {c: info[c] for c in SHARED}
        print(name, counters)
        assert counters == want_counters, name
        assert records == want, name
        assert records == results["bag"][0] and counters == {c: results["bag"][1][c] for c in SHARED}, name
    for name in ("aedat 3.1", "aedat 2.0"):
        assert results[name][1]["n_invalid"] == 0
