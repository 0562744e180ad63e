"""Measure the mcap ingest (design/25_mcap_ingest.md, design/09_measured.md): the n-event synthetic 346 x 260 stream written as three
MCAP files — dvs_msgs/EventArray messages (STRUCT), event_camera_msgs/EventPacket messages of "mono" words and of "evt3" words, all of
--message-events events (default 4096), --chunk-messages of them a chunk (default 14), nothing between them — then medians of
--warmup + --runs runs of
  - the decode in HBM (ecal_events_from_mcap_dev) of each, its passes from the library's own device events (ECAL_TRACE=load)
  - in the same run, ecal_events_from_bag_dev on the same events as a ROS 1 bag (tools/bag_ingest_probe.py's encoder), and the ratio
  - the host message index (ecal_mcap_index_messages over the file in host memory)
  - the host-to-device copy of the STRUCT file's bytes from pinned memory
  - evt3: the gather kernel alone against ecal_copy_dev of the same bytes, and ecal_events_from_raw_dev on the contiguous payload
  - ecal_stream_create_from_mcap_file (wall time, file in /dev/shm)
and one JSON line.
usage: python tools/mcap_ingest_probe.py [--events 50000000] [--message-events 4096] [--chunk-messages 14] [--warmup 5] [--runs 20]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["ECAL_TRACE"] = "load"
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bag_ingest_probe as BP  # noqa: E402
import eventcalib_amd  # noqa: E402
from eventcalib_amd import mcap  # noqa: E402
import mcap_writer as mw  # noqa: E402
import raw_ingest_probe as RP  # noqa: E402
import synth_stream as SS  # noqa: E402

BASE = 1600000000 * 10 ** 9
FRAME_ID = b"davis"
SENTINEL = 0x1122334455667788


def dev_bytes(b, device):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(device)


def le_bytes(v, dtype, width):
    return v.to(dtype).contiguous().view(torch.uint8).reshape(v.numel(), width)


def file_around(kind, fronts_and_bodies, rest_messages, cm, dev):
    """magic, header, a chunk with the schema and the channel, chunks of cm messages each (fronts_and_bodies: [n_msgs, msg_bytes] or
    None), a last chunk with the rest, data end, footer, magic"""
    schema = mw.DVS_SCHEMA if kind == mw.STRUCT else mw.PACKET_SCHEMA
    parts = [dev_bytes(mw.MAGIC + mw.header_record() + mw.chunk_record(mw.schema_record(*schema) + mw.channel_record(0, schema[0], "/dvs/events")), dev)]
    if fronts_and_bodies is not None and fronts_and_bodies.shape[0] >= cm:
        n_chunks, msg_bytes = fronts_and_bodies.shape[0] // cm, fronts_and_bodies.shape[1]
        chunk_front = mw.chunk_record(b"\0" * (cm * msg_bytes))[: -cm * msg_bytes]
        msgs = fronts_and_bodies[: n_chunks * cm].reshape(n_chunks, cm * msg_bytes)
        parts.append(torch.cat([dev_bytes(chunk_front, dev).expand(n_chunks, len(chunk_front)), msgs], 1).reshape(-1))
        left = fronts_and_bodies[n_chunks * cm:]
        if left.shape[0]:
            parts.append(dev_bytes(mw.chunk_record(b"\0" * left.numel())[: -left.numel()], dev))
            parts.append(left.reshape(-1))
    inner = b"".join(mw.message_record(0, m) for m in rest_messages)
    parts.append(dev_bytes((mw.chunk_record(inner) if inner else b"") + mw.record(mw.OP_DATA_END, bytes(4)) + mw.record(mw.OP_FOOTER, bytes(20)) + mw.MAGIC, dev))
    return torch.cat(parts)


def encode_struct(t_ns, x, y, p, per, cm):
    """dvs_msgs/EventArray messages of per events: event 0 of a message 13 bytes + 1, the later ones 16 apart (x 0, y 2, sec 6, nanosec 10,
    polarity 14), the last without its closing byte"""
    n, dev = t_ns.numel(), t_ns.device
    n_msgs = n // per
    body = None
    if n_msgs:
        m = n_msgs * per
        sec, nsec = le_bytes(t_ns[:m] // 10 ** 9, torch.int32, 4), le_bytes(t_ns[:m] % 10 ** 9, torch.int32, 4)
        xb, yb, pb = le_bytes(x[:m], torch.int16, 2), le_bytes(y[:m], torch.int16, 2), p[:m].to(torch.uint8).reshape(m, 1)
        z = torch.zeros(m, 2, dtype=torch.uint8, device=dev)
        later = torch.cat([xb, yb, z, sec, nsec, pb, z[:, :1]], 1).reshape(n_msgs, per, 16)
        first = torch.cat([xb, yb, sec, nsec, pb, z[:, :1]], 1).reshape(n_msgs, per, 14)[:, 0, :]
        events = torch.cat([first, later[:, 1:, :].reshape(n_msgs, (per - 1) * 16)], 1)[:, :-1]
        empty = mw.events_array(np.zeros(per), np.zeros(per), np.zeros(per), np.zeros(per), np.zeros(per))
        front = mw.message_record(0, mw.event_array_message(empty, frame_id=FRAME_ID))[: -events.shape[1]]
        body = torch.cat([dev_bytes(front, dev).expand(n_msgs, len(front)), events], 1)
    r = slice(n_msgs * per, n)
    rest = []
    if n_msgs * per < n:
        tn = t_ns[r].cpu().numpy()
        rest = [mw.event_array_message(mw.events_array(x[r].cpu().numpy(), y[r].cpu().numpy(), tn // 10 ** 9, tn % 10 ** 9, p[r].cpu().numpy()), frame_id=FRAME_ID)]
    return file_around(mw.STRUCT, body, rest, cm, dev)


def packet_fronts(encoding, payload_bytes, time_bases, dev):
    """the record header and the CDR fields in front of every packet's bytes [n_msgs, front bytes], time_base patched in"""
    one = mw.message_record(0, mw.event_packet_message(bytes(payload_bytes), encoding=encoding, time_base=SENTINEL, frame_id=FRAME_ID))[: -payload_bytes]
    at = one.index(SENTINEL.to_bytes(8, "little"))
    fronts = dev_bytes(one, dev).expand(time_bases.numel(), len(one)).clone()
    fronts[:, at: at + 8] = le_bytes(time_bases, torch.int64, 8)
    return fronts


def encode_mono(t_ns, x, y, p, per, cm):
    n, dev = t_ns.numel(), t_ns.device
    n_msgs = n // per
    body = None
    if n_msgs:
        m = n_msgs * per
        tb = t_ns[:m].reshape(n_msgs, per)[:, :1]
        words = (t_ns[:m].reshape(n_msgs, per) - tb) | (x[:m].reshape(n_msgs, per) << 32) | (y[:m].reshape(n_msgs, per) << 48) | (p[:m].reshape(n_msgs, per) << 63)
        body = torch.cat([packet_fronts(b"mono", 8 * per, tb.reshape(-1), dev), words.contiguous().view(torch.uint8).reshape(n_msgs, 8 * per)], 1)
    rest = []
    if n_msgs * per < n:
        r = slice(n_msgs * per, n)
        tn = t_ns[r].cpu().numpy()
        rest = [mw.event_packet_message(mw.mono_words(x[r].cpu().numpy(), y[r].cpu().numpy(), tn - tn[0], p[r].cpu().numpy()), time_base=int(tn[0]), frame_id=FRAME_ID)]
    return file_around(mw.MONO, body, rest, cm, dev)


def encode_evt3(payload, packet_bytes, cm):
    dev = payload.device
    n_msgs = payload.numel() // packet_bytes
    body = None
    if n_msgs:
        fronts = packet_fronts(b"evt3", packet_bytes, torch.zeros(n_msgs, dtype=torch.int64, device=dev), dev)
        body = torch.cat([fronts, payload[: n_msgs * packet_bytes].reshape(n_msgs, packet_bytes)], 1)
    left = payload[n_msgs * packet_bytes:].cpu().numpy().tobytes()
    rest = [mw.event_packet_message(left, encoding=b"evt3", frame_id=FRAME_ID)] if left else []
    return file_around(mw.EVT3, body, rest, cm, dev)


def median_of(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    return statistics.median(fn() for _ in range(runs))


def traced(fn, a, tag):
    """median wall time of fn over the runs, and the medians of the library's "ecal <tag> ingest:" phase lines of those runs"""
    trace = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)
    for _ in range(a.warmup):
        fn()
    sys.stderr.flush()
    os.dup2(trace.fileno(), 2)
    try:
        wall = 1e3 * statistics.median(fn() for _ in range(a.runs))
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(saved)
    trace.seek(0)
    phases = {}
    for m in re.finditer(r"ecal (\w+) ingest: (.+?)\s+([0-9.]+) ms", trace.read().decode()):
        if m.group(1) in tag:
            phases.setdefault(m.group(1) + ": " + m.group(2).strip(), []).append(float(m.group(3)))
    return wall, {k: statistics.median(v) for k, v in phases.items()}


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def probe(ctx, n, a):
    L = ctx._L
    t, xy, pol = SS.unpack_records(SS.make_stream(n, device="cuda"))
    t_ns = torch.round(t * 1e9).to(torch.int64) + BASE
    base = int(t_ns[0]) // 10 ** 9 * 10 ** 9
    x, y, p = xy[:, 0].to(torch.int64), xy[:, 1].to(torch.int64), pol.to(torch.int64)
    res = {"events": n, "message_events": a.message_events, "chunk_messages": a.chunk_messages, "warmup": a.warmup, "runs": a.runs}
    del t, xy, pol

    # ---- the bag ingest on the same events: the figure the STRUCT path is held against
    bag = BP.encode(t_ns, x, y, p, a.message_events, a.chunk_messages)
    table, info = ctx.bag_index_messages(bag.cpu().numpy())
    assert info["n_raw_events"] == n
    tab = torch.from_numpy(table.view("u1").copy()).cuda()
    wall, phases = traced(lambda: timed(lambda: ctx.events_from_bag(bag, tab, capacity=n, time_base=base)), a, ("bag",))
    res["bag"] = {"file_bytes": bag.numel(), "decode_wall_ms": wall, "decode_phases_ms": phases, "decode_device_ms": sum(phases.values())}
    want = ctx.events_from_bag(bag, tab, capacity=n, time_base=base)[0].clone()
    del bag, tab
    torch.cuda.empty_cache()

    for kind, name in ((mw.STRUCT, "struct"), (mw.MONO, "mono")):
        data = (encode_struct if kind == mw.STRUCT else encode_mono)(t_ns, x, y, p, a.message_events, a.chunk_messages)
        host = torch.empty(data.numel(), dtype=torch.uint8).pin_memory()
        host.copy_(data)
        r = {"file_bytes": data.numel()}

        def index():
            t0 = time.perf_counter()
            out = mcap.mcap_index_messages(ctx, host.numpy())
            return time.perf_counter() - t0, out
        r["host_index_ms"] = 1e3 * median_of(lambda: index()[0], 1, 5)
        table, info = index()[1]
        assert info["n_raw_events"] == n and info["first_stamp_ns"] == base and info["kind"] == kind, info
        r["messages"] = len(table)
        tab = torch.from_numpy(table.view("u1").copy()).cuda()
        got = mcap.events_from_mcap(ctx, data, tab, info["layout"], capacity=n, time_base=base)[0]
        assert torch.equal(got, want), "the records differ from the bag ingest's"
        del got
        wall, phases = traced(lambda: timed(lambda: mcap.events_from_mcap(ctx, data, tab, info["layout"], capacity=n, time_base=base)), a, ("mcap",))
        r.update(decode_wall_ms=wall, decode_phases_ms=phases, decode_device_ms=sum(phases.values()))
        r["ratio_to_bag_device"] = r["decode_device_ms"] / res["bag"]["decode_device_ms"]
        if kind == mw.STRUCT:
            dst = torch.empty_like(data)

            def h2d():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(host, non_blocking=True)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            r["h2d_ms"] = median_of(h2d, a.warmup, a.runs)
            del dst
            path = "/dev/shm/ecal_mcap_probe.mcap"
            with open(path, "wb") as f:
                host.numpy().tofile(f)

            def from_file():
                h = ctypes.c_void_p()
                t0 = time.perf_counter()
                rc = mcap.library().ecal_stream_create_from_mcap_file(ctx._h, path.encode(), None, ctypes.byref(h), None)
                dt = time.perf_counter() - t0
                assert rc == 0 and L.ecal_stream_size(h) == n, rc
                L.ecal_stream_destroy(h)
                return dt
            r["stream_from_mcap_file_s"] = median_of(from_file, 2, 5)
            os.remove(path)
        res[name] = r
        del data, host, tab
        torch.cuda.empty_cache()
    del want

    # ---- evt3 packets: the gather against a plain copy of the same bytes, the decode against the raw ingest on the contiguous payload
    t_us = (t_ns - BASE) // 1000
    payload = RP.encode("EVT3", t_us, x, y, p)
    payload = payload[: payload.numel() // 2 * 2]
    packet_bytes = max(2, payload.numel() // max(1, n // a.message_events) // 2 * 2)
    data = encode_evt3(payload, packet_bytes, a.chunk_messages)
    table, info = mcap.mcap_index_messages(ctx, data.cpu().numpy())
    assert info["n_payload_bytes"] == payload.numel() and info["kind"] == mw.EVT3, info
    tab = torch.from_numpy(table.view("u1").copy()).cuda()
    n_raw = ctx.raw_count_events(payload, "EVT3")
    want = ctx.events_from_raw(payload, "EVT3", capacity=n_raw, time_base=0)[0]
    got = mcap.events_from_mcap(ctx, data, tab, info["layout"], capacity=n_raw, time_base=0)[0]
    assert torch.equal(got, want)
    del got, want
    r = {"file_bytes": data.numel(), "payload_bytes": payload.numel(), "packet_bytes": packet_bytes, "messages": len(table)}
    wall, phases = traced(lambda: timed(lambda: mcap.events_from_mcap(ctx, data, tab, info["layout"], capacity=n_raw, time_base=0)), a, ("mcap", "raw"))
    r.update(decode_wall_ms=wall, decode_phases_ms=phases)
    wall, phases = traced(lambda: timed(lambda: ctx.events_from_raw(payload, "EVT3", capacity=n_raw, time_base=0)), a, ("raw",))
    r.update(raw_decode_wall_ms=wall, raw_decode_phases_ms=phases)
    dst = torch.empty_like(payload)

    def copy():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert L.ecal_copy_dev(ctx._h, dst.data_ptr(), payload.data_ptr(), payload.numel(), torch.cuda.current_stream().cuda_stream, 0) == 0
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    r["copy_dev_ms"] = median_of(copy, a.warmup, a.runs)
    r["gather_ms"] = r["decode_phases_ms"].get("mcap: gather")
    r["gather_to_copy"] = r["gather_ms"] / r["copy_dev_ms"] if r["gather_ms"] else None
    res["evt3"] = r
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--message-events", type=int, default=4096)
    ap.add_argument("--chunk-messages", type=int, default=14)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    ctx = eventcalib_amd.Context(0)
    probe(ctx, a.events, a)


if __name__ == "__main__":
    main()
