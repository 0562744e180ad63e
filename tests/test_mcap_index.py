"""CPU suite: ecal_mcap_index_messages (include/ecal_mcap.h) through ctypes, no context and no device, against the reader of
tests/mcap_writer.py, which restates the contract and shares no code with the library: the table and the info must be equal on random
files of every kind (chunked and unchunked, other channels interleaved, with and without a summary section, frame_id and topic
lengths that put the events at every offset mod 16), and on a small file cut at every byte — each cut gives ECAL_OK with the records
wholly present, or an error where the reader raises too."""
import os

import numpy as np
import pytest

import eventcalib_amd
from eventcalib_amd import capi, mcap

import mcap_writer as mw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_FIELDS = ("n_raw_events", "n_messages", "n_other_messages", "n_chunks", "n_schemas", "n_channels", "n_trailing_bytes", "first_stamp_ns",
                "msg_width", "msg_height", "n_payload_bytes", "kind", "layout")
S0 = 1600000000


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    mcap.library()


def index_both(data, topic=None):
    """(table, info) of the library when both agree; the reader's exception and the library's refusal must come together"""
    try:
        want_table, want_info = mw.index_messages(data, topic=topic)
    except mw.McapError as e:
        with pytest.raises(capi.EcalError) as err:
            mcap.mcap_index_messages(None, data, topic=topic)
        assert err.value.status == -1, str(e)
        return None, None
    table, info = mcap.mcap_index_messages(None, data, topic=topic)
    assert table.tobytes() == want_table.tobytes()
    assert {k: info[k] for k in INDEX_FIELDS} == {k: want_info[k] for k in INDEX_FIELDS}
    return table, info


def random_events(rng, n, sec=S0):
    t = np.sort(rng.integers(0, 2 * 10 ** 9, n))
    return mw.events_array(rng.integers(0, 346, n), rng.integers(0, 260, n), sec + t // 10 ** 9, t % 10 ** 9, rng.integers(0, 2, n))


def random_file(rng, kind, n_messages, topic="/dvs/events"):
    schemas = [mw.DVS_SCHEMA, mw.PACKET_SCHEMA, mw.IMAGE_SCHEMA]
    channels = [(7, 1 if kind == mw.STRUCT else 2, topic), (8, 3, "/camera/image_raw"), (9, 0, "/rosout", "json")]
    messages = []
    for k in range(n_messages):
        frame_id = bytes(rng.integers(97, 123, int(rng.integers(0, 16)), dtype=np.uint8))
        n = int(rng.integers(0, 5)) if k % 3 else int(rng.integers(0, 40))
        if kind == mw.STRUCT:
            data = mw.event_array_message(random_events(rng, n), frame_id=frame_id)
        elif kind == mw.MONO:
            data = mw.event_packet_message(mw.mono_words(rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2 ** 32, n), rng.integers(0, 2, n)),
                                           encoding=b"mono", time_base=S0 * 10 ** 9 + 1000 * k, frame_id=frame_id)
        else:
            data = mw.event_packet_message(bytes(rng.integers(0, 256, 2 * n, dtype=np.uint8)), encoding=b"evt3", frame_id=frame_id)
        messages.append((7, data))
        if rng.integers(0, 3) == 0:
            messages.append((8 + int(rng.integers(0, 2)), bytes(rng.integers(0, 256, int(rng.integers(0, 50)), dtype=np.uint8))))
    return mw.write_mcap(schemas, channels, messages, per_chunk=[int(v) for v in rng.integers(0, 6, 4)], summary=bool(rng.integers(0, 2)),
                         closed=bool(rng.integers(0, 4)))


@pytest.mark.parametrize("kind", [mw.STRUCT, mw.MONO, mw.EVT3])
def test_random_files_index_as_the_reader_does(kind):
    rng = np.random.default_rng(100 + kind)
    residues, with_messages = set(), 0
    for it in range(60):
        topic = "/" + "e" * int(rng.integers(1, 20))
        data = random_file(rng, kind, int(rng.integers(0, 41)), topic=topic)
        table, info = index_both(data, topic=None if it % 2 else topic)
        if table is None:          # no message of the channel: the writer leaves its channel record out too, and both refuse
            continue
        assert info["kind"] == kind and len(table) > 0
        with_messages += 1
        residues |= set((table["offset"][table["n"] > 0] % 16).tolist())
    assert with_messages > 40
    assert residues == set(range(16))


def test_event_offsets_fall_on_every_residue_of_the_file():
    """CDR aligns within a message; the message's place in the file is arbitrary: topic and frame_id lengths move event 0 to every
    offset mod 16"""
    seen = set()
    rng = np.random.default_rng(5)
    for pad in range(16):
        messages = [(8, b"x" * pad), (7, mw.event_array_message(random_events(rng, 3), frame_id=b"cam"))]
        data = mw.write_mcap([mw.DVS_SCHEMA, mw.IMAGE_SCHEMA], [(7, 1, "/dvs/events"), (8, 3, "/i")], messages, per_chunk=2)
        table, _ = index_both(data)
        seen.add(int(table["offset"][0]) % 16)
    assert seen == set(range(16))


@pytest.mark.parametrize("kind,per_chunk", [(mw.STRUCT, 2), (mw.MONO, 0), (mw.EVT3, 3)])
def test_a_file_cut_at_every_byte(kind, per_chunk):
    rng = np.random.default_rng(7)
    schemas = [mw.DVS_SCHEMA, mw.PACKET_SCHEMA, mw.IMAGE_SCHEMA]
    channels = [(1, 1 if kind == mw.STRUCT else 2, "/ev"), (2, 3, "/image")]
    messages = []
    for k in range(5):
        if kind == mw.STRUCT:
            data = mw.event_array_message(random_events(rng, k), frame_id=b"ab"[: k % 3])
        elif kind == mw.MONO:
            data = mw.event_packet_message(mw.mono_words([k] * k, [k] * k, list(range(k)), [1] * k), time_base=S0 * 10 ** 9, frame_id=b"ab"[: k % 3])
        else:
            data = mw.event_packet_message(bytes(range(2 * k)), encoding=b"evt3")
        messages += [(1, data), (2, b"\x07" * (3 * k))]
    whole = mw.write_mcap(schemas, channels, messages, per_chunk=per_chunk)
    full, _ = index_both(whole)
    assert len(full) == 5
    ok = refused = 0
    counts = set()
    for cut in range(len(whole)):
        table, info = index_both(whole[:cut])
        if table is None:
            refused += 1
            continue
        ok += 1
        counts.add(len(table))
        assert table.tobytes() == full[: len(table)].tobytes()          # the wholly-present prefix
    assert ok > len(whole) // 2 and refused > 8 and counts == {0, 1, 2, 3, 4, 5}


def test_capacity_of_the_table():
    rng = np.random.default_rng(9)
    data = mw.write_mcap([mw.DVS_SCHEMA], [(1, 1, "/ev")], [(1, mw.event_array_message(random_events(rng, 4))) for _ in range(3)])
    with pytest.raises(capi.EcalError) as e:
        mcap.mcap_index_messages(None, data, capacity=2)
    assert e.value.status == -6 and e.value.info["n_messages"] == 3 and e.value.info["kind"] == mw.STRUCT
    table, info = mcap.mcap_index_messages(None, data, capacity=3)
    assert len(table) == 3 and info["n_raw_events"] == 12
