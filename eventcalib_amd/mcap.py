"""Mcap ingest: the binding of include/ecal_mcap.h (the same libecal.so; design/25_mcap_ingest.md) — ROS 2 MCAP recordings of event
messages (dvs_msgs / prophesee_event_msgs EventArray, event_camera_msgs EventPacket with "mono" or "evt3" packets) decoded in HBM.

The prototypes of that header live here, in a table of their own, and are set on the handle of eventcalib_amd.load_library() by
apply_prototypes — capi.PROTOTYPES is the table of ecal.h and stays that.

    mcap_index_messages(ctx, data, topic=None)        the host indexer -> (table as MCAP_MESSAGE_DTYPE, info dict with the layout)
    mcap_count_events(ctx, data, table, layout)       the events before any drop
    events_from_mcap(ctx, data, table, layout, ...)   the device form -> (records as a uint8 CUDA tensor, info dict)
    mcap_to_bin(ctx, mcap_path, bin_path, ...)        the file's records in file order as a .bin
    stream_from_mcap_file(ctx, path, ...)             the file as a stream in time order -> (events, info, t_first, t_last)
"""
import ctypes
import os

import numpy as np

from . import capi

MCAP_NONE, MCAP_STRUCT, MCAP_MONO, MCAP_EVT3 = 0, 1, 2, 3   # ECAL_MCAP_*
KIND_NAMES = {MCAP_NONE: "none", MCAP_STRUCT: "struct", MCAP_MONO: "mono", MCAP_EVT3: "evt3"}


class McapOptions(ctypes.Structure):
    """ecal_mcap_options.  topic is a byte string that must outlive the call (mcap_options keeps it on the object)."""
    _fields_ = [("topic", ctypes.c_char_p), ("auto_time_base", ctypes.c_int), ("time_base", ctypes.c_int64), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("flip_x", ctypes.c_int), ("flip_y", ctypes.c_int), ("start_time", ctypes.c_double),
                ("has_end_time", ctypes.c_int), ("end_time", ctypes.c_double)]


class McapLayout(ctypes.Structure):
    """ecal_mcap_layout: 32 bytes."""
    _fields_ = [("kind", ctypes.c_uint32), ("lead", ctypes.c_uint32), ("stride", ctypes.c_uint32), ("span", ctypes.c_uint32 * 2),
                ("x", ctypes.c_uint8 * 2), ("y", ctypes.c_uint8 * 2), ("sec", ctypes.c_uint8 * 2), ("nsec", ctypes.c_uint8 * 2),
                ("pol", ctypes.c_uint8 * 2), ("x_bytes", ctypes.c_uint8), ("y_bytes", ctypes.c_uint8)]

    def as_dict(self):
        return {name: (list(getattr(self, name)) if name in ("span", "x", "y", "sec", "nsec", "pol") else int(getattr(self, name)))
                for name, _ in self._fields_}

    @classmethod
    def from_dict(cls, d):
        L = cls()
        for name, _ in cls._fields_:
            v = d.get(name, 0)
            if name in ("span", "x", "y", "sec", "nsec", "pol"):
                getattr(L, name)[0], getattr(L, name)[1] = (int(v[0]), int(v[1])) if v else (0, 0)
            else:
                setattr(L, name, int(v))
        return L


class McapInfo(ctypes.Structure):
    """ecal_mcap_info."""
    _fields_ = [("n_raw_events", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("n_outside", ctypes.c_uint64),
                ("n_negative", ctypes.c_uint64), ("n_before_start", ctypes.c_uint64), ("n_after_end", ctypes.c_uint64),
                ("n_messages", ctypes.c_uint64), ("n_other_messages", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64),
                ("n_schemas", ctypes.c_uint64), ("n_channels", ctypes.c_uint64), ("n_trailing_bytes", ctypes.c_uint64),
                ("first_stamp_ns", ctypes.c_int64), ("time_base", ctypes.c_int64), ("msg_width", ctypes.c_uint32),
                ("msg_height", ctypes.c_uint32), ("n_payload_bytes", ctypes.c_uint64), ("n_no_state", ctypes.c_uint64),
                ("n_other_words", ctypes.c_uint64), ("n_time_wraps", ctypes.c_uint64), ("layout", McapLayout)]

    def as_dict(self):
        d = {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "layout"}
        d["layout"] = self.layout.as_dict()
        d["kind"] = int(self.layout.kind)
        return d


class McapMessage(ctypes.Structure):
    """ecal_mcap_message: 24 bytes."""
    _fields_ = [("offset", ctypes.c_uint64), ("n", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("time_base_ns", ctypes.c_int64)]


MCAP_MESSAGE_DTYPE = np.dtype([("offset", "<u8"), ("n", "<u4"), ("reserved", "<u4"), ("time_base_ns", "<i8")])

_P = ctypes.c_void_p
_u64 = ctypes.c_uint64
_PO, _PI, _PL = ctypes.POINTER(McapOptions), ctypes.POINTER(McapInfo), ctypes.POINTER(McapLayout)
PROTOTYPES = {
    "ecal_mcap_default_options": (None, [_PO]),
    "ecal_mcap_block_events": (ctypes.c_uint32, []),
    "ecal_mcap_index_messages": (ctypes.c_int, [_P, _P, _u64, _PO, _P, _u64, ctypes.POINTER(_u64), _PI]),
    "ecal_mcap_count_events_dev": (ctypes.c_int, [_P, _P, _u64, _P, _u64, _PL, ctypes.POINTER(_u64), _P]),
    "ecal_events_from_mcap_dev": (ctypes.c_int, [_P, _P, _u64, _P, _u64, _PL, _PO, _P, _u64, _PI, _P]),
    "ecal_stream_create_from_mcap_file": (ctypes.c_int, [_P, ctypes.c_char_p, _PO, ctypes.POINTER(_P), _PI]),
    "ecal_mcap_to_bin_file": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_char_p, _PO, _PI]),
}

_applied = None


def apply_prototypes(L):
    """the one place a prototype of ecal_mcap.h is set on a library handle (a missing symbol raises AttributeError)"""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


def library():
    """libecal.so with this module's prototypes in place"""
    global _applied
    L = capi.load_library()
    if _applied is not L:
        _applied = apply_prototypes(L)
    return L


def mcap_options(topic=None, time_base=None, width=0, height=0, flip_x=False, flip_y=False, start_time=None, end_time=None):
    """ecal_mcap_options from ecal_mcap_default_options: topic None = every chosen channel (one topic), time_base None = automatic
    (the first event's whole second; 0 for evt3), else int64 nanoseconds of epoch time (evt3: microseconds of the camera's clock),
    width / height 0 = no bound, flip_x / flip_y need them, start_time None = -inf, end_time None = to the end."""
    o = McapOptions()
    library().ecal_mcap_default_options(ctypes.byref(o))
    o.topic = os.fsencode(topic) if topic else None
    if time_base is not None:
        o.auto_time_base, o.time_base = 0, int(time_base)
    o.width, o.height = int(width), int(height)
    o.flip_x, o.flip_y = int(bool(flip_x)), int(bool(flip_y))
    if start_time is not None:
        o.start_time = float(start_time)
    if end_time is not None:
        o.has_end_time, o.end_time = 1, float(end_time)
    return o


def mcap_block_events():
    """ecal_mcap_block_events: event slots per decode block of this build."""
    return int(library().ecal_mcap_block_events())


def _fail(L, ctx, st, info, what):
    """EcalError of an entry point with the info it filled as .info; ctx None (the indexer without a context): the status' own text"""
    if ctx is not None:
        ctx._fail_with_info(st, info)
    e = capi.EcalError(st, L.ecal_strerror(st).decode() + ": " + what)
    e.info = info.as_dict()
    raise e


def mcap_index_messages(ctx, data, topic=None, capacity=None):
    """ecal_mcap_index_messages over a file's bytes in host memory (bytes or a numpy uint8 array); ctx may be None (no device is
    touched either way) -> (table as a numpy array of MCAP_MESSAGE_DTYPE, info dict: "layout" is what the device form takes).
    capacity None: counted first."""
    L = library()
    o = mcap_options(topic=topic)
    a = capi._u8_array(data)
    ptr = a.ctypes.data if a.size else None
    h = ctx._h if ctx is not None else None
    n, info = ctypes.c_uint64(), McapInfo()
    if capacity is None:
        st = L.ecal_mcap_index_messages(h, ptr, a.size, ctypes.byref(o), None, 0, ctypes.byref(n), ctypes.byref(info))
        if st not in (0, -6):
            _fail(L, ctx, st, info, "ecal_mcap_index_messages")
        capacity = int(n.value)
    table = np.zeros(int(capacity), MCAP_MESSAGE_DTYPE)
    st = L.ecal_mcap_index_messages(h, ptr, a.size, ctypes.byref(o), table.ctypes.data if table.size else None, table.size, ctypes.byref(n),
                                    ctypes.byref(info))
    if st != 0:
        _fail(L, ctx, st, info, "ecal_mcap_index_messages")
    return table[: int(n.value)], info.as_dict()


def _layout(layout):
    return layout if isinstance(layout, McapLayout) else McapLayout.from_dict(layout)


def _device_args(ctx, data, table):
    """(file tensor, table tensor, [d_file, n_bytes, d_table, n_messages])"""
    import torch
    t = ctx._bytes_tensor(data)
    if table is None:
        pk = torch.zeros(0, dtype=torch.uint8, device=t.device)
    elif isinstance(table, torch.Tensor):
        pk = table.contiguous().view(torch.uint8).reshape(-1).to(t.device)
    else:
        a = np.ascontiguousarray(table, MCAP_MESSAGE_DTYPE)
        pk = torch.from_numpy(a.view(np.uint8).copy()).to(t.device) if a.size else torch.zeros(0, dtype=torch.uint8, device=t.device)
    n = pk.numel() // 24
    return t, pk, [t.data_ptr() if t.numel() else None, t.numel(), pk.data_ptr() if n else None, n]


def mcap_count_events(ctx, data, table, layout):
    """ecal_mcap_count_events_dev: the events before any drop (always a sufficient capacity)."""
    import torch
    t, pk, args = _device_args(ctx, data, table)
    n = ctypes.c_uint64()
    lay = _layout(layout)
    ctx._check(library().ecal_mcap_count_events_dev(ctx._h, *args, ctypes.byref(lay), ctypes.byref(n), torch.cuda.current_stream().cuda_stream))
    return int(n.value)


def events_from_mcap(ctx, data, table, layout, capacity=None, out=None, **options):
    """ecal_events_from_mcap_dev: the whole file (bytes, a numpy uint8 array or a torch uint8 tensor; a CUDA tensor is decoded where
    it is), the table and the layout of mcap_index_messages -> (packed 25-byte records in file order as a uint8 CUDA tensor
    [n_events * 25], info dict).  options: mcap_options' — the device form needs an explicit time_base.  capacity None:
    mcap_count_events; a smaller one raises EcalError with status -6 and .info["n_events"] = the count needed.  out: a uint8 CUDA
    tensor to write into (any alignment, capacity * 25 bytes at least)."""
    import torch
    L = library()
    t, pk, args = _device_args(ctx, data, table)
    lay = _layout(layout)
    cap = mcap_count_events(ctx, t, pk, lay) if capacity is None else int(capacity)
    if out is None:
        out = torch.empty(cap * 25 + 16, dtype=torch.uint8, device=t.device)
    info = McapInfo()
    o = mcap_options(**options)
    st = L.ecal_events_from_mcap_dev(ctx._h, *args, ctypes.byref(lay), ctypes.byref(o), out.data_ptr(), cap, ctypes.byref(info),
                                     torch.cuda.current_stream().cuda_stream)
    if st != 0:
        ctx._fail_with_info(st, info)
    return out[: int(info.n_events) * 25], info.as_dict()


def mcap_to_bin(ctx, mcap_path, bin_path, **options):
    """ecal_mcap_to_bin_file: the records of the .mcap file (file order, no sort) as a .bin of the reference's layout -> info dict."""
    library()
    return ctx._to_bin("ecal_mcap_to_bin_file", mcap_path, bin_path, mcap_options(**options), McapInfo())


def stream_from_mcap_file(ctx, path, **options):
    """ecal_stream_create_from_mcap_file, its records copied into a uint8 CUDA tensor (time order: the stream sorts when the file is
    not) -> (events, info dict, t_first, t_last)."""
    library()
    return ctx._stream_from_file("ecal_stream_create_from_mcap_file", path, mcap_options(**options), McapInfo())


# the same as methods of capi.Context
capi.Context.mcap_index_messages = mcap_index_messages
capi.Context.mcap_count_events = mcap_count_events
capi.Context.events_from_mcap = events_from_mcap
capi.Context.mcap_to_bin = mcap_to_bin
capi.Context.stream_from_mcap_file = stream_from_mcap_file
