"""CPU suite: include/ecal_mcap.h against the library and against mcap.PROTOTYPES, the table of that header — every function it
declares is exported by libecal.so and has an entry of the same arity, return type and argument widths; the ctypes structures have
the header's fields and the library's sizes; and ecal.h, which the new header includes and must not touch, still parses to what
tests/test_capi_prototypes.py expects (that module's own HEADER and its own checks, not a copied number)."""
import ctypes
import os
import re

import eventcalib_amd
from eventcalib_amd import capi, mcap

import test_capi_prototypes as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, "include", "ecal_mcap.h")).read()


def _header():
    """name -> (return type, [parameter text]) of every function include/ecal_mcap.h declares (test_capi_prototypes's parse)"""
    text = re.sub(r"/\*.*?\*/", " ", TEXT, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"(?m)^[ \t]*#[^\n]*$", ";", text)
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9\s\*]*?)\b(ecal_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", text):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), TP._split_top_level(m.group(3))
        if ret.startswith("typedef"):
            continue
        assert name not in out, "%s is declared twice" % name
        out[name] = (ret, [] if params in ([""], ["void"]) else params)
    return out


HEADER = _header()


def _struct_fields(name):
    """the member names of `typedef struct name { ... } name;` in declaration order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), TEXT, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.sub(r"\[.*?\]", "", first.split()[-1]).lstrip("*"))
        names += [re.sub(r"\[.*?\]", "", r.strip()).lstrip("*") for r in rest]
    return names


def test_every_declared_function_is_exported_and_in_the_table():
    assert len(HEADER) == 7 and set(HEADER) == set(mcap.PROTOTYPES)
    assert not set(HEADER) & set(TP.HEADER), "a symbol of ecal.h is declared again"
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    L = mcap.library()
    for name, (ret, params) in HEADER.items():
        assert hasattr(L, name), "%s is not exported by libecal.so" % name
        restype, argtypes = mcap.PROTOTYPES[name]
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        assert restype is TP.RESTYPES[ret], (name, ret)
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
        for k, (text, entry) in enumerate(zip(params, argtypes)):
            if "*" in text or re.search(r"\b(uint64_t|size_t|double)\b", text):
                assert entry not in TP.NARROW and ctypes.sizeof(entry) == 8, (name, k, text, entry)
            else:
                assert ctypes.sizeof(entry) == 4, (name, k, text, entry)


def test_the_structures_follow_the_header():
    for name, cls, size in (("ecal_mcap_options", mcap.McapOptions, 64), ("ecal_mcap_layout", mcap.McapLayout, 32),
                            ("ecal_mcap_info", mcap.McapInfo, 184), ("ecal_mcap_message", mcap.McapMessage, 24)):
        assert _struct_fields(name) == [n for n, _ in cls._fields_], name
        assert ctypes.sizeof(cls) == size, name
    assert mcap.MCAP_MESSAGE_DTYPE.itemsize == 24 and list(mcap.MCAP_MESSAGE_DTYPE.names) == [n for n, _ in mcap.McapMessage._fields_]
    for name, value in (("NONE", 0), ("STRUCT", 1), ("MONO", 2), ("EVT3", 3)):
        assert re.search(r"ECAL_MCAP_%s = %d\b" % (name, value), TEXT) and getattr(mcap, "MCAP_" + name) == value


def test_default_options_write_the_whole_structure_and_no_more():
    class Guarded(ctypes.Structure):
        _fields_ = [("o", mcap.McapOptions), ("guard", ctypes.c_uint8 * 64)]
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    g = Guarded()
    ctypes.memset(ctypes.byref(g), 0x5A, ctypes.sizeof(g))
    raw = ctypes.CDLL(capi.lib_path())      # (a handle of the test's own: the shared one keeps its struct-pointer prototype)
    raw.ecal_mcap_default_options.argtypes, raw.ecal_mcap_default_options.restype = [ctypes.c_void_p], None
    raw.ecal_mcap_default_options(ctypes.byref(g))
    assert bytes(g.guard) == b"\x5A" * 64 and g.o.auto_time_base == 1 and g.o.time_base == 0 and g.o.start_time == -float("inf")
    assert not g.o.topic and g.o.has_end_time == 0 and g.o.width == 0 and g.o.flip_x == 0 and g.o.flip_y == 0
    assert mcap.mcap_block_events() == 1024


def test_ecal_h_is_what_the_prototype_test_expects():
    TP.test_the_header_parse_is_whole()
    TP.test_table_header_and_export_list_name_the_same_symbols()
    TP.test_argument_counts_match_the_header()
    assert not set(mcap.PROTOTYPES) & set(capi.PROTOTYPES) and not set(mcap.PROTOTYPES) & set(capi.EXPORTED_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "ecal.h")).read()
    assert "#define ECAL_ABI_VERSION 3" in text and "ecal_mcap" not in text
    assert '#include "ecal.h"' in TEXT
    makefile = open(os.path.join(ROOT, "eventcalib_amd", "csrc", "Makefile")).read()
    assert "build/ecal_mcap.o" in makefile and makefile.count("include/ecal_mcap.h") == 2


def test_the_bag_ingest_still_refuses_an_mcap_file_by_name():
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    L = capi.load_library()
    n, info = ctypes.c_uint64(), capi.BagInfo()
    data = b"\x89MCAP0\r\n" + bytes(64)
    assert L.ecal_bag_index_messages(None, data, len(data), None, None, 0, ctypes.byref(n), ctypes.byref(info)) == -1
