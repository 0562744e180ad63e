"""CPU suite: include/ecal_uncertainty.h against the library and against uncertainty.PROTOTYPES, the table of that header — every
function it declares is exported by libecal.so and has an entry of the same arity, return type and argument widths; and ecal.h, which
the new header includes and must not touch, still parses to what tests/test_capi_prototypes.py expects (that module's own HEADER and
its own checks, not a copied number)."""
import ctypes
import os
import re

import eventcalib_amd
from eventcalib_amd import capi, uncertainty

import test_capi_prototypes as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """name -> (return type, [parameter text]) of every function include/ecal_uncertainty.h declares (test_capi_prototypes's parse)"""
    text = open(os.path.join(ROOT, "include", "ecal_uncertainty.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
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


def test_every_declared_function_is_exported_and_in_the_table():
    assert len(HEADER) == 7 and set(HEADER) == set(uncertainty.PROTOTYPES)
    assert not set(HEADER) & set(TP.HEADER), "a symbol of ecal.h is declared again"
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    L = uncertainty.library()
    for name, (ret, params) in HEADER.items():
        assert hasattr(L, name), "%s is not exported by libecal.so" % name
        restype, argtypes = uncertainty.PROTOTYPES[name]
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        assert restype is TP.RESTYPES[ret], (name, ret)
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
        for k, (text, entry) in enumerate(zip(params, argtypes)):
            if "*" in text or re.search(r"\b(uint64_t|size_t|double)\b", text):
                assert entry not in TP.NARROW and ctypes.sizeof(entry) == 8, (name, k, text, entry)
            else:
                assert ctypes.sizeof(entry) == 4, (name, k, text, entry)


def test_the_structures_have_the_header_sizes():
    assert ctypes.sizeof(uncertainty.UncertaintyOptions) == 8
    assert ctypes.sizeof(uncertainty.UncertaintyResult) == 8 + 8 * 4 + 2 * 8 + (3 * 81 + 3 * 9) * 8


def test_ecal_h_is_what_the_prototype_test_expects():
    TP.test_the_header_parse_is_whole()
    TP.test_table_header_and_export_list_name_the_same_symbols()
    TP.test_argument_counts_match_the_header()
    assert not set(uncertainty.PROTOTYPES) & set(capi.PROTOTYPES) and not set(uncertainty.PROTOTYPES) & set(capi.EXPORTED_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "ecal.h")).read()
    assert "#define ECAL_ABI_VERSION 3" in text and "uncertainty" not in text
    assert '#include "ecal.h"' in open(os.path.join(ROOT, "include", "ecal_uncertainty.h")).read()
