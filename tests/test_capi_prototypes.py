"""CPU suite: capi.PROTOTYPES, the one table of ctypes prototypes, against include/ecal.h — the same symbols, the same argument
counts, the return types, and no pointer or 64-bit argument declared as a 32-bit integer (the mistake that stays silent until an
address lies above 4 GiB); the table is what the loaded handle carries, and no function of the package sets a prototype of its own."""
import ast
import ctypes
import os
import re

import eventcalib_amd
from eventcalib_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESTYPES = {"int": ctypes.c_int, "void": None, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "double": ctypes.c_double, "const char *": ctypes.c_char_p}
NARROW = (ctypes.c_int, ctypes.c_uint, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int16, ctypes.c_uint16, ctypes.c_int8, ctypes.c_uint8,
          ctypes.c_bool, ctypes.c_char)


def _split_top_level(params):
    parts, depth, cur = [], 0, ""
    for ch in params:
        depth += ch == "("
        depth -= ch == ")"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return [" ".join(p.split()) for p in parts + [cur]]


def _header():
    """name -> (return type, [parameter text]) of every function include/ecal.h declares"""
    text = open(os.path.join(ROOT, "include", "ecal.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"(?m)^[ \t]*#[^\n]*$", ";", text)       # (a preprocessor line ends whatever stood before it)
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9\s\*]*?)\b(ecal_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", text):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), _split_top_level(m.group(3))
        if ret.startswith("typedef"):
            continue
        assert name not in out, "%s is declared twice" % name
        out[name] = (ret, [] if params in ([""], ["void"]) else params)
    return out


HEADER = _header()


def test_the_header_parse_is_whole():
    assert len(HEADER) == 194
    for name, (ret, params) in HEADER.items():
        assert ret in RESTYPES or ret.endswith("*"), (name, ret)
        assert all(p and "(" not in p for p in params), (name, params)     # (function pointers are typedefs, never inline)


def test_table_header_and_export_list_name_the_same_symbols():
    assert set(capi.PROTOTYPES) == set(HEADER) == set(capi.EXPORTED_SYMBOLS)
    assert len(capi.EXPORTED_SYMBOLS) == len(set(capi.EXPORTED_SYMBOLS))


def test_argument_counts_match_the_header():
    bad = [(name, len(capi.PROTOTYPES[name][1]), len(params)) for name, (_, params) in HEADER.items()
           if len(capi.PROTOTYPES[name][1]) != len(params)]
    assert not bad, bad


def test_return_types_match_the_header():
    for name, (ret, _) in HEADER.items():
        want = RESTYPES[ret] if ret in RESTYPES else ctypes.c_void_p
        assert capi.PROTOTYPES[name][0] is want, (name, ret, capi.PROTOTYPES[name][0])
    assert [n for n, (ret, _) in HEADER.items() if ret not in RESTYPES] == ["ecal_stream_data"]


def test_no_pointer_or_64_bit_argument_is_declared_narrow():
    """a pointer, uint64_t, size_t or double of the header never goes through as a 32-bit (or smaller) integer; a double is c_double"""
    checked = 0
    for name, (_, params) in HEADER.items():
        for k, (text, entry) in enumerate(zip(params, capi.PROTOTYPES[name][1])):
            if "*" in text or re.search(r"\b(uint64_t|size_t|double)\b", text):
                assert entry not in NARROW and ctypes.sizeof(entry) == 8, (name, k, text, entry)
                checked += 1
            if "*" not in text and re.search(r"\bdouble\b", text):
                assert entry is ctypes.c_double, (name, k, text, entry)
    assert checked > 500       # (the parse found its cases: most of the header's 1200 parameters are pointers or 64 bits wide)


def test_the_loaded_handle_carries_the_table():
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    L = eventcalib_amd.load_library()
    for name, (restype, argtypes) in capi.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype, name
        assert tuple(fn.argtypes) == tuple(argtypes), name
    for name, (restype, argtypes) in capi.DEBUG_PROTOTYPES.items():
        assert name.startswith("ecal_debug_") and name not in HEADER
        if hasattr(L, name):
            assert getattr(L, name).restype is restype and tuple(getattr(L, name).argtypes) == tuple(argtypes), name


def _prototype_assignments(path):
    """(function, line) of every assignment to an attribute named argtypes or restype inside a function of the file"""
    tree = ast.parse(open(path).read())
    hits = []

    def targets(node):
        if isinstance(node, ast.Assign):
            return node.targets
        if isinstance(node, (ast.AugAssign, ast.AnnAssign)):
            return [node.target]
        return []

    def flat(t):
        return [e for x in t.elts for e in flat(x)] if isinstance(t, (ast.Tuple, ast.List)) else [t]

    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            for node in ast.walk(fn):
                for t in targets(node):
                    hits += [(fn.name, node.lineno) for e in flat(t) if isinstance(e, ast.Attribute) and e.attr in ("argtypes", "restype")]
    return hits


def test_only_the_table_sets_prototypes_in_the_package():
    pkg = os.path.join(ROOT, "eventcalib_amd")
    hits = {f: _prototype_assignments(os.path.join(pkg, f)) for f in ("capi.py", "pipeline.py", "adaptive.py")}
    assert hits["pipeline.py"] == [] and hits["adaptive.py"] == []
    assert hits["capi.py"] and {fn for fn, _ in hits["capi.py"]} == {"_apply_prototypes"}, hits["capi.py"]
