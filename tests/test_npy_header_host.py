"""CPU: ecal_npy_parse_header (host only, no context) on files that numpy itself writes in tmp_path: the structured layouts of 13, 14
and 16 bytes (align=True with its '|V3' entry), an (N, 4) f64 array, headers of versions 1 and 2, names by alias and by option — the
layout must address exactly the bytes numpy addresses, checked by running the host walk over the file's bytes through the layout
against the oracle on the arrays — and every refusal by its text."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fields_oracle as FO  # noqa: E402

LAYOUTS = {
    "packed13": np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")]),
    "packed14": np.dtype([("ts", "<i8"), ("X", "<u2"), ("Y", "<u2"), ("pol", "<i2")]),
    "aligned16": np.dtype([("timestamp", "<i8"), ("x", "<u2"), ("y", "<u2"), ("polarity", "?")], align=True),
    "seconds": np.dtype([("Time", "<f8"), ("x", "<f4"), ("y", "<f4"), ("P", "i1"), ("extra", "<c16"), ("tag", "S3")]),
}


@pytest.fixture(scope="module")
def capi():
    import eventcalib_amd
    if not os.path.exists(eventcalib_amd.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    from eventcalib_amd import capi
    return capi


def _structured(dt, n=257, seed=1):
    rng = np.random.default_rng(seed)
    names = [k for k in dt.names if k not in ("extra", "tag")]
    cols = FO.random_columns(rng, n, **{k: dt[name] for k, name in zip("txyp", names)})
    arr = np.zeros(n, dt)
    for name, c in zip(names, cols):
        arr[name] = c
    return arr, cols


def _walk_through_layout(capi, data, lay, **options):
    """the host walk over the file's own bytes with the fields the layout gives"""
    raw = np.frombuffer(data, np.uint8)
    cols = []
    for k in "txyp":
        off, tname = lay["fields"][k]
        dt = np.dtype(capi.FIELD_DTYPES[capi.FIELD_TYPE_NAMES.index(tname)])
        start = lay["data_offset"] + off
        cols.append(np.ndarray(shape=(lay["n_events"],), dtype=dt, buffer=raw, offset=start, strides=(lay["item_stride"],)))
    return capi.events_from_fields_host(*cols, **options)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_structured_files_as_numpy_writes_them(capi, tmp_path, name):
    dt = LAYOUTS[name]
    arr, cols = _structured(dt)
    path = tmp_path / (name + ".npy")
    np.save(path, arr)
    data = path.read_bytes()
    if name == "aligned16":
        assert b"'|V3'" in data[:256] and dt.itemsize == 16
    lay = capi.npy_parse_header(data)
    assert lay["n_events"] == arr.size and lay["item_stride"] == dt.itemsize and lay["version_major"] == 1
    assert lay["data_offset"] == len(data) - arr.nbytes
    got, info = _walk_through_layout(capi, data, lay)
    want, counts = FO.from_fields(*cols, time_magnitude=FO.default_magnitude(cols[0]))
    assert got.tobytes() == want.tobytes() and info["n_events"] == counts["n_events"] == arr.size
    # the header alone, with the file's size beside it
    assert capi.npy_parse_header(data[: lay["data_offset"]], file_bytes=len(data)) == lay
    with pytest.raises(capi.EcalError) as e:
        capi.npy_parse_header(data[:-1])
    assert e.value.status == -1 and "%d bytes there, %d needed" % (arr.nbytes - 1, arr.nbytes) in str(e.value)


def test_a_plain_n_by_4_array_and_its_columns(capi, tmp_path):
    rng = np.random.default_rng(3)
    t, x, y, p = FO.random_columns(rng, 100, t=np.float64, x=np.float64, y=np.float64, p=np.float64)
    for dt in (np.float64, np.float32, np.int64, np.int32, np.uint32):
        ticks = (t * 1e6).round()
        a = np.stack([t if np.dtype(dt).kind == "f" else ticks, np.floor(x), np.floor(y), p], axis=1).astype(dt)
        path = tmp_path / "plain.npy"
        np.save(path, a)
        data = path.read_bytes()
        lay = capi.npy_parse_header(data)
        size = np.dtype(dt).itemsize
        assert lay["item_stride"] == 4 * size and lay["n_events"] == 100
        assert [lay["fields"][k][0] for k in "txyp"] == [0, size, 2 * size, 3 * size]
        got, _ = _walk_through_layout(capi, data, lay)
        want, _ = FO.from_fields(a[:, 0], a[:, 1], a[:, 2], a[:, 3], time_magnitude=FO.default_magnitude(a[:, 0]))
        assert got.tobytes() == want.tobytes()
        np.save(path, np.ascontiguousarray(a[:, [1, 2, 0, 3]]))
        lay = capi.npy_parse_header(path.read_bytes(), columns="xytp")
        got2, _ = _walk_through_layout(capi, path.read_bytes(), lay)
        assert got2.tobytes() == want.tobytes()


def test_headers_of_versions_1_and_2_and_3(capi, tmp_path):
    arr, _ = _structured(LAYOUTS["packed13"], n=10)
    for version in ((1, 0), (2, 0), (3, 0)):
        path = tmp_path / "v.npy"
        with open(path, "wb") as f:
            np.lib.format.write_array(f, arr, version=version)
        data = path.read_bytes()
        assert data[6] == version[0]
        lay = capi.npy_parse_header(data)
        assert (lay["version_major"], lay["version_minor"]) == version
        assert lay["data_offset"] == len(data) - arr.nbytes and lay["item_stride"] == 13
        assert np.array_equal(np.load(path), arr)


def test_names_by_option(capi, tmp_path):
    dt = np.dtype([("t", "<f8"), ("stamp_us", "<i8"), ("col", "<u2"), ("row", "<u2"), ("x", "<f4"), ("on", "?")])
    path = tmp_path / "named.npy"
    np.save(path, np.zeros(4, dt))
    data = path.read_bytes()
    with pytest.raises(capi.EcalError) as e:
        capi.npy_parse_header(data)
    assert "missing field y" in str(e.value)
    lay = capi.npy_parse_header(data, fields={"t": "stamp_us", "x": "col", "y": "row", "p": "on"})
    assert lay["fields"] == {"t": (8, "I64"), "x": (16, "U16"), "y": (18, "U16"), "p": (24, "U8")} and lay["item_stride"] == 25


def _save(tmp_path, a):
    path = tmp_path / "r.npy"
    np.save(path, a)
    return path.read_bytes()


def test_every_refusal_by_its_text(capi, tmp_path):
    def refused(data, text, **kw):
        with pytest.raises(capi.EcalError) as e:
            capi.npy_parse_header(data, **kw)
        assert e.value.status == -1 and text in str(e.value), str(e.value)

    good = LAYOUTS["packed13"]
    refused(_save(tmp_path, np.zeros(3, good.newbyteorder(">"))), "big-endian")
    refused(_save(tmp_path, np.zeros((3, 4), ">f8")), "big-endian")
    refused(_save(tmp_path, np.zeros(3, [("t", "<i8"), ("x", "<u2", (2,)), ("y", "<u2"), ("p", "u1")])), "sub-array")
    refused(_save(tmp_path, np.zeros(3, [("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "O")])), "object dtype")
    refused(_save(tmp_path, np.asfortranarray(np.zeros((3, 4)))), "fortran_order: True on 2-D data")
    refused(_save(tmp_path, np.zeros(3, [("t", "<i8"), ("x", "<u2"), ("p", "u1")])), "missing field y")
    refused(_save(tmp_path, np.zeros(3, [("t", "<i8"), ("time", "<i8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")])), "duplicate field for t")
    refused(_save(tmp_path, np.zeros(3, [("t", "<u2"), ("x", "<u2"), ("y", "<u2"), ("p", "u1")])), "which field t does not take")
    refused(_save(tmp_path, np.zeros(3, [("t", "<i8"), ("x", "<f2"), ("y", "<u2"), ("p", "u1")])), "which field x does not take")
    refused(_save(tmp_path, np.zeros((3, 4), "<u2")), "hold a stamp column")
    refused(_save(tmp_path, np.zeros((3, 5))), "(N, 4) is read")
    refused(_save(tmp_path, np.zeros(12)), "(N, 4) is read")
    refused(_save(tmp_path, np.zeros((3, 2), good)), "2 dimensions")
    refused(_save(tmp_path, np.zeros((3, 4))), "each once", columns="ttxy")
    refused(b"PK\x03\x04" + bytes(100), "not a .npy file")
    refused(b"", "not a .npy file")
    data = _save(tmp_path, np.zeros(3, good))
    refused(data[:40], "cut short")
    refused(data[:6] + b"\x04" + data[7:], "version 4.0")
    refused(data[:-5], "34 bytes there, 39 needed")
    # a fortran-ordered 1-D structured array is the same bytes: taken
    assert capi.npy_parse_header(data.replace(b"'fortran_order': False", b"'fortran_order': True ")) == capi.npy_parse_header(data)
