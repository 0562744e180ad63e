"""eventcalib_amd — MI355X-native (gfx950) implementation of the EventCalib hot path.

The product is the C-ABI library ``libecal.so`` (see ``include/ecal.h``); this package is a thin
ctypes binding used by the tests and ``bench.py``.  There is no CPU fallback: importing
``eventcalib_amd.capi`` and calling into it without the built library raises.
"""
from .capi import Context, EcalError, lib_path, load_library  # noqa: F401
from . import uncertainty  # noqa: F401  (attaches Solver.uncertainty / chunk_scores / chunk_table; sets no prototype until used)
from . import mcap  # noqa: F401  (attaches Context.events_from_mcap / mcap_to_bin / stream_from_mcap_file; sets no prototype until used)

__all__ = ["Context", "EcalError", "lib_path", "load_library"]
