"""CPU-side checks of the frontier cache's node-format entry point at the
drop-in boundary (ABI 8, no compute calls): the header declares
mastic_set_frontier_cache_nodes and its three mode constants, the binding and
the built library export it, and the header, the binding and the integration
stub agree on the ABI version."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mastic_hip.h")


def _lib_path():
    from mastic_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.LIB_PATH


def test_header_declares_the_entry_point_and_modes():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+mastic_set_frontier_cache_nodes\s*\(\s*mastic_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*,"
                     r"\s*int\s*\*\s*last_in\s*,\s*int\s*\*\s*last_out\s*\)\s*;", text)
    for (name, value) in (("SEEDS", 0), ("PAYLOADS", 1), ("AUTO", 2)):
        assert re.search(r"#define MASTIC_FC_NODES_%s %d\b" % (name, value), text), name


def test_binding_and_library_export_the_entry_point():
    from mastic_amd import _lib, vdaf
    assert "mastic_set_frontier_cache_nodes" in _lib.EXPORTS
    lib = ctypes.CDLL(_lib_path())
    assert hasattr(lib, "mastic_set_frontier_cache_nodes")
    # the Python mirror names the modes in the header's order
    assert vdaf.Mastic.CACHE_NODES == ("seeds", "payloads", "auto")
    # a null ctx is refused before anything touches a device
    lib.mastic_set_frontier_cache_nodes.restype = ctypes.c_int
    lib.mastic_set_frontier_cache_nodes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.mastic_set_frontier_cache_nodes(None, -1, None, None) == -22


def test_abi_version_is_8_everywhere():
    from mastic_amd import _lib
    assert _lib.ABI_VERSION == 8
    assert re.search(r"#define MASTIC_ABI_VERSION 8\b", open(HEADER).read())
    stub = open(os.path.join(ROOT, "integration", "poc", "mastic_hip.py")).read()
    assert re.search(r"^ABI_VERSION = 8\b", stub, re.M)
    lib = ctypes.CDLL(_lib_path())
    lib.mastic_abi_version.restype = ctypes.c_int
    assert lib.mastic_abi_version() == 8
