"""The replay set at the drop-in boundary (no GPU): its seven entry points are
declared in include/mastic_hip.h, exported by the built library and listed in
the ctypes binding, and adding them left the ABI version at 8 (nothing that
existed changed its signature)."""
import ctypes
import os
import re

from conftest import ROOT

SYMBOLS = ["mastic_nonce_set_create", "mastic_nonce_set_destroy", "mastic_nonce_set_count",
           "mastic_nonce_set_admit", "mastic_nonce_set_admit_reports", "mastic_nonce_set_contains",
           "mastic_nonce_set_export"]


def _lib_path():
    from mastic_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.LIB_PATH


def test_symbols_in_header_library_and_binding():
    from mastic_amd import _lib
    text = open(os.path.join(ROOT, "include", "mastic_hip.h")).read()
    declared = set(re.findall(r"\b(mastic_nonce_set_[a-z_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    lib = ctypes.CDLL(_lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    bound = _lib.lib()
    assert bound.mastic_nonce_set_count.restype is ctypes.c_size_t
    assert bound.mastic_nonce_set_count(None) == 0
    # a NULL set is an argument error, not a crash
    assert bound.mastic_nonce_set_admit(None, None, 0, None, None) == -22
    assert bound.mastic_nonce_set_contains(None, None, 0, None) == -22
    assert bound.mastic_nonce_set_export(None, None, 0, None) == -22


def test_library_holds_the_kernels_and_abi_is_still_8():
    data = open(_lib_path(), "rb").read()
    for kernel in (b"k_ns_insert", b"k_ns_resolve", b"k_ns_commit", b"k_ns_rehash"):
        assert kernel in data, kernel
    lib = ctypes.CDLL(_lib_path())
    lib.mastic_abi_version.restype = ctypes.c_int
    assert lib.mastic_abi_version() == 8
    text = open(os.path.join(ROOT, "include", "mastic_hip.h")).read()
    assert re.search(r"#define MASTIC_ABI_VERSION 8\b", text)


def test_package_exports_nonce_set():
    import mastic_amd
    assert mastic_amd.NonceSet is mastic_amd.nonce_set.NonceSet
    for method in ("admit", "contains", "export", "load", "__len__"):
        assert callable(getattr(mastic_amd.NonceSet, method))
