"""CPU-side checks of the grouped fold's boundary (no compute call without a
GPU): mastic_aggregate_grouped is declared in include/mastic_hip.h, exported
by the built library and bound by the ctypes layer; the change is additive
(the ABI version stays 8); the library holds the new kernel; the package
exports NO_GROUP and the metrics driver."""
import ctypes
import os
import re

from conftest import ROOT


def _lib_path():
    from mastic_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.LIB_PATH


def _header():
    return open(os.path.join(ROOT, "include", "mastic_hip.h")).read()


def test_symbol_in_header_library_and_binding():
    from mastic_amd import _lib
    text = _header()
    assert re.search(r"\bint mastic_aggregate_grouped\(mastic_ctx\* ctx, int agg_id, const uint32_t\* group, "
                     r"size_t n_groups,\s+const uint8_t\* valid, uint8_t\* agg_shares, uint64_t\* counts\);", text)
    assert re.search(r"#define MASTIC_GROUP_NONE 0xFFFFFFFFu\b", text)
    assert re.search(r"#define MASTIC_MAX_GROUPS 65536\b", text)
    assert "mastic_aggregate_grouped" in _lib.EXPORTS
    lib = ctypes.CDLL(_lib_path())
    assert hasattr(lib, "mastic_aggregate_grouped")


def test_abi_version_is_still_8():
    from mastic_amd import _lib
    lib = ctypes.CDLL(_lib_path())
    lib.mastic_abi_version.restype = ctypes.c_int
    assert lib.mastic_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert re.search(r"#define MASTIC_ABI_VERSION 8\b", _header())


def test_library_holds_the_grouped_fold_kernel():
    data = open(_lib_path(), "rb").read()
    assert b"k_fold_grouped" in data
    assert b"k_fold_shares" in data and b"k_foldI" in data  # the ungrouped fold and the chunk merge are still there


def test_null_ctx_is_refused_without_a_device():
    lib = ctypes.CDLL(_lib_path())
    lib.mastic_aggregate_grouped.restype = ctypes.c_int
    lib.mastic_aggregate_grouped.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.mastic_aggregate_grouped(None, 0, None, 1, None, None, None) == -22


def test_package_exports_no_group_and_metrics():
    import mastic_amd
    assert mastic_amd.NO_GROUP == 0xFFFFFFFF
    assert callable(mastic_amd.metrics.compute_attribute_metrics)
    assert callable(mastic_amd.Mastic.aggregate_grouped)


def test_group_fold_header_is_host_only():
    """csrc/group_fold.hpp holds the plan and the arithmetic and includes no
    HIP header (it compiles with a plain host compiler once a field type is
    given); the fold executor, csrc/fold.hpp, takes every decision from it."""
    text = open(os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd", "csrc", "group_fold.hpp")).read()
    code = re.sub(r"//.*", "", text)
    assert "#include <hip" not in code and '#include "' not in code
    for name in ("check_groups", "plan_group_fold", "limbs_to_elem"):
        assert re.search(r"\b%s\b" % name, code), name
    hip = open(os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd", "csrc", "fold.hpp")).read()
    assert "plan_group_fold(" in hip and "check_groups(" in hip and "plan_fold(" in hip
