"""csrc/rows_kernels.hpp's k_gather_rows alone (tests/host/rows_ops.hip, a
test-only library built by build()), out of place, against numpy's take.

Source rows and the destination range are embedded in random canary bytes and
start at byte offsets that take every residue mod 16 (destination) and mod 4
(source) over the grid, so source and destination alignment differ from row to
row and from case to case.  After a launch the whole destination buffer is
compared: the bytes before the first row, after the last one and every row
beyond ``count`` must be bit-identical, which is what a 16-byte or 4-byte
read-modify-write at a row's ends, or any overrun, would break (the
neighbouring rows are written by other lanes of the same launch).

Row sizes: 1 (wire flags), 16 (nonces), the sizes around the 16-byte slot and
the 64-lane wave, odd public-share sizes (65, 121, 193, 579), and rows wider
than a workgroup's 4 KiB (4099) and than many workgroups (65539).  Row counts
1, 2, 65 and 1000 cover one lane, several rows per wave, and more than one
workgroup at every row size.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "host", "_build", "librows_ops.so")
ROW_BYTES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65, 121, 193, 255, 256, 257, 579, 4099, 65539]
PAD = 64  # canary bytes around the rows, besides the byte offset


@pytest.fixture(scope="module")
def rows_ops():
    if not os.path.exists(LIB):
        pytest.fail("librows_ops.so missing: build() was not run")
    lib = ctypes.CDLL(LIB)
    (sz, P) = (ctypes.c_size_t, ctypes.c_void_p)
    lib.rows_ops_gather.restype = ctypes.c_int
    lib.rows_ops_gather.argtypes = [P, sz, sz, P, sz, sz, sz, P, sz, sz, sz]
    return lib


def _counts(rb):
    if rb == 65539:
        return [1, 2, 17]
    if rb == 4099:
        return [1, 2, 65]
    return [1, 2, 65, 1000]


def _patterns(count, rng):
    """(name, number of source rows, idx of the count gathered rows)"""
    yield ("shift by one", count + 1, np.arange(1, count + 1))
    yield ("every other row", 2 * count, np.arange(0, 2 * count, 2))
    yield ("random ascending", 3 * count, np.sort(rng.choice(3 * count, size=count, replace=False)))
    yield ("last row only", count, np.array([count - 1]))


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("rb", ROW_BYTES)
def test_gather_rows_writes_its_rows_and_nothing_else(rows_ops, rb):
    rng = np.random.default_rng(1000 + rb)
    case = 0
    for count_ in _counts(rb):
        for (name, n_src, sel) in _patterns(count_, rng):
            count = len(sel)
            # every destination residue mod 16 and source residue mod 4 comes up over the grid
            dst_off = PAD + (case * 5 + rb) % 16
            src_off = PAD + (case * 3 + 1) % 16
            first = case % 4
            case += 1
            extra = 2  # destination rows beyond `count`, which must stay as they were
            src = rng.integers(0, 256, size=src_off + n_src * rb + PAD, dtype=np.uint8)
            dst = rng.integers(0, 256, size=dst_off + (count + extra) * rb + PAD, dtype=np.uint8)
            idx = np.concatenate([np.full(first, 0xFFFFFFF0, np.uint32), sel.astype(np.uint32),
                                  np.full(2, 0xFFFFFFF0, np.uint32)])  # entries outside the range are never read
            want = dst.copy()
            rows = src[src_off:src_off + n_src * rb].reshape(n_src, rb)
            want[dst_off:dst_off + count * rb] = np.take(rows, sel, axis=0).reshape(-1)
            rc = rows_ops.rows_ops_gather(_ptr(src), src.size, src_off, _ptr(dst), dst.size, dst_off, rb,
                                          _ptr(idx), idx.size, first, count)
            assert rc == 0, (rb, count, name, rc)
            what = (rb, count, name, dst_off % 16, src_off % 4)
            assert np.array_equal(dst[:dst_off], want[:dst_off]), ("bytes before the first row changed", what)
            assert np.array_equal(dst[dst_off + count * rb:], want[dst_off + count * rb:]), \
                ("bytes after the last row changed", what)
            got = dst[dst_off:dst_off + count * rb].reshape(count, rb)
            exp = want[dst_off:dst_off + count * rb].reshape(count, rb)
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert bad.size == 0, ("rows differ from take", what, bad[:8])


def test_harness_refuses_a_launch_that_would_leave_its_buffers(rows_ops):
    src = np.zeros(PAD + 4 * 8, np.uint8)
    dst = np.zeros(PAD + 4 * 8, np.uint8)
    idx = np.array([0, 1, 2, 4], np.uint32)  # row 4 of a 4-row source
    assert rows_ops.rows_ops_gather(_ptr(src), src.size, PAD, _ptr(dst), dst.size, PAD, 8, _ptr(idx), 4, 0, 4) == -1
    assert rows_ops.rows_ops_gather(_ptr(src), src.size, PAD, _ptr(dst), dst.size, PAD + 1, 8, _ptr(idx), 4, 0, 3) == 0
    assert rows_ops.rows_ops_gather(_ptr(src), src.size, PAD, _ptr(dst), dst.size, PAD + 1, 8, _ptr(idx), 3, 0, 4) == -1
