"""csrc/field.hpp's device code against Python integers.  The product's
kernels are pinned only through end-to-end vectors, which never reach the rare
branches of the reductions; the gfx950 code generation of the __int128
arithmetic is compared here directly: tests/host/field_ops.hip (a test-only
library built by build()) applies add, sub, mul, neg and finv element-wise, one
launch per field, over every ordered pair of tests/field_grid.py's edge values
(the grid tests/test_field_host.py shows to reach every fold count and final
subtract) plus 4,096 random pairs."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import ROOT
import field_grid as fg
from test_gpu_parity import mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "host", "_build", "libfield_ops.so")


@pytest.mark.parametrize("bits", [64, 128])
def test_device_field_ops_match_python_integers(mastic_amd, bits):  # noqa: F811
    if not os.path.exists(LIB):
        pytest.fail("libfield_ops.so missing: build() was not run")
    lib = ctypes.CDLL(LIB)
    lib.field_ops_run.restype = ctypes.c_int
    lib.field_ops_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    p = fg.P64 if bits == 64 else fg.P128
    vals = fg.values(bits)
    rng = random.Random(4096 + bits)
    pairs = [(a, b) for a in vals for b in vals] + [(rng.randrange(p), rng.randrange(p)) for _ in range(4096)]
    n, w = len(pairs), bits // 64

    def pack(xs):
        return np.frombuffer(b"".join(x.to_bytes(8 * w, "little") for x in xs), np.uint64).copy()
    (a, b) = (pack([x for (x, _) in pairs]), pack([y for (_, y) in pairs]))
    out = np.zeros(5 * n * w, np.uint64)
    rc = lib.field_ops_run(bits, a.ctypes.data, b.ctypes.data, out.ctypes.data, n)
    assert rc == 0, "hip error %d" % rc
    raw = out.tobytes()
    esz = 8 * w
    got = [[int.from_bytes(raw[(k * n + i) * esz:(k * n + i + 1) * esz], "little") for i in range(n)] for k in range(5)]
    names = ["add", "sub", "mul", "neg", "inv"]
    for (i, (x, y)) in enumerate(pairs):
        want = fg.expected(p, x, y)
        for k in range(5):
            assert got[k][i] == want[k], "%s(%#x, %#x) = %#x, want %#x" % (names[k], x, y, got[k][i], want[k])
        if x:
            assert x * got[4][i] % p == 1
