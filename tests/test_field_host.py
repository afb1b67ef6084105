"""csrc/field.hpp against Python integers, on the host.  The end-to-end
vectors never reach the rare branches of the two reductions (the final
conditional subtract of F64::reduce128: 2^-32 per product; F128::add with a
sum in [p, 2^128): 2^-59; the later fold iterations of F128::mul), so
tests/host/field_check.hip applies add, sub, mul, neg and finv to every
ordered pair of a grid of edge values (tests/field_grid.py) and this test
compares every line with plain integer arithmetic mod p.  The program is
built with UBSan, so undefined shifts or signed overflow in the __int128 code
abort it.

F128::mul's fold loop is unrolled five times.  The grid reaches every
iteration count from 0 to 4: 4 is the maximum (the high half shrinks from
< 2^128 to < 2^69, < 2^11, <= 1, 0), and pairs that need the fourth are
constructed from a * b mod p in [c, ~2^79) (field_grid._constructed); a fifth
iteration cannot happen."""
import os
import subprocess

import pytest

from conftest import ROOT
import field_grid as fg

SRC = os.path.join(ROOT, "tests", "host", "field_check.hip")
CSRC = os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd", "csrc")


@pytest.fixture(scope="module")
def field_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("field") / "field_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-I" + CSRC,
                           "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    return exe


def test_grid_reaches_the_rare_branches():
    counts = {}
    final_sub = 0
    v = fg.values(128)
    for a in v:
        for b in v:
            (n, r) = fg.f128_fold_count(a, b)
            counts[n] = counts.get(n, 0) + 1
            final_sub += r >= fg.P128
    print("F128::mul fold iterations -> pairs:", sorted(counts.items()), "final subtract:", final_sub)
    assert sorted(counts) == [0, 1, 2, 3, 4]
    assert final_sub > 0
    assert any(a + b >= fg.P128 and a + b < 2 ** 128 for a in v for b in v), "F128::add, sum in [p, 2^128)"
    assert any(a + b >= 2 ** 128 for a in v for b in v), "F128::add, carry out"
    v = fg.values(64)
    seen = [set(), set(), set()]
    for a in v:
        for b in v:
            for (s, x) in zip(seen, fg.f64_reduce_branches(a, b)):
                s.add(x)
    assert all(s == {False, True} for s in seen), "reduce128: borrow, carry and final subtract, taken and not"
    assert any(a + b >= 2 ** 64 for a in v for b in v) and any(fg.P64 <= a + b < 2 ** 64 for a in v for b in v)


@pytest.mark.parametrize("bits", [64, 128])
def test_field_hpp_matches_python_integers(field_check, bits):
    p = fg.P64 if bits == 64 else fg.P128
    vals = fg.values(bits)
    r = subprocess.run([field_check, str(bits)], input="".join("%x\n" % v for v in vals), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(vals) ** 2
    k = 0
    for a in vals:
        for b in vals:
            got = tuple(int(x, 16) for x in lines[k].split())
            assert got == (a, b) + fg.expected(p, a, b), "pair %#x %#x (add sub mul neg inv)" % (a, b)
            k += 1
