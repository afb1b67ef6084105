"""The grouped fold's host-side rules (csrc/group_fold.hpp: the id check, the
launch plan of k_fold_grouped and limbs_to_elem, the exact recombination of
the kernel's integer word sums) on the host under ASan/UBSan.
tests/host/group_fold_host.cpp checks limbs_to_elem for both fields against
repeated F::add and against count * x for counts up to 2^31 - 1, check_groups
(sentinel, first bad index, counts with and without a mask), and the plan's
invariants over a grid of shapes.  The program includes csrc/field.hpp, which
needs the HIP headers, so hipcc compiles it and the sanitizers instrument its
host side; it is a stand-alone program, run on the CPU.  The GPU runs the
kernel itself in tests/test_gpu_aggregate_grouped.py."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "group_fold_host.cpp")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_limbs_ids_and_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "group_fold_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    cmd = ["hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g"]
    for flag in san:
        cmd += ["-Xarch_host", flag]
    subprocess.check_call(cmd + ["-o", exe, SRC] + san[:1])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    checked = [ln for ln in r.stdout.splitlines() if ln.startswith("plans checked: ")]
    assert checked and int(checked[0].split(": ")[1]) >= 3000
    assert r.stdout.rstrip().endswith("group_fold_host: OK")
