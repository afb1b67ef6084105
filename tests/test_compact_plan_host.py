"""The plan of mastic_reports_compact (csrc/compact_plan.hpp, which
reports.hpp executes with k_gather_rows and device-to-device copies), on the
host under ASan/UBSan.  tests/host/compact_plan_host.cpp runs every plan on a
byte array with launch semantics, over random masks, all kept, none kept, only
the first dropped, only the last kept, alternating and a dropped run inside a
kept run, n up to 4099 and staging sizes from one row up, and checks that no
launch reads a row it or an earlier launch writes, that the result is the
reference filter, that the identity prefix is untouched and that staging rows
and launch count stay within their bounds.  The GPU side runs the same plans
in tests/test_gpu_reports_compact.py."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "compact_plan_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "compact_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checked = [ln for ln in r.stdout.splitlines() if ln.startswith("plans checked: ")]
    assert checked and int(checked[0].split(": ")[1]) >= 5000
    assert r.stdout.rstrip().endswith("compact_plan_host: OK")
