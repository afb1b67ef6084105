"""The memory plan of a prep_init (csrc/memplan.hpp: the frontier cache's hit
test and commit, the spare slot's growth rule, and the chunking that
prep.hpp mastic_prep_init executes), on the host under ASan/UBSan.
tests/host/memplan_host.cpp checks that the functions return what the text of
mastic_prep_init returned before it moved there, over a grid of batch sizes,
per-report layouts, paddings, arena states, free-memory figures, explicit
budgets (the GPU tests' among them), chunk caps, pipelining, cache on / off and
allocation outcomes, and that every plan's chunks are multiples of 64 that fit
the arena (or its half), cover the batch exactly and respect the budget.  The
GPU side runs the same plans in tests/test_gpu_parity.py (budgeted cases),
tests/test_gpu_frontier_cache.py and tests/test_gpu_alloc_recovery.py."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "memplan_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_recorded_values_and_plan_invariants_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "memplan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checked = [ln for ln in r.stdout.splitlines() if ln.startswith("chunk cases checked: ")]
    assert checked and int(checked[0].split(": ")[1]) >= 80000
    assert r.stdout.rstrip().endswith("memplan_host: OK")
