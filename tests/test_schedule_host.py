"""The launch plan of a prep_init chunk (csrc/schedule.hpp: the level-geometry
helpers and plan_chunk, which prep.hpp struct Chunk executes), on the host
under ASan/UBSan.  tests/host/schedule_host.cpp checks that the helpers return
the values recorded before they moved out of mastic_hip.hip, and that every
plan over a grid of tree depths and widths, both fields, hit / miss, cache
on / off, pipelined or not, and every SchedKnobs field that changes a plan
(forced segments, split sponges, fuse_proofs, absorb_mode, seg_balance)
covers each level, node proof and sponge byte exactly once, in an order that
its streams and waits enforce, with legal kernel variants and the event
counts it declares.  The GPU side runs the same plans in the prep_init tests
(tests/test_gpu_last_level_segments.py counts its launches)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "schedule_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_helpers_and_plan_invariants_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "schedule_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checked = [ln for ln in r.stdout.splitlines() if ln.startswith("plans checked: ")]
    assert checked and int(checked[0].split(": ")[1]) >= 10000
    assert r.stdout.rstrip().endswith("schedule_host: OK")
