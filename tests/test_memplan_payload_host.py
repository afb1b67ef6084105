"""The frontier cache's node formats in the memory plan (csrc/memplan.hpp:
the node width a cached level records, slot capacity in words, and the rule by
which ``auto`` chooses payloads-format nodes), on the host under ASan/UBSan.
tests/host/memplan_payload_host.cpp checks that a cached level of either width
hits, that a payload-width slot holds a wider seeds-format level without
growing, that spare_capacity's defaulted width is the rule it was, the policy
at DESIGN.md §7's two anchors (1M reports on one GPU: seeds; 125k reports per
rank: payloads) and its monotonicity and fit over a grid.  The GPU side runs
the same decisions in tests/test_gpu_cache_payloads.py."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "memplan_payload_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_node_formats_and_auto_policy_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "memplan_payload_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checked = [ln for ln in r.stdout.splitlines() if ln.startswith("policy cases checked: ")]
    # 4 value widths x 3 held sizes x 6 batch sizes x 6 node counts x 7 free sizes
    assert checked and int(checked[0].split(": ")[1]) == 4 * 3 * 6 * 6 * 7
    assert r.stdout.rstrip().endswith("memplan_payload_host: OK")
