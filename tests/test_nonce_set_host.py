"""The replay set's host-side rules (csrc/nonce_set.hpp: the keyed hash, the
probe step, the table-size and growth rules) on the host under ASan/UBSan.
tests/host/nonce_set_host.cpp checks the sizing rule over a grid (a power of
two, monotone, load <= 1/2 after a worst-case admit, <= 32 B per nonce above
the minimum), the keying, and a sequential model of the insert / resolve /
commit / rehash kernels, written with the header's own probe and hash
functions, against std::set semantics: the empty batch, one nonce, 257 equal
nonces, nonces equal in three of four words, a batch whose home slots are the
table's last two (the probe wraps), and a sequence that grows the table four
times.  The GPU runs the kernels themselves in tests/test_gpu_nonce_set.py."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "nonce_set_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_rules_and_sequential_model_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nonce_set_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checked = [ln for ln in r.stdout.splitlines() if ln.startswith("admits checked: ")]
    assert checked and int(checked[0].split(": ")[1]) >= 20
    assert r.stdout.rstrip().endswith("nonce_set_host: OK")
