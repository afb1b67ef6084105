"""Probe (GPU box): the time of one replay-set admit over a resident batch,
beside what a caller had to do before the set existed: download the nonces
and walk them through a Python ``set``.

After one warm-up, the median of 5 runs of
  * admit_reports of 12,288 nonces (one C2 step's slice) into an empty set,
  * admit_reports of 1M nonces into an empty set,
  * admit_reports of 1M nonces into a set holding 16M,
each with the set sized up front (``capacity``) and, for the empty sets, also
left to grow from the minimum (the allocations and rehashes are then in the
time).  Every device mask is checked against the host path's.

  python3 tools/nonce_set_probe.py [--base 16777216] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd"))
import torch  # noqa: E402,F401  (one HIP runtime, see tests/conftest.py)
from mastic_amd import MasticCount, NonceSet, _lib  # noqa: E402
from mastic_amd.vdaf import Reports, _check  # noqa: E402

RUNS = 5


def resident(m, nonces: bytes):
    rep = Reports(m, len(nonces) // 16)
    rep.upload(nonces, None)
    return rep


def download_nonces(m, rep) -> bytes:
    """The nonces only (Reports.download() would also fetch the shares)."""
    out = np.empty(16 * rep.n, np.uint8)
    _check(m._ctx, _lib.lib().mastic_reports_download(rep._ptr, _lib.buf(out), None, None, None))
    return out.tobytes()


def host_admit(seen: set, data: bytes):
    fresh = bytearray(len(data) // 16)
    for i in range(len(fresh)):
        x = data[16 * i:16 * i + 16]
        if x not in seen:
            seen.add(x)
            fresh[i] = 1
    return fresh


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0, r)


def batch(n, dup_every=16):
    """n nonces, one in dup_every a copy of an earlier one of the batch."""
    a = np.frombuffer(os.urandom(16 * n), np.uint8).reshape(n, 16).copy()
    idx = np.arange(dup_every, n, dup_every)
    a[idx] = a[idx - dup_every // 2 - 1]
    return a.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", type=int, default=1 << 24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m = MasticCount(8)
    lines = ["replay set admit vs download + Python set (median of %d after one warm-up; seconds)" % RUNS,
             "host clock around each blocking call, fresh mask copied back; 'dev grow': a set left to grow from",
             "the minimum; host: mastic_reports_download of the nonces only, then a Python set walked in index order",
             "%-44s %10s %10s %10s %8s" % ("case", "device", "dev grow", "host", "host/dev")]

    def case(name, n, base_dev, base_host):
        """base_dev: None (empty sets) or a set sized for base + (RUNS + 1) batches."""
        dev_t, grow_t, host_t = [], [], []
        for run in range(RUNS + 1):
            data = batch(n)
            rep = resident(m, data)
            m.synchronize()
            ns = base_dev if base_dev is not None else NonceSet(m, capacity=n)
            (td, fresh) = timed(lambda: ns.admit(rep))
            if base_dev is None:
                small = NonceSet(m)
                (tg, fresh_g) = timed(lambda: small.admit(rep))
                assert fresh_g.tolist() == fresh.tolist()
            else:
                tg = float("nan")
            seen = base_host if base_host is not None else set()
            (th, want) = timed(lambda: host_admit(seen, download_nonces(m, rep)))
            assert bytes(want) == fresh.tobytes(), "device and host masks differ"
            if run:  # run 0 is the warm-up
                dev_t.append(td), grow_t.append(tg), host_t.append(th)
        d, g, h = statistics.median(dev_t), statistics.median(grow_t), statistics.median(host_t)
        lines.append("%-44s %10.5f %10.5f %10.5f %8.1f" % (name, d, g, h, h / d))
        print(lines[-1], flush=True)

    case("12,288 into an empty set", 12288, None, None)
    case("1,048,576 into an empty set", 1 << 20, None, None)
    base = os.urandom(16 * args.base)
    big = NonceSet(m, capacity=args.base + (RUNS + 1) * (1 << 20))
    (tb, _f) = timed(lambda: big.admit(base))
    lines.append("(building the %d-nonce set from host nonces, one admit: %.3f s)" % (args.base, tb))
    host_base = set(base[i:i + 16] for i in range(0, len(base), 16))
    case("1,048,576 into a set holding %d" % args.base, 1 << 20, big, host_base)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
