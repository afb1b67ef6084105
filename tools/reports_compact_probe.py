"""Timing of mastic_reports_compact (Reports.compact) on one MI355X.

copy    the blocking call's host time, median of 5 (after one warm-up), for
        1M C2-shaped reports keeping a random 50 %, 99 % and 1 %, and 16,384
        C5-shaped reports keeping 50 %, at staging sizes of 16, 64 and 256 MiB
        (C2) or the default (C5), against the yardstick: one device-to-device
        copy (torch's copy_ of a byte tensor, a hipMemcpyAsync) of the same
        number of moved bytes in the same process.  Only the nonces are
        uploaded (their first four bytes number the rows, and the survivors'
        numbers are checked after every call); the other segments hold
        whatever the allocation held, which a copy's rate does not depend on.
        The plan's bytes and launches are counted on the host by the model
        below (compact_plan.hpp's rule, restated).
sweep   one C2 heavy-hitters sweep (tools/sweep_probe.py's population) over
        131,072 reports of which half are replays of the other half, with a
        NonceSet, frontier cache on: `sweep none` is the sweep without
        compaction, `sweep 0.25` compacts.  Prints the HIP-event time of the
        prep_inits of the levels after 0 and the wall time.  Run it in fresh
        processes, alternating the two.

GPU box only:  python3 tools/reports_compact_probe.py copy [c2|c5]
               python3 tools/reports_compact_probe.py sweep none|<t> [n_reports]
"""
import os
import statistics
import sys
import time

import numpy as np
import torch  # first: the library then binds the HIP runtime torch loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd")]

from mastic_amd import Mastic, NonceSet  # noqa: E402
from mastic_amd.heavy_hitters import compute_heavy_hitters  # noqa: E402
from mastic_amd.vdaf import Reports  # noqa: E402

MIB = 1 << 20
DEFAULT_STAGING = 64 * MIB  # csrc/compact_plan.hpp CompactKnobs::default_staging_bytes


def plan_model(keep, row_sizes, staging_bytes):
    """(moved rows, bytes read + written, launches) of the plan, per the rule of
    csrc/compact_plan.hpp: direct where 2 * gap >= staging rows, else staged."""
    src = np.nonzero(keep)[0]
    n_kept = len(src)
    gap = src - np.arange(n_kept)
    prefix = int(np.searchsorted(gap, 1))
    moved = n_kept - prefix
    widest = max(row_sizes)
    sb = min(max(staging_bytes or DEFAULT_STAGING, widest), widest * max(1, moved))
    traffic = launches = 0
    for rb in row_sizes:
        S = max(1, sb // rb)
        a = prefix
        while a < n_kept:
            g = int(gap[a])
            if 2 * g >= S:
                cnt = min(g, n_kept - a)
                traffic += 2 * cnt * rb
                launches += 1
            else:
                cnt = min(S, n_kept - a)
                traffic += 4 * cnt * rb
                launches += 2
            a += cnt
    return (moved, traffic, launches)


def d2d_yardstick(nbytes, reps=5):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst.copy_(src)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    del src, dst
    torch.cuda.empty_cache()
    return ts


def copy_case(m, n, keep, staging, label):
    sizes = [16, m.sizes.public_share_size, m.sizes.input_share_size[0], m.sizes.input_share_size[1], 1]
    nonces = np.zeros((n, 4), "<u4")
    nonces[:, 0] = np.arange(n)
    in0 = np.zeros(n * sizes[2], np.uint8)
    in1 = np.zeros(n * sizes[3], np.uint8)
    want = np.nonzero(keep)[0]
    ts = []
    for it in range(6):  # the first is the warm-up
        rep = Reports(m, n)
        rep.upload(nonces.tobytes(), None, in0.tobytes(), in1.tobytes())
        m.synchronize()
        t = time.perf_counter()
        rep.compact(keep, staging)
        dt = time.perf_counter() - t
        if it:
            ts.append(dt)
        from mastic_amd import _lib
        got = np.empty((rep.n, 4), "<u4")
        assert _lib.lib().mastic_reports_download(rep._ptr, _lib.buf(got), None, None, None) == 0
        assert np.array_equal(got[:, 0], want), "the survivors' row numbers are wrong"
        del rep
    (moved, traffic, launches) = plan_model(keep, sizes, staging)
    moved_bytes = moved * sum(sizes)
    ys = d2d_yardstick(moved_bytes) if moved_bytes else [0.0]
    (t_med, y_med) = (statistics.median(ts), statistics.median(ys))
    print("%-28s staging %4d MiB  moved %8.1f MB  plan traffic %8.1f MB in %4d launches | compact ms %s median %.2f"
          " | d2d copy ms %s median %.2f | copy/compact %.2f | %.2f TB/s moved-bytes rate" % (
              label, (staging or DEFAULT_STAGING) // MIB, moved_bytes / 1e6, traffic / 1e6, launches,
              " ".join("%.2f" % (1e3 * x) for x in ts), 1e3 * t_med,
              " ".join("%.2f" % (1e3 * x) for x in ys), 1e3 * y_med, y_med / t_med if t_med else 0,
              2 * moved_bytes / t_med / 1e12 if t_med else 0), flush=True)


def run_copy(which):
    rng = np.random.default_rng(12345)
    if which in ("c2", "all"):
        m = Mastic(32, "Sum", device=0, max_measurement=255)
        n = 1000000
        for (name, p) in (("keep 50 %", 0.5), ("keep 99 %", 0.99), ("keep 1 %", 0.01)):
            keep = rng.random(n) < p
            for staging in (16 * MIB, 64 * MIB, 256 * MIB):
                copy_case(m, n, keep, staging, "C2 1M reports, " + name)
        # a gap of one for ever: every tile is staged
        keep = np.ones(n, bool)
        keep[0] = False
        copy_case(m, n, keep, 0, "C2 1M reports, first dropped")
        del m
    if which in ("c5", "all"):
        m = Mastic(32, "SumVec", device=0, length=1024, sum_vec_bits=1, chunk_length=32)
        n = 16384
        copy_case(m, n, rng.random(n) < 0.5, 0, "C5 16,384 reports, keep 50 %")


def run_sweep(compact, n_rep):
    from bench import _attrs
    bits, mx = 32, 255
    half = n_rep // 2
    m = Mastic(bits, "Sum", device=0, max_measurement=mx)
    ctx = b"mastic-mi355x-bench"
    seed = 0x4D41 + 2
    pool = _attrs(np.random.default_rng(seed), bits, 10000)
    rrng = np.random.default_rng(seed * 1000003)
    ranks = rrng.zipf(1.1, size=half)
    while (ranks > len(pool)).any():
        bad = ranks > len(pool)
        ranks[bad] = rrng.zipf(1.1, size=int(bad.sum()))
    alpha_b = pool[ranks - 1].tobytes()
    w = rrng.integers(0, mx + 1, size=half)
    nb = mx.bit_length()
    off = 2 ** nb - 1 - mx
    betas = np.concatenate([(w[:, None] >> np.arange(nb)) & 1, ((w + off)[:, None] >> np.arange(nb)) & 1],
                           axis=1).astype("<u8").tobytes()
    threshold = max(1, int(np.ceil(0.0005 * half * mx / 2)))
    nonces = rrng.integers(0, 256, size=16 * half, dtype=np.uint8).tobytes()
    rands = rrng.integers(0, 256, size=m.RAND_SIZE * half, dtype=np.uint8).tobytes()
    fresh = m.reports_shard(ctx, alpha_b, betas, nonces, rands)
    # every report twice, interleaved by a seeded shuffle: half of the batch are replays
    order = rrng.permutation(np.concatenate([np.arange(half), np.arange(half)]))
    segs = [np.frombuffer(b, np.uint8).reshape(half, -1)[order].tobytes() for b in fresh.download()]
    del fresh
    reps = m.reports_upload(*segs)
    del segs
    vk = np.random.default_rng(0x4D41).integers(0, 256, size=16, dtype=np.uint8).tobytes()
    m.synchronize()
    (timing, trace, cached) = ([], [], [])
    t0 = time.perf_counter()
    hh = compute_heavy_hitters(m, ctx, {"default": threshold}, reps, verify_key=vk, trace=trace, timing=timing,
                               frontier_cache=True, cached_levels=cached, nonce_set=NonceSet(m), compact=compact)
    m.synchronize()
    wall = time.perf_counter() - t0
    gpu = [timing[2 * i][6] + timing[2 * i + 1][6] for i in range(len(timing) // 2)]
    print("sweep compact=%s: %d reports (%d fresh), batch afterwards %d, %d heavy hitters, n_valid %d, "
          "cached levels %d | prep_init HIP-event ms: level 0 %.1f, levels 1.. %.1f | wall %.3f s" % (
              compact, n_rep, half, reps.n, len(hh), trace[-1].n_valid, len(cached), gpu[0], sum(gpu[1:]), wall),
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("copy", "sweep"):
        sys.exit(__doc__)
    if sys.argv[1] == "copy":
        run_copy(sys.argv[2] if len(sys.argv) > 2 else "all")
    else:
        run_sweep(None if sys.argv[2] == "none" else float(sys.argv[2]),
                  int(sys.argv[3]) if len(sys.argv) > 3 else 131072)
