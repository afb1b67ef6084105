"""Timing of mastic_decide_peer on one MI355X against the host detour it
replaces, for one aggregator of two.

The job: this aggregator (agg_id 0) has its prep_init result in HBM and the
peer's prep shares in host memory, as they came off the wire; it wants its
accept mask.
  peer     one mastic_decide_peer: upload of the peer's rows, k_decide_peer,
           download of accept, codes and (joint randomness) prep messages
  detour   what INTEGRATION.md §4 described before: mastic_prep_result (the own
           prep shares, joint-rand seeds where the call has them, status) +
           mastic_decide_batch (both shares uploaded again) + the numpy
           confirmation (status == 0, prep message == own joint-rand seed)
With --knobs-lib (a -DMASTIC_EXPERIMENT_KNOBS build of the library) `peer` is
timed twice, with k_decide_peer reading the peer's rows per lane (direct) and
through LDS (lds): the two access patterns DESIGN.md "Deciding against a peer"
compares.

Configurations: c2 = Mastic(32, Sum 255), Field64, no joint randomness;
f128 = Mastic(32, Histogram length 8 chunk 3), Field128 with joint randomness;
f128wide = Mastic(32, Histogram length 12 chunk 6), whose level-0 rows (288
bytes) are above the 252 bytes the LDS pattern holds, so its `lds` is the
direct pattern too.
Levels: 0 with the weight check (2 candidates), 1 without (4 candidates).

Every figure is the host wall time of the blocking C call(s) into
preallocated, touched host buffers, each ending in a stream synchronise; the
variants alternate within one process, --reps rounds after one warm-up round,
median (min..max).  The accept masks of all variants are compared.

GPU box only:
  python3 tools/decide_peer_probe.py --config c2 --reports 65536     one process
  python3 tools/decide_peer_probe.py --all [--knobs-lib PATH]        a fresh process per configuration and size
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd")]

CONFIGS = {
    "c2": dict(circuit="Sum", kw=dict(bits=32, max_measurement=255)),
    "f128": dict(circuit="Histogram", kw=dict(bits=32, length=8, chunk_length=3)),
    "f128wide": dict(circuit="Histogram", kw=dict(bits=32, length=12, chunk_length=6)),
}
SIZES = (65536, 1048576)
CTX = b"mastic-mi355x-bench"
LDS_KNOB = "MASTIC_DECIDE_PEER_LDS"


def level_param(level):
    """Every candidate of the level, the weight check at level 0 only."""
    from bench import agg_param_bytes
    count = 2 ** (level + 1)
    attrs = np.array([[v << (7 - level)] for v in range(count)], np.uint8)
    return agg_param_bytes(level, attrs)[:-1] + bytes([int(level == 0)])


def run(config, n, reps, knobs_lib):
    from bench import synth
    from mastic_amd import Mastic, _lib
    if knobs_lib:
        _lib.load(knobs_lib)
    cfg = CONFIGS[config]
    m = Mastic(cfg["kw"]["bits"], cfg["circuit"], **{k: v for (k, v) in cfg["kw"].items() if k != "bits"})
    lib = _lib.lib()
    (_attrs, alphas, betas, nonces, rands) = synth(m, cfg, 0, n, 10000, 0x4D41)
    dev = m.reports_shard(CTX, alphas, betas, nonces, rands)
    vk = bytes(range(16))
    jr = m.JOINT_RAND_LEN > 0
    for level in (0, 1):
        enc = level_param(level)
        wc = level == 0
        psz = m.prep_share_size(wc)
        for agg_id in range(2):
            m.prep_init_device(dev, vk, CTX, agg_id, enc)
        peer = np.frombuffer(m.prep_result(dev, 1, enc)[0], np.uint8).copy()  # what came off the wire
        check_jr = wc and jr
        # preallocated, touched host buffers
        own = np.zeros(n * psz, np.uint8)
        seeds = np.zeros(32 * n, np.uint8)
        status = np.zeros(n, np.int32)
        msgs = np.zeros(32 * n, np.uint8)
        valid = np.zeros(n, np.uint8)
        acc = np.zeros(n, np.uint8)
        code = np.zeros(n, np.uint8)
        pmsgs = np.zeros(32 * n, np.uint8)

        def peer_call():
            t = time.perf_counter()
            rc = lib.mastic_decide_peer(m._ctx, 0, CTX, len(CTX), _lib.buf(peer), None, n, _lib.buf(acc),
                                        _lib.buf(code), _lib.buf(pmsgs) if check_jr else None)
            dt = time.perf_counter() - t
            assert rc == 0
            return (dt, acc.copy())

        def detour():
            t = time.perf_counter()
            rc = lib.mastic_prep_result(m._ctx, 0, _lib.buf(own), _lib.buf(seeds) if check_jr else None, None,
                                        _lib.buf(status))
            assert rc == 0
            rc = lib.mastic_decide_batch(m._ctx, CTX, len(CTX), enc, len(enc), n, _lib.buf(own), _lib.buf(peer),
                                         _lib.buf(msgs), _lib.buf(valid))
            assert rc == 0
            mask = (valid == 1) & (status == 0)
            if check_jr:
                mask &= (msgs.reshape(n, 32) == seeds.reshape(n, 32)).all(axis=1)
            dt = time.perf_counter() - t
            return (dt, mask.astype(np.uint8))

        def with_knob(value):
            def call():
                os.environ[LDS_KNOB] = value
                try:
                    return peer_call()
                finally:
                    del os.environ[LDS_KNOB]
            return call

        variants = [("detour", detour)]
        variants += [("peer-direct", with_knob("0")), ("peer-lds", with_knob("1"))] if knobs_lib else [("peer", peer_call)]
        times = {name: [] for (name, _f) in variants}
        masks = {}
        for it in range(reps + 1):  # the first round is the warm-up
            for (name, f) in variants:
                (dt, mask) = f()
                masks[name] = mask
                if it:
                    times[name].append(dt)
        ref = masks["detour"]
        assert ref.all(), "honest reports: every one is accepted"
        for (name, mask) in masks.items():
            assert np.array_equal(mask, ref), name
        base = statistics.median(times["detour"])
        for (name, _f) in variants:
            ts = times[name]
            med = statistics.median(ts)
            print("%-4s n=%-8d level %d wc=%d psz=%-4d %-12s %9.3f ms (%.3f..%.3f)  x%.2f of detour  wire %.1f MB" % (
                config, n, level, int(wc), psz, name, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), med / base,
                n * psz / 1e6), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--reports", type=int, default=SIZES[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--knobs-lib", default=None, help="a -DMASTIC_EXPERIMENT_KNOBS build: time both row access patterns")
    ap.add_argument("--all", action="store_true", help="every configuration and size, a fresh process each")
    ap.add_argument("--timeout", type=int, default=280, help="seconds per process of --all")
    args = ap.parse_args()
    if not args.all:
        run(args.config, args.reports, args.reps, args.knobs_lib)
        sys.exit(0)
    for config in sorted(CONFIGS):
        for n in SIZES:
            cmd = [sys.executable, os.path.abspath(__file__), "--config", config, "--reports", str(n),
                   "--reps", str(args.reps)] + (["--knobs-lib", args.knobs_lib] if args.knobs_lib else [])
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
            if rc != 0:  # nothing more runs on the GPU after a failure
                sys.exit("decide_peer_probe: %s n=%d exited with %d" % (config, n, rc))
