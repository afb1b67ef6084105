"""Timing of mastic_aggregate_grouped on one MI355X against the folds it
replaces, all in one process on one box.

Shapes
  c2      the C2 step: Mastic(32, Sum 255), 16,384 reports, 10,000 prefixes at
          level 31 (bench.py's inputs), 20,000 rows of Field64
  sweep   a sweep level: the same instance, 350 prefixes at level 15 (700
          rows) over --reports reports (default 1,000,000, c2sweep's batch)

At each shape and G = 1, 8, 64, 4,096 groups:
  (a) one unmasked mastic_aggregate
  (b) G masked mastic_aggregate calls, one per group (the only way to get G
      bucket shares without the grouped call); the masks are built outside
      the timed region
  (c) one mastic_aggregate_grouped, for ids in time-ordered runs (report r in
      group r * G // n: whole waves share an id) and for uniformly random ids
(a) and (b) run k_fold, which the grouped fold does not touch: they are the
baseline.  Every figure is the host wall time of the blocking C call(s) into
preallocated, touched host buffers (each call ends in a stream synchronise and
includes its own mask / id upload and the download of its result: G shares in
(b) and in (c) alike), the median of --reps runs after one warm-up.  The (c)
result is compared with (b)'s shares, byte for byte.

GPU box only:  python3 tools/grouped_fold_probe.py [--shape c2|sweep|all] [--reports N] [--reps R]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd")]

GROUPS = (1, 8, 64, 4096)


def setup(shape, n_reports):
    """A Mastic with aggregator 0's prep_init result of the shape in HBM."""
    from bench import CONFIGS, agg_param_bytes, synth
    from mastic_amd import Mastic
    cfg = CONFIGS["c2"]
    m = Mastic(32, "Sum", max_measurement=255)
    n = 16384 if shape == "c2" else n_reports
    (attrs, alphas, betas, nonces, rands) = synth(m, cfg, 0, n, 10000, 0x4D41)
    ctx = b"mastic-mi355x-bench"
    dev = m.reports_shard(ctx, alphas, betas, nonces, rands)
    if shape == "c2":
        enc = agg_param_bytes(31, attrs)
    else:
        pfx = np.unique(attrs[:, :2], axis=0)[:350]  # distinct 16-bit prefixes, MSB-first rows, sorted
        enc = agg_param_bytes(15, pfx)
    m.prep_init_device(dev, bytes(range(16)), ctx, 0, enc)
    m.synchronize()
    rows = int.from_bytes(enc[2:6], "big") * (1 + m.OUTPUT_LEN)
    print("# %s: %d reports x %d rows of %d B, out shares %.2f GB" % (
        shape, n, rows, m.field.ENCODED_SIZE, n * rows * m.field.ENCODED_SIZE / 1e9), flush=True)
    return (m, dev, n, rows)


def median_ms(ts):
    return 1e3 * statistics.median(ts)


def run_table(shape, n_reports, reps):
    from mastic_amd import _lib
    (m, _dev, n, rows) = setup(shape, n_reports)
    lib = _lib.lib()
    share = rows * m.field.ENCODED_SIZE
    rng = np.random.default_rng(7)

    def fold(mask, out):
        t = time.perf_counter()
        rc = lib.mastic_aggregate(m._ctx, 0, _lib.buf(mask), _lib.buf(out))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt

    def grouped(ids, G, out, counts):
        t = time.perf_counter()
        rc = lib.mastic_aggregate_grouped(m._ctx, 0, _lib.buf(ids), G, None, _lib.buf(out), _lib.buf(counts))
        dt = time.perf_counter() - t
        assert rc == 0
        return dt

    one = np.zeros(share, np.uint8)
    fold(None, one)
    a = median_ms([fold(None, one) for _ in range(reps)])
    print("%-6s (a) one unmasked mastic_aggregate: %.3f ms = %.2f TB/s of out shares" % (
        shape, a, n * share / a / 1e9), flush=True)
    print("%-6s %5s %-7s | (b) G masked folds ms | (c) grouped ms (min..max)   | c/b    | c/a" % (shape, "G", "ids"))
    for G in GROUPS:
        out_b = np.zeros(G * share, np.uint8)
        out_c = np.zeros(G * share, np.uint8)
        counts = np.zeros(G, np.uint64)
        for pattern in ("runs", "random"):
            if pattern == "runs":
                ids = (np.arange(n, dtype=np.uint64) * G // n).astype(np.uint32)
            else:
                ids = rng.integers(0, G, size=n, dtype=np.uint32)
            grouped(ids, G, out_c, counts)
            cs = [grouped(ids, G, out_c, counts) for _ in range(reps)]
            assert list(counts) == list(np.bincount(ids, minlength=G))
            bs = []
            for it in range(reps + 1):  # the first is the warm-up
                total = 0.0
                for g in range(G):
                    mask = (ids == g).astype(np.uint8)
                    total += fold(mask, out_b[g * share:(g + 1) * share])
                if it:
                    bs.append(total)
                assert np.array_equal(out_b, out_c), "grouped shares differ from the masked folds"
            (b, c) = (median_ms(bs), median_ms(cs))
            print("%-6s %5d %-7s | %10.3f            | %9.3f (%.3f..%.3f) | %.4f | %.2f" % (
                shape, G, pattern, b, c, 1e3 * min(cs), 1e3 * max(cs), c / b, c / a), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="all", choices=("c2", "sweep", "all"))
    ap.add_argument("--reports", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for shape in (("c2", "sweep") if args.shape == "all" else (args.shape,)):
        run_table(shape, args.reports, args.reps)
