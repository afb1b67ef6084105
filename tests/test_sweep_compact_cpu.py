"""The sweep driver's compaction (``compute_heavy_hitters(..., compact=t)``),
host logic on the CPU, with the plaintext stand-in aggregator of
tests/test_sweep.py, the model nonce set of tests/test_sweep_replays_cpu.py and
a stub batch whose ``compact`` filters its rows: the batch is compacted only
after the admit and after level 0's fold, only when the dead share reaches t,
and every level's result is what the masking sweep computes.  The GPU run with
the real batch is tests/test_gpu_sweep_compact.py."""
import random

import numpy as np
import pytest

from conftest import PKG_ROOT  # noqa: F401  (puts the package on sys.path)
from mastic_amd.heavy_hitters import compute_heavy_hitters
from test_sweep import _StubMastic, _StubReports, index, plain_heavy_hitters
from test_sweep_replays_cpu import _ModelNonceSet


class _Reports(_StubReports):
    """fails_from[i]: the level from which report i fails decide (None: never)."""

    def __init__(self, meas, nonces, fails_from):
        super().__init__(meas)
        self.nonces = list(nonces)
        self.fails_from = list(fails_from)
        self.compactions = []

    def compact(self, keep, staging_bytes=0):
        assert len(keep) == self.n
        self.compactions.append((self.n, int(np.count_nonzero(keep))))
        for name in ("meas", "nonces", "fails_from"):
            setattr(self, name, [x for (x, k) in zip(getattr(self, name), keep) if k])
        self.n = len(self.meas)
        return self.n


class _Mastic(_StubMastic):
    def decide_batch(self, ctx, agg_param, ps0, ps1):
        f = self._dev.fails_from
        return (b"", np.array([0 if (x is not None and agg_param[0] >= x) else 1 for x in f], np.uint8))


BITS = 6


def _job(seed=5, n=90, n_replays=40, bad0=(4, 30, 31), bad3=(50,)):
    rng = random.Random(seed)
    heavy = [rng.randrange(2 ** BITS) for _ in range(3)]
    rows = []
    for i in range(n):
        v = rng.choice(heavy) if rng.random() < 0.6 else rng.randrange(2 ** BITS)
        rows.append((i.to_bytes(16, "big"), (index(v, BITS), 1), 0 if i in bad0 else 3 if i in bad3 else None))
    mixed = rows + [rng.choice(rows) for _ in range(n_replays)]
    rng.shuffle(mixed)
    honest = [m for (_n, m, f) in rows if f is None]
    return (mixed, honest, n, len(bad0))


def _sweep(mixed, compact, with_set=True):
    rep = _Reports([m for (_n, m, _f) in mixed], [n for (n, _m, _f) in mixed], [f for (_n, _m, f) in mixed])
    trace = []
    hh = compute_heavy_hitters(_Mastic(BITS), b"ctx", {"default": 6}, rep, verify_key=bytes(32), trace=trace,
                               nonce_set=_ModelNonceSet() if with_set else None, compact=compact)
    return (hh, [(t.level, t.prefixes, t.agg_result, t.n_valid) for t in trace], rep)


def test_compaction_points_and_results():
    (mixed, honest, n, n_bad0) = _job()
    (hh, trace, rep) = _sweep(mixed, None)
    assert rep.compactions == [] and rep.n == len(mixed)
    assert hh == plain_heavy_hitters(honest, {"default": 6}, BITS) and hh
    # t = 0: whenever a report is dead at one of the two points
    (hh0, trace0, rep0) = _sweep(mixed, 0.0)
    assert (hh0, trace0) == (hh, trace)
    assert rep0.compactions == [(len(mixed), n), (n, n - n_bad0)]  # never for the level-3 rejection
    assert rep0.n == n - n_bad0 and len(rep0.meas) == rep0.n
    # t = 0.2: 40 of 130 dead after the admit, 3 of 90 after level 0
    (hh2, trace2, rep2) = _sweep(mixed, 0.2)
    assert (hh2, trace2) == (hh, trace)
    assert rep2.compactions == [(len(mixed), n)] and rep2.n == n
    # t = 1: only a batch that is dead altogether
    (hh1, trace1, rep1) = _sweep(mixed, 1.0)
    assert (hh1, trace1) == (hh, trace) and rep1.compactions == []


def test_nothing_dead_nothing_compacted():
    (mixed, _honest, _n, _b) = _job(n_replays=0, bad0=(), bad3=(7,))
    (_hh, _trace, rep) = _sweep(mixed, 0.0)
    assert rep.compactions == []


def test_everything_dead_leaves_an_empty_batch():
    (mixed, _honest, _n, _b) = _job(n=20, n_replays=0, bad0=tuple(range(20)), bad3=())
    (hh, trace, rep) = _sweep(mixed, 1.0, with_set=False)
    assert rep.compactions == [(20, 0)] and rep.n == 0 and hh == []
    (hh_m, trace_m, _rep) = _sweep(mixed, None, with_set=False)
    assert (hh, trace) == (hh_m, trace_m)


def test_share_outside_0_1_is_refused():
    with pytest.raises(ValueError):
        compute_heavy_hitters(_Mastic(BITS), b"ctx", {"default": 6}, [], verify_key=bytes(32), compact=-0.1)
