"""The sweep driver's replay protection (``compute_heavy_hitters(...,
nonce_set=...)``), host logic on the CPU: with the plaintext stand-in
aggregator of tests/test_sweep.py and a stub nonce set (a ``dict`` walked in
index order), the reports the set does not admit vanish from every level's
result and from ``n_valid``, exactly like reports that fail verification.  The
GPU run with the real set is tests/test_gpu_sweep_replays.py."""
import random

import numpy as np

from conftest import PKG_ROOT  # noqa: F401  (puts the package on sys.path)
from mastic_amd.heavy_hitters import compute_heavy_hitters
from test_sweep import _StubMastic, _StubReports, index, plain_heavy_hitters, plain_sums


class _ModelNonceSet:
    """The set's contract in ten lines: first occurrence wins, by index."""

    def __init__(self):
        self.seen = {}
        self.calls = 0

    def admit(self, reports):
        self.calls += 1
        fresh = np.zeros(reports.n, np.uint8)
        for (i, nonce) in enumerate(reports.nonces):
            if nonce not in self.seen:
                self.seen[nonce] = True
                fresh[i] = 1
        return fresh


class _Reports(_StubReports):
    def __init__(self, meas, nonces):
        super().__init__(meas)
        self.nonces = nonces


def _workload(seed, bits, n, n_replays):
    rng = random.Random(seed)
    heavy = [rng.randrange(2 ** bits) for _ in range(3)]
    originals = []
    for i in range(n):
        v = rng.choice(heavy) if rng.random() < 0.5 else rng.randrange(2 ** bits)
        originals.append((i.to_bytes(16, "big"), (index(v, bits), 1)))
    # replays of reports of the heaviest value, so that counting them changes the result
    top = max(heavy, key=lambda h: sum(m[0] == index(h, bits) for (_n, m) in originals))
    pool = [r for r in originals if r[1][0] == index(top, bits)]
    mixed = originals + [rng.choice(pool) for _ in range(n_replays)]
    rng.shuffle(mixed)
    return (originals, mixed)


def test_replays_vanish_from_every_level_and_from_n_valid():
    bits = 7
    (originals, mixed) = _workload(11, bits, 120, 25)
    th = {'default': 8}
    want_trace, got_trace, plain_trace = [], [], []
    want = compute_heavy_hitters(_StubMastic(bits), b"ctx", th,
                                 _Reports([m for (_n, m) in originals], [n for (n, _m) in originals]),
                                 verify_key=bytes(32), trace=want_trace)
    ns = _ModelNonceSet()
    rep = _Reports([m for (_n, m) in mixed], [n for (n, _m) in mixed])
    got = compute_heavy_hitters(_StubMastic(bits), b"ctx", th, rep, verify_key=bytes(32), trace=got_trace,
                                nonce_set=ns)
    assert ns.calls == 1
    assert got == want == plain_heavy_hitters([m for (_n, m) in originals], th, bits)
    assert [(t.prefixes, t.agg_result, t.n_valid) for t in got_trace] == \
        [(t.prefixes, t.agg_result, t.n_valid) for t in want_trace]
    assert all(t.n_valid == 120 for t in got_trace)
    # without the set the replays are counted
    compute_heavy_hitters(_StubMastic(bits), b"ctx", th, rep, verify_key=bytes(32), trace=plain_trace)
    assert all(t.n_valid == 145 for t in plain_trace)
    assert sum(plain_trace[0].agg_result) == 145 and sum(got_trace[0].agg_result) == 120
    # a second sweep over the same reports with the same set keeps none of them
    again = []
    assert compute_heavy_hitters(_StubMastic(bits), b"ctx", th, rep, verify_key=bytes(32), trace=again,
                                 nonce_set=ns) == []
    assert [t.n_valid for t in again] == [0] * bits and again[0].agg_result == [0, 0]


def test_replays_and_rejected_reports_are_dropped_alike():
    """A replay (dropped before level 0) and a report that fails decide from
    level 2 on are both missing from the later levels' sums."""
    bits = 4
    meas = [(index(0b1010, bits), 1)] * 6
    nonces = [bytes([i]) * 16 for i in (0, 1, 2, 0, 1, 3)]  # reports 3 and 4 replay 0 and 1
    trace = []
    m = _StubMastic(bits, bad=(5,), bad_level=2)
    got = compute_heavy_hitters(m, b"ctx", {'default': 3}, _Reports(meas, nonces), verify_key=bytes(32), trace=trace,
                                nonce_set=_ModelNonceSet())
    assert [t.n_valid for t in trace] == [4, 4, 3, 3]
    assert [plain_sums(meas[:t.n_valid], t.prefixes) for t in trace] == [t.agg_result for t in trace]
    assert got == [index(0b1010, bits)]


def test_without_the_argument_nothing_changes():
    bits = 5
    (_originals, mixed) = _workload(3, bits, 40, 9)
    rep = _Reports([m for (_n, m) in mixed], [n for (n, _m) in mixed])
    a, b = [], []
    ra = compute_heavy_hitters(_StubMastic(bits), b"ctx", {'default': 4}, rep, verify_key=bytes(32), trace=a)
    rb = compute_heavy_hitters(_StubMastic(bits), b"ctx", {'default': 4}, rep, verify_key=bytes(32), trace=b,
                               nonce_set=None)
    assert ra == rb and [t.agg_result for t in a] == [t.agg_result for t in b]
    assert all(t.n_valid == 49 for t in a)
