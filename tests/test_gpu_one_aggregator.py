"""Two :class:`~mastic_amd.aggregator.Aggregator` objects on two ctxs, each
over a batch that lacks the other's input share, against the both-on-one-GPU
drivers on a third ctx with both shares: ``sweep_lockstep`` must compute what
``compute_heavy_hitters`` computes, level by level."""
import hashlib
import random

import numpy as np
import pytest

from conftest import PKG_ROOT  # noqa: F401
from test_sweep import index, plain_heavy_hitters

pytestmark = pytest.mark.gpu

BITS = 6
N = 200
CTX = b"one aggregator of two"
BUDGET = 1 << 30  # HBM work budget per ctx: several ctxs are alive at once, and the default is most of the free HBM


class _TotalAtLeast:
    """Threshold on a vector-valued aggregate (Histogram): its total."""

    def __init__(self, t):
        self.t = t

    def __le__(self, other):  # `count >= threshold` with count a list
        return sum(other) >= self.t


def _budgeted(m):
    m.set_memory_budget(BUDGET)
    return m


def _make(name):
    from mastic_amd import MasticCount, MasticHistogram, MasticSum
    return _budgeted({"Count": lambda: MasticCount(BITS), "Sum": lambda: MasticSum(BITS, 255),
                      "Histogram": lambda: MasticHistogram(BITS, 4, 2)}[name]())


def _weight(name, rng):
    return {"Count": lambda: int(rng.random() < 0.9), "Sum": lambda: rng.randrange(256),
            "Histogram": lambda: rng.randrange(4)}[name]()


def _threshold(name):
    return {"Count": {"default": 12}, "Sum": {"default": 1500, index(0b1, 1): 2500},
            "Histogram": {"default": _TotalAtLeast(12)}}[name]


class _Job:
    """Three ctxs of one configuration and N sharded reports as wire bytes."""

    def __init__(self, gpu_available, name):
        self.name = name
        self.ms = [_make(name) for _ in range(3)]
        m = self.ms[2]
        rng = random.Random(100 + sum(map(ord, name)))
        heavy = [rng.randrange(2 ** BITS) for _ in range(4)]
        self.vals = [rng.choice(heavy) if rng.random() < 0.6 else rng.randrange(2 ** BITS) for _ in range(N)]
        self.weights = [_weight(name, rng) for _ in range(N)]
        alphas = [index(v, BITS) for v in self.vals]
        nonces = rng.randbytes(16 * N)
        (pub, in0, in1) = m.shard_batch(CTX, alphas, self.weights, nonces, rng.randbytes(m.RAND_SIZE * N))
        self.seg = [np.frombuffer(b, np.uint8).reshape(N, -1).copy() for b in (nonces, pub, in0, in1)]
        self.vk = rng.randbytes(16)

    def rows(self, order=None):
        return [(s if order is None else s[order]).tobytes() for s in self.seg]

    def batches(self, rows):
        (nonces, pub, in0, in1) = rows
        return [self.ms[0].reports_upload(nonces, pub, in0, None), self.ms[1].reports_upload(nonces, pub, None, in1),
                self.ms[2].reports_upload(nonces, pub, in0, in1)]


_jobs = {}


@pytest.fixture(scope="module")
def job(gpu_available):
    def get(name):
        if name not in _jobs:
            _jobs[name] = _Job(gpu_available, name)
        return _jobs[name]
    yield get
    _jobs.clear()


def _levels(trace):
    return [(t.level, t.prefixes, t.agg_result, t.n_valid) for t in trace]


@pytest.mark.parametrize("name", ["Count", "Sum", "Histogram"])
def test_lockstep_sweep_equals_the_two_share_sweep(job, name):
    from mastic_amd import Aggregator
    from mastic_amd.aggregator import sweep_lockstep
    from mastic_amd.heavy_hitters import compute_heavy_hitters
    j = job(name)
    th = _threshold(name)
    (dev0, dev1, dev2) = j.batches(j.rows())
    (want_trace, trace) = ([], [])
    want = compute_heavy_hitters(j.ms[2], CTX, th, dev2, verify_key=j.vk, trace=want_trace)
    aggs = [Aggregator(j.ms[a], a, CTX, j.vk, dev) for (a, dev) in enumerate((dev0, dev1))]
    got = sweep_lockstep(aggs[0], aggs[1], th, trace)
    assert got == want and got, "the workload has heavy hitters"
    assert _levels(trace) == _levels(want_trace)
    assert len(trace) == BITS and all(t.n_valid == N for t in trace)
    if name != "Histogram":
        assert got == plain_heavy_hitters([(index(v, BITS), w) for (v, w) in zip(j.vals, j.weights)], th, BITS)


@pytest.mark.parametrize("name", ["Count", "Sum", "Histogram"])
def test_lockstep_sweep_with_dead_reports_cache_and_compaction(job, name):
    """One report with the seed correction word of level 2 corrupted (dropped
    from level 2 on), one byte-exact replay (dropped by each aggregator's own
    NonceSet), the frontier cache on; then the same with compact=0.0."""
    from mastic_amd import Aggregator, NonceSet
    from mastic_amd.aggregator import run_round, sweep_lockstep  # noqa: F401
    from mastic_amd.heavy_hitters import compute_heavy_hitters
    j = job(name)
    th = _threshold(name)
    order = list(range(N)) + [17]  # report 17 again, at the end
    rows = j.rows(order)
    pub = np.frombuffer(rows[1], np.uint8).reshape(N + 1, -1).copy()
    pub[40, (2 * BITS + 7) // 8 + 16 * 2] ^= 1
    rows[1] = pub.tobytes()
    results = {}
    for compact in (None, 0.0):
        (dev0, dev1, dev2) = j.batches(rows)
        (want_trace, want_cached) = ([], [])
        want = compute_heavy_hitters(j.ms[2], CTX, th, dev2, verify_key=j.vk, trace=want_trace,
                                     nonce_set=NonceSet(j.ms[2]), frontier_cache=True, cached_levels=want_cached,
                                     compact=compact)
        aggs = [Aggregator(j.ms[a], a, CTX, j.vk, dev, nonce_set=NonceSet(j.ms[a]), frontier_cache=True,
                           compact=compact) for (a, dev) in enumerate((dev0, dev1))]
        assert [a.n_valid for a in aggs] == [N, N]
        cached = [[], []]

        class _Spy:  # the collector's view of each round: which levels took the cache's hit path
            def __init__(self, agg, log):
                (self.agg, self.log) = (agg, log)

            def __getattr__(self, k):
                return getattr(self.agg, k)

            def settle(self, verdict):
                out = self.agg.settle(verdict)
                if self.agg.last_was_cached:
                    self.log.append(len(self.agg.prev_agg_params) - 1)
                return out

        trace = []
        got = sweep_lockstep(_Spy(aggs[0], cached[0]), _Spy(aggs[1], cached[1]), th, trace)
        assert got == want
        assert _levels(trace) == _levels(want_trace)
        assert [t.n_valid for t in trace] == [N, N] + [N - 1] * (BITS - 2)
        assert cached[0] == cached[1] == want_cached and want_cached
        assert [a.n for a in aggs] == [dev2.n, dev2.n] and dev2.n == (N + 1 if compact is None else N)
        results[compact] = (got, _levels(trace))
        for m in j.ms:
            m.set_frontier_cache(False)
    assert results[None] == results[0.0]


def _reports(mastic, ctx, measurements, rng):
    out = []
    for m in measurements:
        nonce = rng.randbytes(16)
        (pub, ins) = mastic.shard(ctx, m, nonce, rng.randbytes(mastic.RAND_SIZE))
        out.append((nonce, pub, ins))
    return out


def _pair(make, ctx, reports, verify_key):
    from mastic_amd import Aggregator
    return [Aggregator(make(), a, ctx, verify_key, [(nonce, pub, ins[a]) for (nonce, pub, ins) in reports])
            for a in range(2)]


def test_example_weighted_heavy_hitters_mode(gpu_available):
    """poc/examples.py:94-128, as tests/test_gpu_sweep.py states it."""
    from mastic_amd import MasticCount
    from mastic_amd.aggregator import sweep_lockstep
    bits = 4
    ctx = b'example_weighted_heavy_hitters_mode'
    mastic = _budgeted(MasticCount(bits))
    ix = mastic.vidpf.test_index_from_int
    measurements = [(ix(v, bits), w) for (v, w) in [
        (0b1001, 1), (0b0000, 1), (0b0000, 0), (0b0000, 1), (0b1001, 1), (0b0000, 1),
        (0b1100, 1), (0b0011, 1), (0b1111, 0), (0b1111, 0), (0b1111, 1)]]
    reports = _reports(mastic, ctx, measurements, random.Random(5))
    (a0, a1) = _pair(lambda: _budgeted(MasticCount(bits)), ctx, reports, random.Random(1).randbytes(16))
    assert sweep_lockstep(a0, a1, {'default': 2}) == [ix(0b0000, bits), ix(0b1001, bits)]


def test_example_weighted_heavy_hitters_mode_with_different_thresholds(gpu_available):
    """poc/examples.py:131-169"""
    from mastic_amd import MasticCount
    from mastic_amd.aggregator import sweep_lockstep
    bits = 4
    ctx = b'example_weighted_heavy_hitters_mode_with_different_thresholds'
    mastic = _budgeted(MasticCount(bits))
    ix = mastic.vidpf.test_index_from_int
    measurements = [(ix(v, bits), 1) for v in
                    [0b0000, 0b0001, 0b1001, 0b1001, 0b1010, 0b1010, 0b1111, 0b1111, 0b1111, 0b1111, 0b1111]]
    reports = _reports(mastic, ctx, measurements, random.Random(6))
    thresholds = {'default': 2, ix(0b00, 2): 1, ix(0b10, 2): 3, ix(0b11, 2): 5}
    (a0, a1) = _pair(lambda: _budgeted(MasticCount(bits)), ctx, reports, random.Random(2).randbytes(16))
    trace = []
    assert sweep_lockstep(a0, a1, thresholds, trace) == [ix(0b0000, bits), ix(0b0001, bits), ix(0b1111, bits)]
    assert [t.n_valid for t in trace] == [11] * bits


def test_example_attribute_based_metrics_mode(gpu_available):
    """poc/examples.py:172-260: one round at the last level with the weight
    check, each aggregator on its own ctx."""
    from mastic_amd import MasticSum
    from mastic_amd.aggregator import run_round
    from mastic_amd.rounds import unshard_raw
    bits = 8
    ctx = b'example_attribute_based_metrics_mode'
    mastic = _budgeted(MasticSum(bits, 3))

    def h(attr):
        return mastic.vidpf.test_index_from_int(hashlib.sha3_256(attr.encode('ascii')).digest()[0], bits)

    measurements = [('United States', 1), ('Greece', 1), ('United States', 2), ('Greece', 0),
                    ('United States', 0), ('India', 1), ('Greece', 0), ('United States', 1),
                    ('Greece', 1), ('Greece', 3), ('Greece', 1)]
    reports = _reports(mastic, ctx, [(h(a), v) for (a, v) in measurements], random.Random(7))
    attrs = ['Greece', 'Mexico', 'United States']
    agg_param = (bits - 1, list(map(h, attrs)), True)
    (a0, a1) = _pair(lambda: _budgeted(MasticSum(bits, 3)), ctx, reports, random.Random(3).randbytes(16))
    alive = run_round(a0, a1, mastic.encode_agg_param(agg_param))
    assert alive.all() and a0.n_valid == a1.n_valid == len(measurements)
    shares = [a0.agg_share(raw=True), a1.agg_share(raw=True)]
    assert unshard_raw(mastic, shares, len(measurements)) == [6, 0, 4]
    assert mastic.unshard(agg_param, [a0.agg_share(raw=False), a1.agg_share(raw=False)], len(measurements)) == [6, 0, 4]


@pytest.mark.parametrize("name", ["Sum", "Histogram"])
def test_one_grouped_round(job, name):
    """Aggregator.aggregate_grouped after settle equals Mastic.aggregate_grouped
    of the two-share ctx under the same mask (one report is rejected)."""
    from mastic_amd import NO_GROUP, Aggregator
    from mastic_amd.aggregator import run_round
    j = job(name)
    rows = j.rows()
    in0 = np.frombuffer(rows[2], np.uint8).reshape(N, -1).copy()
    in0[9, 20] ^= 0x40  # a bit of report 9's leader proof share: the FLP rejects it
    rows[2] = in0.tobytes()
    (dev0, dev1, dev2) = j.batches(rows)
    enc = j.ms[2].encode_agg_param((0, ((False,), (True,)), True))
    aggs = [Aggregator(j.ms[a], a, CTX, j.vk, dev) for (a, dev) in enumerate((dev0, dev1))]
    alive = run_round(aggs[0], aggs[1], enc)
    for a in range(2):
        j.ms[2].prep_init_device(dev2, j.vk, CTX, a, enc)
    (accept, _codes) = j.ms[2].decide_results(CTX, N)
    assert alive.tolist() == (accept == 1).tolist() == [i != 9 for i in range(N)]
    rng = random.Random(8)
    n_groups = 5
    groups = np.array([NO_GROUP if rng.random() < 0.1 else rng.randrange(n_groups) for _ in range(N)], np.uint32)
    for a in range(2):
        (want, want_counts) = j.ms[2].aggregate_grouped(a, enc, groups, n_groups, valid=accept, raw=True)
        (got, counts) = aggs[a].aggregate_grouped(groups, n_groups, raw=True)
        assert got == want and counts.tolist() == want_counts.tolist()
        assert aggs[a].agg_share(raw=True) == j.ms[2].aggregate_device(a, enc, accept, raw=True)
    assert sum(counts.tolist()) == int(((groups != NO_GROUP) & alive).sum())
