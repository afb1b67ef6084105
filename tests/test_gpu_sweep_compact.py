"""The heavy-hitters sweep with compaction on the GPU
(``compute_heavy_hitters(..., compact=t)``): a 10-bit Sum sweep over 600
reports of which 180 are byte-exact replays of others (dropped by a
``NonceSet``), 4 encode an out-of-range weight (rejected at level 0) and one
has its seed correction word of level 4 corrupted (rejected from level 4 on,
where the sweep only masks).  ``compact=0.0`` and ``compact=0.2`` must compute
what ``compact=None``, the sweep without compaction, computes: the heavy
hitters, and every level's candidates, aggregate and ``n_valid``, with the
frontier cache on and off, and the plaintext heavy hitters of the fresh
honest reports.

What the resident batch holds afterwards follows from the two compaction
points.  After the admit 30 % of the batch is dead, so both thresholds compact
it to the 420 fresh reports.  After level 0 the dead share is 4 / 420: at
t = 0.0 the batch is compacted again, to the 416 fresh reports that passed
level 0; at t = 0.2 it is not, and the four stay masked.
"""
import random

import numpy as np
import pytest

from conftest import PKG_ROOT  # noqa: F401
from test_gpu_merge import torch_cuda  # noqa: F401
from test_sweep import index, plain_heavy_hitters

pytestmark = pytest.mark.gpu

BITS, N_FRESH, N_REPLAYS = 10, 420, 180
BAD_WEIGHT = (3, 77, 200, 419)
BAD_CW = 150      # seed correction word of level BAD_LEVEL corrupted; weight 0
BAD_LEVEL = 4
CTX = b"sweep with compaction"
TH = {"default": 25}


class _Job:
    def __init__(self):
        from mastic_amd import MasticSum
        self.m = m = MasticSum(BITS, 3)
        rng = random.Random(2718)
        heavy = [rng.randrange(2 ** BITS) for _ in range(5)]
        vals = [rng.choice(heavy) if rng.random() < 0.6 else rng.randrange(2 ** BITS) for _ in range(N_FRESH)]
        weights = [rng.randrange(1, 4) for _ in range(N_FRESH)]
        weights[BAD_CW] = 0
        F = m.field
        bad = [F(1), F(1), F(0), F(1)]  # 3 with inconsistent offset bits: the FLP rejects it
        betas = b"".join(F.encode_vec(bad if i in BAD_WEIGHT else m.encode_measurement(weights[i]))
                         for i in range(N_FRESH))
        alphas = b"".join((v << (16 - BITS)).to_bytes(2, "big") for v in vals)
        nonces = rng.randbytes(16 * N_FRESH)
        (pub, in0, in1) = m.shard_encoded(CTX, N_FRESH, alphas, betas, nonces, rng.randbytes(m.RAND_SIZE * N_FRESH))
        seg = [np.frombuffer(b, np.uint8).reshape(N_FRESH, -1).copy() for b in (nonces, pub, in0, in1)]
        seg[1][BAD_CW, (2 * BITS + 7) // 8 + 16 * BAD_LEVEL] ^= 1
        order = list(range(N_FRESH)) + rng.choices(range(N_FRESH), k=N_REPLAYS)
        rng.shuffle(order)
        self.rows = [s[order].tobytes() for s in seg]
        self.vk = rng.randbytes(32)
        self.honest = [(index(v, BITS), w) for (i, (v, w)) in enumerate(zip(vals, weights))
                       if i not in BAD_WEIGHT and i != BAD_CW]

    def sweep(self, compact, frontier_cache, merge=None):
        from mastic_amd import NonceSet
        from mastic_amd.heavy_hitters import compute_heavy_hitters
        rep = self.m.reports_upload(*self.rows)  # a compaction mutates the batch: a new one per sweep
        (trace, cached) = ([], [])
        hh = compute_heavy_hitters(self.m, CTX, TH, rep, verify_key=self.vk, trace=trace, nonce_set=NonceSet(self.m),
                                   frontier_cache=frontier_cache, cached_levels=cached, compact=compact, merge=merge)
        return (hh, [(t.level, t.prefixes, t.agg_result, t.n_valid) for t in trace], cached, rep.n)


@pytest.fixture(scope="module")
def job(gpu_available):
    return _Job()


@pytest.mark.parametrize("frontier_cache", [False, True], ids=["cache off", "cache on"])
def test_compacting_sweeps_equal_the_masking_sweep(job, frontier_cache):
    (hh, trace, cached, n) = job.sweep(None, frontier_cache)
    assert n == N_FRESH + N_REPLAYS
    assert hh == plain_heavy_hitters(job.honest, TH, BITS) and hh
    assert [t[3] for t in trace[:BAD_LEVEL]] == [N_FRESH - len(BAD_WEIGHT)] * BAD_LEVEL
    assert all(t[3] == N_FRESH - len(BAD_WEIGHT) - 1 for t in trace[BAD_LEVEL:])
    for (t, n_after) in ((0.0, N_FRESH - len(BAD_WEIGHT)), (0.2, N_FRESH)):
        (hh_c, trace_c, cached_c, n_c) = job.sweep(t, frontier_cache)
        assert hh_c == hh, t
        assert trace_c == trace, t
        assert n_c == n_after, t
        if frontier_cache:
            assert cached_c, "the cache recovers after the miss a compaction forces"
            assert set(cached_c) >= set(c for c in cached if c > 1), (cached_c, cached)
    job.m.set_frontier_cache(False)


def test_compaction_rejects_a_share_outside_0_1(job):
    from mastic_amd.heavy_hitters import compute_heavy_hitters
    with pytest.raises(ValueError):
        compute_heavy_hitters(job.m, CTX, TH, [], verify_key=job.vk, compact=1.5)


def test_device_merge_sees_the_shorter_mask(torch_cuda, job):  # noqa: F811
    from mastic_amd.merge import CommMerge
    (hh, trace, _cached, _n) = job.sweep(None, False)
    m = job.m
    m.comm_init(1, 0, m.comm_unique_id())
    try:
        (hh_c, trace_c, _c, n_c) = job.sweep(0.0, False, merge=CommMerge(m))
    finally:
        m.comm_destroy()
    assert hh_c == hh and trace_c == trace and n_c == N_FRESH - len(BAD_WEIGHT)
