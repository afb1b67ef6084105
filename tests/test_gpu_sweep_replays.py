"""The heavy-hitters sweep with replay protection on the GPU:
``compute_heavy_hitters(..., nonce_set=NonceSet(mastic))`` over 60 reports and
10 byte-exact replays of some of them, shuffled together (70 in all: two
groups of 64 reports, one partial), computes what the sweep over the 60
originals computes, at every level; without the set the replays are counted;
a second sweep with the same set keeps no report."""
import random

import pytest

from conftest import PKG_ROOT  # noqa: F401
from test_sweep import index, plain_heavy_hitters, plain_sums

pytestmark = pytest.mark.gpu


def _rows(data, size, order):
    return b"".join(data[size * i:size * (i + 1)] for i in order)


def test_sweep_with_nonce_set_equals_sweep_over_the_originals(gpu_available):
    from mastic_amd import MasticCount, NonceSet
    from mastic_amd.heavy_hitters import compute_heavy_hitters
    bits, n, n_replays = 8, 60, 10
    rng = random.Random(41)
    m = MasticCount(bits)
    ctx = b"sweep with replays"
    vals = [rng.choice([0x5a, 0xc3, 0x11]) if rng.random() < 0.6 else rng.randrange(256) for _ in range(n)]
    meas = [(index(v, bits), 1) for v in vals]
    nonces = rng.randbytes(16 * n)
    (pub, in0, in1) = m.shard_batch(ctx, [a for (a, _w) in meas], [w for (_a, w) in meas], nonces,
                                    rng.randbytes(m.RAND_SIZE * n))
    # the replays: copies of reports of the most frequent value, so counting them changes the aggregate
    top = max(set(vals), key=vals.count)
    order = list(range(n)) + rng.choices([i for i in range(n) if vals[i] == top], k=n_replays)
    rng.shuffle(order)
    sizes = (16, m.public_share_size(), m.input_share_size(0), m.input_share_size(1))
    originals = m.reports_upload(nonces, pub, in0, in1)
    mixed = m.reports_upload(*[_rows(d, s, order) for (d, s) in zip((nonces, pub, in0, in1), sizes)])
    assert mixed.n == 70
    th = {'default': 5}
    vk = rng.randbytes(32)

    want_trace, got_trace, plain_trace, again = [], [], [], []
    want = compute_heavy_hitters(m, ctx, th, originals, verify_key=vk, trace=want_trace)
    assert want == plain_heavy_hitters(meas, th, bits) and want
    ns = NonceSet(m)
    got = compute_heavy_hitters(m, ctx, th, mixed, verify_key=vk, trace=got_trace, nonce_set=ns)
    assert got == want and len(ns) == n
    assert [(t.prefixes, t.agg_result, t.n_valid) for t in got_trace] == \
        [(t.prefixes, t.agg_result, t.n_valid) for t in want_trace]
    for t in got_trace:
        assert t.n_valid == n and t.agg_result == plain_sums(meas, t.prefixes), t.level

    # without the set the replays are accepted and counted
    compute_heavy_hitters(m, ctx, th, mixed, verify_key=vk, trace=plain_trace)
    mixed_meas = [meas[i] for i in order]
    for t in plain_trace:
        assert t.n_valid == n + n_replays and t.agg_result == plain_sums(mixed_meas, t.prefixes), t.level
    assert sum(plain_trace[0].agg_result) == 70 > sum(got_trace[0].agg_result) == 60
    assert plain_trace[-1].agg_result != got_trace[-1].agg_result or plain_trace[-1].prefixes != got_trace[-1].prefixes

    # the same reports again, the same set: every one is a replay now
    assert compute_heavy_hitters(m, ctx, th, mixed, verify_key=vk, trace=again, nonce_set=ns) == []
    assert [t.n_valid for t in again] == [0] * bits and again[0].agg_result == [0, 0]
    assert len(ns) == n
