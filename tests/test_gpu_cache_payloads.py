"""Payloads-format frontier-cache nodes (Mastic.set_frontier_cache_nodes;
include/mastic_hip.h mastic_set_frontier_cache_nodes, ABI 8).

A cache slot holds its nodes as seeds (20 B: a hit re-runs each parent's
convert stream) or as payloads (next seed, control bit and the corrected
payload: a hit recomputes nothing).  The format is chosen by the call that
writes the slot and a hit reads either, so every case here is a result
comparison: prep shares and out shares of every level equal a cache-off
context's (and the CPU oracle's for sampled reports), whatever the formats of
the slot read and the slot written.

Shapes: 150 reports (two full 64-lane groups and a ragged one of 22), alphas
from a pool of 12 so that candidates survive to the last level, and three
circuits -- Count bits 10 (Field64, VALUE_LEN 2: one block per stream), Sum
bits 9 max 5 (Field64, an odd element count: the two-elements-per-block tail)
and Histogram bits 6 length 4 chunk 2 (Field128, one element per block): the
smallest at which the node stride, the ragged group and both field widths can
each go wrong.  The candidate lists are those of a real sweep
(compute_heavy_hitters' trace) for Count and Sum; the sweep driver thresholds
scalar results only, so for Histogram they are the lists a Count sweep over
the same alphas yields (every prefix held by >= 4 reports, both children), and
the driver's heavy hitters are compared for Count and Sum."""
import ctypes
import json
import os
import random

import pytest

from conftest import GOLDEN
from test_gpu_parity import CTX, _oracle_for, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

N = 150
CIRCUITS = {
    "Count": ("Count", dict(bits=10)),
    "Sum": ("Sum", dict(bits=9, max_measurement=5)),
    "Histogram": ("Histogram", dict(bits=6, length=4, chunk_length=2)),
}


def _mk(pkg, name):
    (circuit, kw) = CIRCUITS[name]
    kw = dict(kw)
    return pkg.Mastic(kw.pop("bits"), circuit, **kw)


def _reports(m, rng, n, pool_size):
    pool = [tuple(bool(rng.getrandbits(1)) for _ in range(m.BITS)) for _ in range(pool_size)]
    alphas = [pool[min(int(rng.paretovariate(1.0)) - 1, pool_size - 1)] for _ in range(n)]
    if m.circuit == "Count":
        weights = [rng.randrange(2) for _ in range(n)]
    elif m.circuit == "Histogram":
        weights = [rng.randrange(m.length) for _ in range(n)]
    else:
        weights = [rng.randrange(m.max_measurement + 1) for _ in range(n)]
    nonces = bytes(rng.getrandbits(8) for _ in range(16 * n))
    rands = bytes(rng.getrandbits(8) for _ in range(m.RAND_SIZE * n))
    return alphas, weights, nonces, rands


def _plain_levels(alphas, bits, th):
    """The candidate lists of a threshold sweep over the alphas alone."""
    levels, prefixes = [], [(False,), (True,)]
    for level in range(bits):
        if not prefixes:
            break
        levels.append((level, tuple(prefixes), level == 0))
        keep = [p for p in prefixes if sum(a[:level + 1] == p for a in alphas) >= th]
        prefixes = [p + (b,) for p in keep for b in (False, True)]
    return levels


class Walk:
    """One circuit's batch, its sweep levels and the cache-off results of
    every level and aggregator: computed once, shared by the tests, never
    changed."""

    def __init__(self, pkg, name):
        from mastic_amd.heavy_hitters import compute_heavy_hitters
        rng = random.Random(4100 + sorted(CIRCUITS).index(name))
        self.pkg, self.name = pkg, name
        self.m_off = _mk(pkg, name)
        (self.alphas, weights, self.nonces, rands) = _reports(self.m_off, rng, N, 12)
        (self.pub, self.in0, self.in1) = self.m_off.shard_batch(CTX, self.alphas, weights, self.nonces, rands)
        self.vk = bytes(rng.getrandbits(8) for _ in range(32))
        self.dev_off = self.m_off.reports_upload(self.nonces, self.pub, self.in0, self.in1)
        self.hh = None
        if name == "Histogram":
            self.levels = _plain_levels(self.alphas, self.m_off.BITS, 4)
        else:
            trace = []
            self.hh = compute_heavy_hitters(self.m_off, CTX, {"default": 4}, self.dev_off, verify_key=self.vk,
                                            trace=trace)
            self.levels = [(lv.level, tuple(lv.prefixes), lv.level == 0) for lv in trace if lv.prefixes]
        assert self.levels[-1][0] == self.m_off.BITS - 1, "the workload should keep candidates down to the last level"
        self.want = {}
        for ap in self.levels:
            for agg_id in range(2):
                self.m_off.prep_init_device(self.dev_off, self.vk, CTX, agg_id, ap)
                r = self.m_off.prep_result(self.dev_off, agg_id, ap, want_out_shares=True)
                self.want[(ap[0], agg_id)] = (r[0], r[2])
        self.runs = {}

    def upload(self, m):
        return m.reports_upload(self.nonces, self.pub, self.in0, self.in1)

    def run(self, key, modes, oracle_hits=0):
        """The walk on a fresh cache-on context, the mode set before each
        level from ``modes`` (cycled): asserts every level bit-identical to
        cache-off and returns (levels that hit per aggregator, the (in, out)
        pairs of all calls in order).  Memoised by ``key``."""
        if key in self.runs:
            return self.runs[key]
        m = _mk(self.pkg, self.name)
        dev = self.upload(m)
        m.set_frontier_cache(True)
        o = _oracle_for(m) if oracle_hits else None
        psz, isz = m.public_share_size(), m.input_share_size(1)
        hits, pairs, checked = set(), [], 0
        try:
            for (k, ap) in enumerate(self.levels):
                m.set_frontier_cache_nodes(modes[k % len(modes)])
                for agg_id in range(2):
                    m.prep_init_device(dev, self.vk, CTX, agg_id, ap)
                    got = m.prep_result(dev, agg_id, ap, want_out_shares=True)
                    assert (got[0], got[2]) == self.want[(ap[0], agg_id)], "level %d agg %d" % (ap[0], agg_id)
                    pair = m.last_cache_nodes()
                    pairs.append(pair)
                    cached = m.last_prep_was_cached()
                    assert (pair[0] is not None) == cached and pair[1] is not None
                    if cached:
                        hits.add((ap[0], agg_id))
                        if agg_id == 1 and checked < oracle_hits:
                            checked += 1
                            for i in (0, N - 1):  # sampled reports of a cached level through the oracle
                                cws = o.vidpf.decode_public_share(self.pub[psz * i:psz * (i + 1)])
                                isd = o.decode_input_share(1, self.in1[isz * i:isz * (i + 1)])
                                (_st, sh) = o.prep_init(self.vk, CTX, 1, ap, self.nonces[16 * i:16 * (i + 1)], cws, isd)
                                enc = o.test_vec_encode_prep_share(sh)
                                assert got[0][len(enc) * i:len(enc) * (i + 1)] == enc, (ap[0], i)
        finally:
            m.set_frontier_cache(False)
        assert checked == min(oracle_hits, sum(1 for h in hits if h[1] == 1))
        self.runs[key] = (hits, pairs, m, dev)
        return self.runs[key]


@pytest.fixture(scope="module")
def walks():
    """The circuits' walks, made on first use and released with the module
    (their contexts hold HBM)."""
    made = {}

    def get(pkg, name):
        if name not in made:
            made[name] = Walk(pkg, name)
        return made[name]
    yield get
    for w in made.values():
        w.runs.clear()
    made.clear()


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_walk_in_payloads_mode(mastic_amd, walks, name):
    """Every level of the sweep, both aggregators, in payloads mode: identical
    to cache-off; at least 2 hits; from the second cached call of an
    aggregator on, hits read payloads and write payloads; the first hits'
    reports 0 and n-1 equal the oracle; the sweep driver's heavy hitters."""
    from mastic_amd.heavy_hitters import compute_heavy_hitters
    w = walks(mastic_amd, name)
    (hits, pairs, m, dev) = w.run("payloads", ["payloads"], oracle_hits=3)
    assert len(hits) >= 2, hits
    assert pairs[0] == (None, "payloads") and pairs[1] == (None, "payloads")  # both aggregators' level-0 misses
    for (k, pair) in enumerate(pairs):
        # the slot a call reads was written in payloads mode, and so is the one it writes
        assert pair in ((None, "payloads"), ("payloads", "payloads")), (k, pair)
    assert ("payloads", "payloads") in pairs[2:]
    if w.hh is not None:
        m.set_frontier_cache_nodes("seeds")
        cached = []
        assert compute_heavy_hitters(m, CTX, {"default": 4}, dev, verify_key=w.vk, frontier_cache=True,
                                     cache_nodes="payloads", cached_levels=cached) == w.hh
        assert len(cached) >= 1
        assert m.last_cache_nodes()[1] == "payloads"
        assert m.set_frontier_cache_nodes() == "seeds", "the sweep leaves the mode as it found it"
        m.set_frontier_cache(False)


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_mixed_formats(mastic_amd, walks, name):
    """The mode switched before each level -- payloads, seeds, payloads, ...:
    a format change never forces a miss (every level that hit in payloads mode
    still hits), hits read one format and write the other, and every level is
    identical to cache-off."""
    w = walks(mastic_amd, name)
    (hits_p, _pairs, _m, _dev) = w.run("payloads", ["payloads"], oracle_hits=3)
    (hits, pairs, _m, _dev) = w.run("mixed", ["payloads", "seeds"])
    assert hits >= hits_p, sorted(hits_p - hits)
    assert ("seeds", "payloads") in pairs and ("payloads", "seeds") in pairs, pairs
    for (k, pair) in enumerate(pairs):
        assert pair[1] == ("payloads", "seeds")[(k // 2) % 2], (k, pair)


def _rejection_mastic(pkg, fx):
    if fx["circuit"] == "MasticSum":
        return pkg.MasticSum(fx["bits"], 255)
    return pkg.MasticHistogram(fx["bits"], 64, 8)


@pytest.mark.parametrize("force_slow", [None, 0, 3])
@pytest.mark.parametrize("fixture", ["rejection_f64.json", "rejection_f128.json"])
def test_rejection_fixture_payloads(mastic_amd, fixture, force_slow):
    """The rejection fixtures in payloads mode: level 0 is a miss that writes
    both level-0 nodes' payloads -- report B's through the real rejection on
    the exact stream (and, with force_slow_blk, through a forced handover) --
    and level 1 a hit that reads them.  Prep shares and out shares equal
    cache-off and the oracle for every report."""
    from oracle import mastic as om
    fx = json.load(open(os.path.join(GOLDEN, fixture)))
    o = om.MasticSum(fx["bits"], 255) if fx["circuit"] == "MasticSum" else om.MasticHistogram(fx["bits"], 64, 8)
    m_on, m_off = _rejection_mastic(mastic_amd, fx), _rejection_mastic(mastic_amd, fx)
    if force_slow is not None:
        for m in (m_on, m_off):
            m.set_test_hooks(force_slow_blk=force_slow)
    m_on.set_frontier_cache(True)
    assert m_on.set_frontier_cache_nodes("payloads") == "seeds"
    ctx, nonce = bytes.fromhex(fx["ctx"]), bytes.fromhex(fx["nonce"])
    reps = fx["reports"]
    n = len(reps)
    pub = bytes.fromhex("".join(r["public_share"] for r in reps))
    ins = [bytes.fromhex("".join(r["input_shares"][a] for r in reps)) for a in range(2)]
    dev_on = m_on.reports_upload(nonce * n, pub, ins[0], ins[1])
    dev_off = m_off.reports_upload(nonce * n, pub, ins[0], ins[1])
    vk = bytes.fromhex(fx["verify_key"])
    F, T = False, True
    ap0 = (0, ((F,), (T,)), False)
    ap1 = (1, ((F, F), (F, T), (T, F), (T, T)), False)
    for agg_id in range(2):
        for ap in (ap0, ap1):
            m_on.prep_init_device(dev_on, vk, ctx, agg_id, ap)
            m_off.prep_init_device(dev_off, vk, ctx, agg_id, ap)
            a = m_on.prep_result(dev_on, agg_id, ap, want_out_shares=True)
            b = m_off.prep_result(dev_off, agg_id, ap, want_out_shares=True)
            want_pair = ("payloads", "payloads") if ap is ap1 else (None, "payloads")
            assert m_on.last_cache_nodes() == want_pair, (ap[0], agg_id)
            assert a[0] == b[0] and a[2] == b[2], (ap[0], agg_id)
            psz = len(a[0]) // n
            for (i, r) in enumerate(reps):
                cws = o.vidpf.decode_public_share(bytes.fromhex(r["public_share"]))
                isd = o.decode_input_share(agg_id, bytes.fromhex(r["input_shares"][agg_id]))
                (_st, sh) = o.prep_init(vk, ctx, agg_id, ap, nonce, cws, isd)
                assert a[0][psz * i:psz * (i + 1)] == o.test_vec_encode_prep_share(sh), (ap[0], agg_id, i)
    m_on.set_frontier_cache(False)


def _full_levels(depth):
    """Levels 0 .. depth-1 with every prefix a candidate: each extends the previous one (a hit)."""
    out = []
    for level in range(depth):
        prefixes = tuple(tuple(bool((v >> (level - j)) & 1) for j in range(level + 1)) for v in range(2 << level))
        out.append((level, prefixes, level == 0))
    return out


def _small_batch(pkg, name, n, seed):
    rng = random.Random(seed)
    m_on, m_off = _mk(pkg, name), _mk(pkg, name)
    (alphas, weights, nonces, rands) = _reports(m_off, rng, n, 10)
    (pub, in0, in1) = m_off.shard_batch(CTX, alphas, weights, nonces, rands)
    vk = bytes(rng.getrandbits(8) for _ in range(16))
    return m_on, m_off, m_on.reports_upload(nonces, pub, in0, in1), m_off.reports_upload(nonces, pub, in0, in1), vk


def _same(m_on, dev_on, m_off, dev_off, vk, agg_id, ap):
    m_off.prep_init_device(dev_off, vk, CTX, agg_id, ap)
    m_on.prep_init_device(dev_on, vk, CTX, agg_id, ap)
    a = m_off.prep_result(dev_off, agg_id, ap, want_out_shares=True)
    b = m_on.prep_result(dev_on, agg_id, ap, want_out_shares=True)
    assert a[0] == b[0] and a[2] == b[2], "level %d agg %d" % (ap[0], agg_id)


def test_payloads_across_hbm_chunks(mastic_amd):
    """200 reports under an explicit memory budget of 128-report (even levels)
    or 64-report (odd levels) chunks, i.e. 2 or 4 chunks per call: the cache's
    planes hold all reports, each chunk writes and reads its columns of the
    payload-format nodes.  A miss and two hits, identical to cache-off."""
    from mastic_amd import _lib
    (m_on, m_off, dev_on, dev_off, vk) = _small_batch(mastic_amd, "Sum", 200, 4201)
    m_on.set_frontier_cache(True)
    m_on.set_frontier_cache_nodes("payloads")
    hits = 0
    try:
        for ap in _full_levels(3):
            per = m_on.work_bytes(ap) + 64 * 1024
            groups = 1 if ap[0] % 2 else 2
            _lib.lib().mastic_set_memory_budget(m_on._ctx, ctypes.c_uint64(per * 64 * groups + per * 64))
            for agg_id in range(2):
                _same(m_on, dev_on, m_off, dev_off, vk, agg_id, ap)
                hits += m_on.last_prep_was_cached()
                assert m_on.last_cache_nodes() == ("payloads" if ap[0] else None, "payloads")
    finally:
        _lib.lib().mastic_set_memory_budget(m_on._ctx, ctypes.c_uint64(0))
        m_on.set_frontier_cache(False)
    assert hits == 4, hits


def test_payloads_with_last_level_segments(mastic_amd):
    """set_last_level_segments(3) with the cache on in payloads mode: the last
    level goes into the cache addressed by parent (whole or in parent ranges,
    as the schedule decides), the next level hits on it, and every level is
    identical to cache-off."""
    (m_on, m_off, dev_on, dev_off, vk) = _small_batch(mastic_amd, "Count", N, 4202)
    m_on.set_last_level_segments(3)
    m_on.set_frontier_cache(True)
    m_on.set_frontier_cache_nodes("payloads")
    try:
        for ap in _full_levels(4):
            for agg_id in range(2):
                _same(m_on, dev_on, m_off, dev_off, vk, agg_id, ap)
                assert m_on.last_prep_was_cached() == (ap[0] > 0)
                assert m_on.last_cache_nodes() == ("payloads" if ap[0] else None, "payloads")
    finally:
        m_on.set_frontier_cache(False)
        m_on.set_last_level_segments(0)


def test_payload_slot_allocation_fallback(mastic_amd):
    """The payload-width slot's allocation fails (fail_allocs test hook): the
    call still succeeds, with seeds-format nodes or without the cache, and the
    next level's call is correct and writes payloads again.  The result
    buffers are sized beforehand by a cache-off call over the larger tree, so
    the three injected failures meet the cache's sponge-state planes, its root
    sum and then the payload-width slot."""
    (m_on, m_off, dev_on, dev_off, vk) = _small_batch(mastic_amd, "Sum", N, 4203)
    (ap0, ap1, ap2) = _full_levels(3)
    m_on.prep_init_device(dev_on, vk, CTX, 0, ap2)  # no cache yet: results of the largest tree
    m_on.set_frontier_cache(True)
    m_on.set_frontier_cache_nodes("payloads")
    try:
        m_on.set_test_hooks(fail_allocs=3)
        _same(m_on, dev_on, m_off, dev_off, vk, 0, ap0)
        assert m_on.set_test_hooks() == 0, "the injected allocation failures were not all reached"
        first = m_on.last_cache_nodes()
        assert first[0] is None and first[1] in ("seeds", None), first
        _same(m_on, dev_on, m_off, dev_off, vk, 0, ap1)
        # a hit on the seeds-format slot if the cache survived, else a miss; payloads again either way
        assert m_on.last_cache_nodes() == ("seeds" if first[1] else None, "payloads")
        assert m_on.last_prep_was_cached() == (first[1] is not None)
        _same(m_on, dev_on, m_off, dev_off, vk, 0, ap2)
        assert m_on.last_cache_nodes() == ("payloads", "payloads")
    finally:
        m_on.set_test_hooks()
        m_on.set_frontier_cache(False)


def test_auto_on_a_small_batch(mastic_amd):
    """auto: the three slots of a 150-report batch are a few MB, far inside a
    quarter of the free HBM, so every call writes payloads; identical to
    cache-off."""
    (m_on, m_off, dev_on, dev_off, vk) = _small_batch(mastic_amd, "Histogram", N, 4204)
    m_on.set_frontier_cache(True)
    assert m_on.set_frontier_cache_nodes("auto") == "seeds"
    assert m_on.set_frontier_cache_nodes() == "auto"
    try:
        for ap in _full_levels(3):
            for agg_id in range(2):
                _same(m_on, dev_on, m_off, dev_off, vk, agg_id, ap)
                assert m_on.last_cache_nodes() == ("payloads" if ap[0] else None, "payloads")
    finally:
        m_on.set_frontier_cache(False)
    assert m_on.set_frontier_cache_nodes("seeds") == "auto"
    with pytest.raises(ValueError):
        m_on.set_frontier_cache_nodes("wide")
