"""Compacting a resident batch in place (``Reports.compact``,
``mastic_reports_compact``): the kept reports, in their order, become reports
0..k-1 of the same HBM, for every segment and the wire-check verdicts.

Every expected value comes from a host filter of what was uploaded, or from a
second context given a fresh upload of only the kept reports; never from the
code under test.

Shapes.  The circuits are chosen so that the rows of a batch (16-byte nonces,
public shares, both input shares) take every residue mod 4 and odd as well as
even sizes, asserted below from ``mastic.sizes`` itself: source and destination
of a moved row then differ in alignment from row to row.  n = 1, 63, 64, 65
are the wave edges, 4099 is more than one workgroup for every segment.  The
staging sizes of one row and three rows force staged tiles and plans of many
tiles at these n; 0 is the default (everything direct or one staged tile).
"""
import random

import numpy as np
import pytest

from test_gpu_parity import CTX, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

CIRCUITS = {
    "count1": ("MasticCount", (1,)),
    "count5": ("MasticCount", (5,)),
    "count9": ("MasticCount", (9,)),
    "sum255-bits1": ("MasticSum", (1, 255)),
    "hist-field128": ("MasticHistogram", (2, 4, 2)),
}
SIZES = [1, 63, 64, 65, 4099]
STATUS_NONCANONICAL = -3


@pytest.fixture(scope="module")
def circuits(mastic_amd):  # noqa: F811
    return {name: getattr(mastic_amd, cls)(*args) for (name, (cls, args)) in CIRCUITS.items()}


def _row_sizes(m):
    return [16, m.sizes.public_share_size, m.sizes.input_share_size[0], m.sizes.input_share_size[1]]


def _masks(n, rng):
    yield ("random", rng.random(n) < 0.5)
    yield ("all kept", np.ones(n, bool))
    yield ("none kept", np.zeros(n, bool))
    k = np.ones(n, bool)
    k[0] = False
    yield ("only the first dropped", k)
    k = np.zeros(n, bool)
    k[n - 1] = True
    yield ("only the last kept", k)
    yield ("alternating", np.arange(n) % 2 == 1)
    k = np.ones(n, bool)
    k[n // 3:n // 3 + max(1, n // 4)] = False
    yield ("a dropped run inside a kept run", k)


def _download(rep, with_in1=True):
    """The batch's rows as [nonces, pub, in0, in1] byte matrices (Reports.download
    insists on both input shares)."""
    from mastic_amd import _lib
    m, n = rep._m, rep.n
    bufs = [np.empty((n, rb), np.uint8) for rb in _row_sizes(m)]
    args = [_lib.buf(b) for b in bufs]
    if not with_in1:
        args[3] = None
    rc = _lib.lib().mastic_reports_download(rep._ptr, *args)
    assert rc == 0, rc
    return bufs if with_in1 else bufs[:3]


def test_row_sizes_cover_every_alignment(circuits):
    sizes = set()
    for m in circuits.values():
        sizes |= set(_row_sizes(m))
    assert {s % 4 for s in sizes} == {0, 1, 2, 3}, sorted(sizes)
    assert {(s % 16) % 2 for s in sizes} == {0, 1}, sorted(sizes)
    # the three Counts' public shares alone take residues 1, 2 and 3 (65, 322 and 579 bytes)
    assert {circuits[n].sizes.public_share_size % 4 for n in ("count1", "count5", "count9")} == {1, 2, 3}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_round_trip_equals_the_host_filter(circuits, name, n):
    m = circuits[name]
    rng = np.random.default_rng(n * 31 + len(name))
    rows = [rng.integers(0, 256, size=(n, rb), dtype=np.uint8) for rb in _row_sizes(m)]
    widest = max(_row_sizes(m))
    for (what, keep) in _masks(n, rng):
        for staging in (0, widest, 3 * widest):
            rep = m.reports_upload(*[r.tobytes() for r in rows])
            assert rep.compact(keep, staging) == int(keep.sum()) == rep.n
            for (seg, (g, r)) in enumerate(zip(_download(rep), rows)):
                assert np.array_equal(g, r[keep]), (name, n, what, staging, "segment %d" % seg)


@pytest.mark.parametrize("n", [65, 4099])
def test_batch_without_helper_shares(circuits, n):
    m = circuits["count5"]
    rng = np.random.default_rng(n)
    rows = [rng.integers(0, 256, size=(n, rb), dtype=np.uint8) for rb in _row_sizes(m)[:3]]
    keep = rng.random(n) < 0.6
    rep = m.reports_upload(rows[0].tobytes(), rows[1].tobytes(), rows[2].tobytes(), None)
    assert rep.compact(keep, 2 * max(_row_sizes(m))) == int(keep.sum())
    for (g, r) in zip(_download(rep, with_in1=False), rows):
        assert np.array_equal(g, r[keep])
    # the allocations stay: a later upload of n_kept rows works
    rep.upload(*[r[:rep.n].tobytes() for r in rows], None)
    for (g, r) in zip(_download(rep, with_in1=False), rows):
        assert np.array_equal(g, r[:rep.n])


# ----------------------------------------------------------- real reports
def _pack_alphas(alphas):
    return bytes(sum(int(b) << (7 - i) for (i, b) in enumerate(a[:8])) & 0xff for a in alphas)


class _Job:
    """70 Sum reports (bits 5, weights 0..3) with, among them: replays of
    earlier reports, encodings of an out-of-range weight, a seed correction
    word corrupted at level 0 and one at level 1."""

    N = 70
    REPLAYS = {9: 2, 33: 32, 34: 2, 64: 63, 69: 0}   # row -> the earlier row it repeats
    BAD_WEIGHT = (5, 40, 65)
    BAD_CW0 = 17
    BAD_CW1 = 50

    def __init__(self, mastic_amd):
        self.m = m = mastic_amd.MasticSum(5, 3)
        rng = random.Random(4242)
        n = self.N
        self.alphas = [tuple(bool(rng.getrandbits(1)) for _ in range(5)) for _ in range(n)]
        self.weights = [rng.randrange(4) for _ in range(n)]
        F = m.field
        bad = [F(1), F(1), F(0), F(1)]  # 3 with inconsistent offset bits (test_invalid_weight_rejected_by_flp)
        betas = b"".join(F.encode_vec(bad if i in self.BAD_WEIGHT else m.encode_measurement(self.weights[i]))
                         for i in range(n))
        nonces = rng.randbytes(16 * n)
        (pub, in0, in1) = m.shard_encoded(CTX, n, _pack_alphas(self.alphas), betas, nonces,
                                          rng.randbytes(m.RAND_SIZE * n))
        seg = [np.frombuffer(b, np.uint8).reshape(n, -1).copy() for b in (nonces, pub, in0, in1)]
        for (i, level) in ((self.BAD_CW0, 0), (self.BAD_CW1, 1)):
            nctrl = (2 * 5 + 7) // 8
            seg[1][i, nctrl + 16 * level] ^= 1  # the seed correction word of that level
        for (dst, src) in self.REPLAYS.items():
            for s in seg:
                s[dst] = s[src]
        self.seg = seg
        self.vk = rng.randbytes(32)
        fresh = np.ones(n, bool)
        fresh[list(self.REPLAYS)] = False
        ok0 = np.ones(n, bool)
        for i in self.BAD_WEIGHT + (self.BAD_CW0,):
            ok0[i] = False
        for (dst, src) in self.REPLAYS.items():
            ok0[dst] = ok0[src]
        self.fresh, self.ok0 = fresh, ok0
        self.keep = fresh & ok0  # what the model says survives the admit and level 0

    def upload(self, m, rows=None):
        seg = self.seg if rows is None else [s[rows] for s in self.seg]
        return m.reports_upload(*[s.tobytes() for s in seg])


@pytest.fixture(scope="module")
def job(mastic_amd):  # noqa: F811
    return _Job(mastic_amd)


AP0 = (0, ((False,), (True,)), True)
AP1 = (1, ((False, False), (False, True), (True, False), (True, True)), False)


def _level(m, rep, vk, ap):
    """Both aggregators' prep_init, decide and fold at one level."""
    res = []
    for a in range(2):
        m.prep_init_device(rep, vk, CTX, a, ap)
    for a in range(2):
        res.append(m.prep_result(rep, a, ap, want_out_shares=True))
    (accept, codes) = m.decide_results(CTX, rep.n)
    aggs = [m.aggregate_device(a, ap, accept, raw=True) for a in range(2)]
    return (res, accept, codes, aggs)


def test_compacted_batch_equals_a_fresh_upload_of_the_kept_reports(mastic_amd, job):  # noqa: F811
    from mastic_amd import NonceSet
    m = job.m
    rep = job.upload(m)
    admit = NonceSet(m).admit(rep) == 1
    assert admit.tolist() == job.fresh.tolist()
    (_res, accept0, _codes, _aggs) = _level(m, rep, job.vk, AP0)
    assert (accept0 == 1).tolist() == job.ok0.tolist()
    keep = admit & (accept0 == 1)
    assert rep.compact(keep) == int(job.keep.sum()) == 70 - 5 - 4
    got = _level(m, rep, job.vk, AP1)

    m2 = mastic_amd.MasticSum(5, 3)
    rep2 = job.upload(m2, job.keep)
    want = _level(m2, rep2, job.vk, AP1)
    for a in range(2):
        assert got[0][a][0] == want[0][a][0], "prep shares of aggregator %d" % a
        assert got[0][a][2] == want[0][a][2], "out shares of aggregator %d" % a
        assert np.array_equal(got[0][a][3], want[0][a][3])
        assert got[3][a] == want[3][a], "agg share of aggregator %d" % a
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    # the report corrupted at level 1 survived level 0 and is rejected now, at its new index
    kept_rows = np.nonzero(job.keep)[0]
    assert (got[1] == 1).tolist() == [int(i) != job.BAD_CW1 for i in kept_rows]
    shares = [m.field.decode_vec(s) for s in got[3]]
    plain = [sum(job.weights[i] for i in kept_rows if i != job.BAD_CW1 and job.alphas[i][:2] == p) for p in AP1[1]]
    assert m.unshard(AP1, shares, int((got[1] == 1).sum())) == plain


def test_noncanonical_verdict_travels_with_its_report(mastic_amd):  # noqa: F811
    m = mastic_amd.MasticSum(5, 13)
    rng = random.Random(99)
    n, k = 65, 40
    alphas = [tuple(bool(rng.getrandbits(1)) for _ in range(5)) for _ in range(n)]
    weights = [rng.randrange(14) for _ in range(n)]
    nonces = rng.randbytes(16 * n)
    (pub, in0, in1) = m.shard_batch(CTX, alphas, weights, nonces, rng.randbytes(m.RAND_SIZE * n))
    enc, vl = m.field.ENCODED_SIZE, m.VALUE_LEN
    at = m.public_share_size() * k + (2 * 5 + 7) // 8 + 16 * 5 + (3 * vl + 0) * enc  # payload CW of level 3
    pub = pub[:at] + m.field.MODULUS.to_bytes(enc, "little") + pub[at + enc:]
    rep = m.reports_upload(nonces, pub, in0, in1)
    ap = (2, tuple(dict.fromkeys(a[:3] for a in alphas[:3])), False)
    vk = bytes(32)

    def statuses():
        out = []
        for a in range(2):
            m.prep_init_device(rep, vk, CTX, a, ap)
            out.append(m.prep_result(rep, a, ap)[3].tolist())
        return out

    assert statuses() == [[STATUS_NONCANONICAL if i == k else 0 for i in range(n)]] * 2
    keep = np.ones(n, bool)
    keep[[0, 7, 39, 60]] = False
    assert rep.compact(keep, m.public_share_size()) == n - 4
    assert statuses() == [[STATUS_NONCANONICAL if i == k - 3 else 0 for i in range(n - 4)]] * 2


@pytest.mark.parametrize("drop", [True, False], ids=["one dropped: miss", "none dropped: hit"])
def test_frontier_cache_sees_a_compaction(mastic_amd, job, drop):  # noqa: F811
    m_on, m_off = mastic_amd.MasticSum(5, 3), job.m  # (job.m: another context, its cache off)
    m_on.set_frontier_cache(True)
    rows = np.nonzero(job.keep)[0]  # honest, fresh reports
    keep = np.ones(len(rows), bool)
    if drop:
        keep[11] = False
    rep = job.upload(m_on, rows)
    for a in range(2):
        m_on.prep_init_device(rep, job.vk, CTX, a, AP0)
        assert not m_on.last_prep_was_cached()
    assert rep.compact(keep) == int(keep.sum())
    got = []
    for a in range(2):
        m_on.prep_init_device(rep, job.vk, CTX, a, AP1)
        assert m_on.last_prep_was_cached() == (not drop)
        got.append(m_on.prep_result(rep, a, AP1, want_out_shares=True))
    rep_off = job.upload(m_off, rows[keep])
    for a in range(2):
        m_off.prep_init_device(rep_off, job.vk, CTX, a, AP1)
        want = m_off.prep_result(rep_off, a, AP1, want_out_shares=True)
        assert got[a][0] == want[0] and got[a][2] == want[2] and np.array_equal(got[a][3], want[3])
    m_on.set_frontier_cache(False)


def test_errors_and_failure_atomicity(mastic_amd, job):  # noqa: F811
    from mastic_amd import MasticError
    m = job.m
    rep = job.upload(m)
    with pytest.raises(MasticError) as e:
        rep.view(3, 20).compact(np.ones(20, bool))
    assert e.value.code == -22 and "view" in str(e.value)
    with pytest.raises(MasticError) as e:
        rep.compact(None)
    assert e.value.code == -22
    from mastic_amd import _lib
    assert _lib.lib().mastic_reports_compact(rep._ptr, None, 0, None) == -22
    before = _download(rep)
    keep = np.arange(job.N) % 3 != 0
    m.set_test_hooks(fail_allocs=1)
    with pytest.raises(MasticError) as e:
        rep.compact(keep)
    assert e.value.code == -12
    assert m.set_test_hooks() == 0, "the injected allocation failure was not reached"
    assert rep.n == job.N
    for (g, b) in zip(_download(rep), before):
        assert np.array_equal(g, b)
    assert rep.compact(keep) == int(keep.sum())  # the same call then succeeds
    for (g, b) in zip(_download(rep), before):
        assert np.array_equal(g, b[keep])


def test_empty_batch_and_a_mask_that_keeps_nothing(mastic_amd, job):  # noqa: F811
    from mastic_amd.heavy_hitters import compute_heavy_hitters
    m = job.m
    empty = m.reports_upload(b"", b"", b"", b"")
    assert empty.compact(np.zeros(0, bool)) == 0 and empty.n == 0
    rep = job.upload(m)
    assert rep.compact(np.zeros(job.N, bool)) == 0 and rep.n == 0
    trace = []
    assert compute_heavy_hitters(m, CTX, {"default": 1}, rep, verify_key=job.vk, trace=trace) == []
    assert trace[0].agg_result == [0, 0] and trace[0].n_valid == 0
