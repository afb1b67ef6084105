"""mastic_aggregate_grouped / Mastic.aggregate_grouped on the GPU: one agg
share per batch bucket from one pass over the out shares (k_fold_grouped).

The expected value never comes from the code under test: the out shares of
each aggregator are fetched with prep_result(want_out_shares=True) and summed
per group with Python integers mod p.  Out shares are pseudo-random field
elements, so the sums wrap (asserted).  Tiny trees (BITS = 4, level 3, five
prefixes, weight check on), both fields, both aggregators; the batch sizes
are one report, less than a workgroup's stride of 1,024, more than it, and
8,453: the smallest convenient size above 2 x 4,096 reports, where the plan
(csrc/group_fold.hpp) splits these row counts into two report chunks (checked
on the host in tests/host/group_fold_host.cpp), and no multiple of 256.
One prep_init per (field, n) is shared by the cases and left unchanged."""
import ctypes
import functools
import hashlib
import random

import numpy as np
import pytest

from conftest import PKG_ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

BITS = 4
CTX = b"grouped fold"
FIELDS = {"Field64": ("Sum", dict(max_measurement=7)), "Field128": ("Histogram", dict(length=3, chunk_length=2))}
SIZES = [1, 150, 1100, 8453]
NONE = 0xFFFFFFFF


class _Batch:
    """n resident reports, both aggregators' prep_init results live in the
    ctx, and the out shares as Python integers: per[agg_id][r][row]."""

    def __init__(self, field, n):
        import mastic_amd
        (circuit, kw) = FIELDS[field]
        self.m = m = mastic_amd.Mastic(BITS, circuit, **kw)
        self.n = n
        rng = random.Random(n * 7 + len(field))
        vals = [rng.randrange(2 ** BITS) for _ in range(n)]
        alphas = b"".join((v << (8 - BITS)).to_bytes(1, "big") for v in vals)
        meas = [rng.randrange(8 if circuit == "Sum" else 3) for _ in range(n)]
        betas = b"".join(m.field.encode_vec(m.encode_measurement(x)) for x in meas)
        self.dev = m.reports_shard(CTX, alphas, betas, rng.randbytes(16 * n), rng.randbytes(m.RAND_SIZE * n))
        cand = tuple(tuple(bool((v >> (BITS - 1 - i)) & 1) for i in range(BITS)) for v in (1, 4, 7, 10, 13))
        self.enc = m.encode_agg_param((BITS - 1, cand, True))
        self.rows = len(cand) * (1 + m.OUTPUT_LEN)
        self.p = m.field.MODULUS
        self.esz = m.field.ENCODED_SIZE
        self.share = self.rows * self.esz
        self.per = []
        for agg_id in range(2):
            m.prep_init_device(self.dev, bytes(range(16)), CTX, agg_id, self.enc)
            (_ps, _js, out, st) = m.prep_result(self.dev, agg_id, self.enc, want_out_shares=True)
            assert list(st) == [0] * n
            el = [int.from_bytes(out[i:i + self.esz], "little") for i in range(0, len(out), self.esz)]
            self.per.append([el[r * self.rows:(r + 1) * self.rows] for r in range(n)])

    def want(self, agg_id, groups, n_groups, valid=None, raw_sums=None):
        """{g: share bytes} of the non-empty groups and the counts, from Python integers."""
        sums, counts = {}, np.zeros(n_groups, np.uint64)
        for r in range(self.n):
            g = int(groups[r])
            if g == NONE or (valid is not None and not valid[r]):
                continue
            acc = sums.setdefault(g, [0] * self.rows)
            for (i, x) in enumerate(self.per[agg_id][r]):
                acc[i] += x
            counts[g] += 1
        if raw_sums is not None:
            raw_sums.extend(x for acc in sums.values() for x in acc)
        return ({g: b"".join((x % self.p).to_bytes(self.esz, "little") for x in acc) for (g, acc) in sums.items()},
                counts)

    def check(self, agg_id, groups, n_groups, valid=None, raw_sums=None):
        (shares, counts) = self.m.aggregate_grouped(agg_id, self.enc, groups, n_groups, valid, raw=True)
        (want, want_counts) = self.want(agg_id, groups, n_groups, valid, raw_sums)
        assert len(shares) == n_groups and counts.dtype == np.uint64
        assert list(counts) == list(want_counts)
        zeros = bytes(self.share)
        for g in range(n_groups):
            assert shares[g] == want.get(g, zeros), "group %d" % g
        return shares


@functools.lru_cache(maxsize=None)
def _batch(field, n):
    return _Batch(field, n)


@pytest.fixture(scope="module", autouse=True)
def _drop_batches():
    yield
    _batch.cache_clear()  # the contexts go with the module, not at interpreter exit


GRID = pytest.mark.parametrize("n", SIZES)
BOTH = pytest.mark.parametrize("field", list(FIELDS))


@BOTH
@GRID
def test_one_group_is_the_ungrouped_fold(field, n):
    b = _batch(field, n)
    for agg_id in range(2):
        raw = []
        (share,) = b.check(agg_id, np.zeros(n, np.uint32), 1, raw_sums=raw)
        assert share == b.m.aggregate_device(agg_id, b.enc, raw=True)
        if n >= 150:
            assert any(x >= b.p for x in raw), "the sums wrapped mod p"
    # decoded form: field vectors, as aggregate_device returns them
    (vecs, _counts) = b.m.aggregate_grouped(0, b.enc, np.zeros(n, np.uint32), 1)
    assert b.m.field.encode_vec(vecs[0]) == b.m.aggregate_device(0, b.enc, raw=True)


@BOTH
@GRID
def test_three_groups_empty_single_none_and_mask(field, n):
    """Group 1 empty, group 2 only the last report, about a tenth of the
    reports in no group and about 30 % masked, all at once; each group's share
    also equals the ungrouped fold under that group's mask."""
    b = _batch(field, n)
    rng = random.Random(n + 1)
    groups = np.array([NONE if rng.random() < 0.1 else 0 for _ in range(n)], np.uint32)
    valid = np.array([rng.random() >= 0.3 for _ in range(n)], np.uint8)
    groups[n - 1] = 2
    valid[n - 1] = 1
    if n > 1:
        assert (groups == NONE).any() and (valid == 0).any() and (groups[valid == 0] == 0).any()
    for agg_id in range(2):
        shares = b.check(agg_id, groups, 3, valid)
        (_w, counts) = b.want(agg_id, groups, 3, valid)
        assert counts[1] == 0 and counts[2] == 1 and shares[1] == bytes(b.share)
        assert shares[2] == b"".join(x.to_bytes(b.esz, "little") for x in b.per[agg_id][n - 1])
        for g in range(3):
            mask = ((groups == g) & (valid != 0)).astype(np.uint8)
            assert shares[g] == b.m.aggregate_device(agg_id, b.enc, mask, raw=True)
    # without the mask the masked reports are back
    b.check(0, groups, 3)


@BOTH
@GRID
def test_64_groups_random_ids(field, n):
    b = _batch(field, n)
    rng = random.Random(n + 2)
    groups = np.array([rng.randrange(64) for _ in range(n)], np.uint32)
    for agg_id in range(2):
        raw = []
        b.check(agg_id, groups, 64, raw_sums=raw)
        if n >= 1100:
            assert any(x >= b.p for x in raw)


@BOTH
@GRID
def test_64_groups_time_ordered_runs(field, n):
    """Ids in runs of 100 reports: run boundaries fall inside waves, whole
    waves share one id (every lane of a wave adds into one group)."""
    b = _batch(field, n)
    groups = np.array([(r // 100) % 64 for r in range(n)], np.uint32)
    valid = np.ones(n, np.uint8)
    valid[::7] = 0
    for agg_id in range(2):
        b.check(agg_id, groups, 64)
    b.check(1, groups, 64, valid)


@BOTH
def test_65536_groups_many_passes(field):
    """More groups than one pass holds (16 passes Field64, 32 Field128), nearly
    all of them empty; ids include the first and the last group."""
    b = _batch(field, 150)
    rng = random.Random(5)
    groups = np.array([rng.randrange(65536) for _ in range(150)], np.uint32)
    groups[0], groups[1], groups[2], groups[3] = 0, 65535, 4095, 4096  # both ends and a pass boundary
    groups[10] = NONE
    for agg_id in range(2):
        b.check(agg_id, groups, 65536)


def _raw_call(b, agg_id, groups, n_groups, out, counts, m=None):
    from mastic_amd import _lib
    return _lib.lib().mastic_aggregate_grouped((m or b.m)._ctx, agg_id, _lib.buf(groups), n_groups, None,
                                               _lib.buf(out), _lib.buf(counts))


@BOTH
def test_einval_leaves_the_output_untouched(field):
    import mastic_amd
    b = _batch(field, 150)
    n = b.n
    zeros = np.zeros(n, np.uint32)
    bad = zeros.copy()
    bad[17] = 3
    bad[40] = 9
    (circuit, kw) = FIELDS[field]
    fresh = mastic_amd.Mastic(BITS, circuit, **kw)
    cases = [("id == n_groups", b.m, 0, bad, 3), ("n_groups 0", b.m, 0, zeros, 0),
             ("n_groups 65537", b.m, 0, zeros, 65537), ("no prep result", fresh, 0, zeros, 1),
             ("agg_id 2", b.m, 2, zeros, 1)]
    for (name, m, agg_id, groups, n_groups) in cases:
        out = np.full(4 * b.share, 0xA5, np.uint8)
        counts = np.full(4, 0x5A5A5A5A, np.uint64)
        rc = _raw_call(b, agg_id, groups, n_groups, out, counts, m)
        assert rc == -22, name
        assert (out == 0xA5).all() and (counts == 0x5A5A5A5A).all(), name
    # the message names the first offending report
    rc = _raw_call(b, 0, bad, 3, np.zeros(3 * b.share, np.uint8), np.zeros(3, np.uint64))
    from mastic_amd import _lib
    assert rc == -22 and b"report 17" in _lib.lib().mastic_last_error(b.m._ctx)
    # the Python method: a wrong length never reaches the library, the library's EINVAL is a ValueError
    with pytest.raises(ValueError, match="entries"):
        b.m.aggregate_grouped(0, b.enc, np.zeros(n - 1, np.uint32), 1)
    with pytest.raises(ValueError):
        b.m.aggregate_grouped(0, b.enc, bad, 3)
    with pytest.raises(ValueError):
        b.m.aggregate_grouped(0, b.enc, zeros, 0)
    # and the prep result is still there
    b.check(0, zeros, 1)


@BOTH
def test_enomem_then_the_same_call_succeeds(field):
    from mastic_amd import MasticError
    b = _batch(field, 1100)
    rng = random.Random(9)
    groups = np.array([rng.randrange(5) for _ in range(b.n)], np.uint32)
    valid = np.array([rng.random() < 0.9 for _ in range(b.n)], np.uint8)
    b.m.set_test_hooks(fail_allocs=1)
    try:
        with pytest.raises(MasticError) as e:
            b.m.aggregate_grouped(1, b.enc, groups, 5, valid, raw=True)
        assert e.value.code == -12
        b.check(1, groups, 5, valid)
    finally:
        b.m.set_test_hooks()
    assert b.check(1, np.zeros(b.n, np.uint32), 1)[0] == b.m.aggregate_device(1, b.enc, raw=True)


@BOTH
def test_grouped_result_merges_like_a_single_share(field):
    """Multi-rank needs no new collective: the n_groups x rows vector goes
    through mastic_merge_host as one share (world 1: unchanged)."""
    b = _batch(field, 150)
    groups = np.array([r % 6 for r in range(b.n)], np.uint32)
    (shares, _counts) = b.m.aggregate_grouped(0, b.enc, groups, 6, raw=True)
    blob = b"".join(shares)
    assert b.m.merge_host(blob, 1, 6 * b.rows) == blob
    # two ranks' worth, merged on the host side of the same call: group-wise field sums
    (other, _c) = b.m.aggregate_grouped(1, b.enc, groups, 6, raw=True)
    both = b.m.merge_host(blob + b"".join(other), 2, 6 * b.rows)
    (w0, _) = b.want(0, groups, 6)
    (w1, _) = b.want(1, groups, 6)
    for g in range(6):
        a0 = [int.from_bytes(w0[g][i:i + b.esz], "little") for i in range(0, b.share, b.esz)]
        a1 = [int.from_bytes(w1[g][i:i + b.esz], "little") for i in range(0, b.share, b.esz)]
        assert both[g * b.share:(g + 1) * b.share] == b"".join(((x + y) % b.p).to_bytes(b.esz, "little")
                                                                for (x, y) in zip(a0, a1))


def test_attribute_metrics_two_buckets_one_tampered_report():
    """compute_attribute_metrics with the real library on the reference's
    election example (poc/examples.py:172-260), split into two buckets.  One
    extra report is tampered with as tests/test_gpu_decide_rejects.py does to
    a verifier element, one step earlier: element 0 of the leader's proof
    share becomes element + 1 mod p, so the FLP decides false and the report
    counts in no bucket."""
    import mastic_amd
    from mastic_amd.metrics import compute_attribute_metrics
    bits = 8
    ctx = b"example_attribute_based_metrics_mode"
    m = mastic_amd.MasticSum(bits, 3)

    def h(attr):
        return m.vidpf.test_index_from_int(hashlib.sha3_256(attr.encode("ascii")).digest()[0], bits)

    measurements = [("United States", 1), ("Greece", 1), ("United States", 2), ("Greece", 0),
                    ("United States", 0), ("India", 1), ("Greece", 0), ("United States", 1),
                    ("Greece", 1), ("Greece", 3), ("Greece", 1)]
    attrs = ["Greece", "Mexico", "United States"]
    rng = random.Random(7)
    reports = []
    for (a, v) in measurements + [("Greece", 2)]:
        nonce = rng.randbytes(16)
        (pub, ins) = m.shard(ctx, (h(a), v), nonce, rng.randbytes(m.RAND_SIZE))
        reports.append((nonce, pub, [m.test_vec_encode_input_share(s) for s in ins]))
    honest = compute_attribute_metrics(m, ctx, [h(a) for a in attrs], reports[:-1], verify_key=bytes(range(16)))
    assert honest == [([6, 0, 4], 11)]
    # untampered, the twelfth report counts: (Greece, 2)
    assert compute_attribute_metrics(m, ctx, [h(a) for a in attrs], reports) == [([8, 0, 4], 12)]
    (nonce, pub, ins) = reports[-1]
    leader = bytearray(ins[0])
    esz = m.field.ENCODED_SIZE
    x = int.from_bytes(leader[16:16 + esz], "little")
    leader[16:16 + esz] = ((x + 1) % m.field.MODULUS).to_bytes(esz, "little")
    reports[-1] = (nonce, pub, [bytes(leader), ins[1]])
    groups = [i % 2 for i in range(len(reports))]
    out = compute_attribute_metrics(m, ctx, [h(a) for a in attrs], reports, groups=groups, n_groups=2)
    plain = []
    for g in range(2):
        part = [mv for (i, mv) in enumerate(measurements) if groups[i] == g]  # the tampered report is index 11
        plain.append(([sum(v for (a, v) in part if a == attr) for attr in attrs], len(part)))
    assert out == plain
    assert [a + b for (a, b) in zip(out[0][0], out[1][0])] == [6, 0, 4] and out[0][1] + out[1][1] == 11
    # a replayed batch adds nothing: the nonce set keeps none of its reports
    ns = mastic_amd.NonceSet(m)
    first = compute_attribute_metrics(m, ctx, [h(a) for a in attrs], reports, nonce_set=ns, groups=groups, n_groups=2)
    again = compute_attribute_metrics(m, ctx, [h(a) for a in attrs], reports, nonce_set=ns, groups=groups, n_groups=2)
    assert first == plain and again == [([0, 0, 0], 0), ([0, 0, 0], 0)]
