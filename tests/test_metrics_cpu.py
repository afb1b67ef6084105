"""The attribute-metrics driver (mastic_amd.metrics.compute_attribute_metrics,
poc/examples.py:222-260), host logic on the CPU, with the plaintext stand-in
aggregator of tests/test_sweep.py extended by ``aggregate_grouped`` (plaintext
per-bucket sums for aggregator 0, zeros for aggregator 1) and the model nonce
set of tests/test_sweep_replays_cpu.py.  The GPU run with the real library is
in tests/test_gpu_aggregate_grouped.py."""
import hashlib

import numpy as np
import pytest

from conftest import PKG_ROOT  # noqa: F401  (puts the package on sys.path)
import mastic_amd
from mastic_amd.metrics import compute_attribute_metrics
from test_sweep import _StubMastic, index, plain_sums
from test_sweep_replays_cpu import _ModelNonceSet, _Reports

BITS = 8
NO_GROUP = mastic_amd.NO_GROUP


def h(attr):
    """examples.py:178-189: the first byte of SHA3-256 as an 8-bit index."""
    return index(hashlib.sha3_256(attr.encode("ascii")).digest()[0], BITS)


# examples.py:197-209
MEASUREMENTS = [("United States", 1), ("Greece", 1), ("United States", 2), ("Greece", 0), ("United States", 0),
                ("India", 1), ("Greece", 0), ("United States", 1), ("Greece", 1), ("Greece", 3), ("Greece", 1)]
ATTRS = ["Greece", "Mexico", "United States"]


class _Mastic(_StubMastic):
    """The stand-in with the grouped fold: bucket g's share is the plaintext
    sums over the unmasked reports whose id is g."""

    def aggregate_grouped(self, agg_id, agg_param, groups, n_groups, valid=None, raw=False):
        assert not raw and len(groups) == self._dev.n and (valid is None or len(valid) == self._dev.n)
        assert all(g < n_groups or g == NO_GROUP for g in groups)
        keep = [True] * self._dev.n if valid is None else [bool(v) for v in valid]
        shares, counts = [], np.zeros(n_groups, np.uint64)
        for g in range(n_groups):
            meas = [m for (m, k, gi) in zip(self._dev.meas, keep, groups) if k and gi == g]
            counts[g] = len(meas)
            shares.append(plain_sums(meas, agg_param[1]) if agg_id == 0 else [0] * len(agg_param[1]))
        self.grouped_calls = getattr(self, "grouped_calls", 0) + 1
        return (shares, counts)


def _batch(meas=MEASUREMENTS, nonces=None):
    rows = [(h(a), v) for (a, v) in meas]
    return _Reports(rows, nonces if nonces is not None else [i.to_bytes(16, "big") for i in range(len(rows))])


def _plain(meas):
    return plain_sums([(h(a), v) for (a, v) in meas], [h(a) for a in ATTRS])


def test_election_example_ungrouped():
    m = _Mastic(BITS)
    out = compute_attribute_metrics(m, b"ctx", [h(a) for a in ATTRS], _batch(), verify_key=bytes(32))
    assert out == [([6, 0, 4], len(MEASUREMENTS))]
    assert m.calls == [(0, BITS - 1, 3), (1, BITS - 1, 3)]  # one prep_init per aggregator, whole attributes
    assert m.grouped_calls == 2                             # and one fold per aggregator


def test_two_buckets_sum_to_the_whole():
    groups = [i % 2 for i in range(len(MEASUREMENTS))]
    out = compute_attribute_metrics(_Mastic(BITS), b"ctx", [h(a) for a in ATTRS], _batch(), verify_key=bytes(32),
                                    groups=groups, n_groups=2)
    assert len(out) == 2
    for g in range(2):
        part = [m for (m, gi) in zip(MEASUREMENTS, groups) if gi == g]
        assert out[g] == (_plain(part), len(part))
    assert [a + b for (a, b) in zip(out[0][0], out[1][0])] == [6, 0, 4]
    assert out[0][1] + out[1][1] == len(MEASUREMENTS)
    assert out[0][0] != out[1][0]  # the split is not trivial


def test_n_groups_defaults_to_the_buckets_named_and_empty_buckets_are_zero():
    groups = [3 if i < 4 else 0 for i in range(len(MEASUREMENTS))]
    out = compute_attribute_metrics(_Mastic(BITS), b"ctx", [h(a) for a in ATTRS], _batch(), verify_key=bytes(32),
                                    groups=groups)
    assert len(out) == 4
    assert out[1] == ([0, 0, 0], 0) and out[2] == ([0, 0, 0], 0)
    assert out[3] == (_plain(MEASUREMENTS[:4]), 4) and out[0] == (_plain(MEASUREMENTS[4:]), 7)


def test_replayed_and_rejected_reports_count_in_no_bucket():
    # report 11 replays report 1's nonce (Greece, 1 again); report 9 (Greece, 3) fails decide
    meas = MEASUREMENTS + [("Greece", 1)]
    nonces = [i.to_bytes(16, "big") for i in range(len(MEASUREMENTS))] + [(1).to_bytes(16, "big")]
    groups = [i % 2 for i in range(len(meas))]
    ns = _ModelNonceSet()
    out = compute_attribute_metrics(_Mastic(BITS, bad=(9,)), b"ctx", [h(a) for a in ATTRS], _batch(meas, nonces),
                                    verify_key=bytes(32), nonce_set=ns, groups=groups, n_groups=2)
    assert ns.calls == 1
    for g in range(2):
        part = [m for (i, (m, gi)) in enumerate(zip(meas, groups)) if gi == g and i not in (9, 11)]
        assert out[g] == (_plain(part), len(part))
    assert [a + b for (a, b) in zip(out[0][0], out[1][0])] == [3, 0, 4]
    assert out[0][1] + out[1][1] == len(MEASUREMENTS) - 1
    # ungrouped: the same reports are dropped from the single bucket
    out1 = compute_attribute_metrics(_Mastic(BITS, bad=(9,)), b"ctx", [h(a) for a in ATTRS], _batch(meas, nonces),
                                     verify_key=bytes(32), nonce_set=_ModelNonceSet())
    assert out1 == [([3, 0, 4], len(MEASUREMENTS) - 1)]


def test_no_group_reports_are_excluded():
    groups = [NO_GROUP if i in (0, 9) else i % 2 for i in range(len(MEASUREMENTS))]
    out = compute_attribute_metrics(_Mastic(BITS), b"ctx", [h(a) for a in ATTRS], _batch(), verify_key=bytes(32),
                                    groups=groups, n_groups=2)
    for g in range(2):
        part = [m for (m, gi) in zip(MEASUREMENTS, groups) if gi == g]
        assert out[g] == (_plain(part), len(part))
    assert [a + b for (a, b) in zip(out[0][0], out[1][0])] == [3, 0, 3]  # without (US, 1) and (Greece, 3)
    assert out[0][1] + out[1][1] == len(MEASUREMENTS) - 2


def test_wrong_groups_length_and_group_count_raise():
    attrs = [h(a) for a in ATTRS]
    with pytest.raises(ValueError):
        compute_attribute_metrics(_Mastic(BITS), b"ctx", attrs, _batch(), verify_key=bytes(32),
                                  groups=[0] * (len(MEASUREMENTS) - 1), n_groups=1)
    with pytest.raises(ValueError):
        compute_attribute_metrics(_Mastic(BITS), b"ctx", attrs, _batch(), verify_key=bytes(32),
                                  groups=[0] * (len(MEASUREMENTS) + 1))
    for bad in (0, 65537):
        with pytest.raises(ValueError):
            compute_attribute_metrics(_Mastic(BITS), b"ctx", attrs, _batch(), verify_key=bytes(32),
                                      groups=[0] * len(MEASUREMENTS), n_groups=bad)


def test_empty_batch_gives_zero_buckets():
    out = compute_attribute_metrics(_Mastic(BITS), b"ctx", [h(a) for a in ATTRS], [], verify_key=bytes(32),
                                    groups=[], n_groups=2)
    assert out == [([0, 0, 0], 0), ([0, 0, 0], 0)]
