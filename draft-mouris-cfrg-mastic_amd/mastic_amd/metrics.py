"""Attribute-based metrics (the reference's second use case).

Mirrors ``example_attribute_based_metrics_mode`` (poc/examples.py:222-260):
one aggregation parameter whose candidate prefixes are the (hashed) attributes
the collector asks about, weight check on, and one aggregate result per
attribute.  As in the heavy-hitters sweep the work is batched, not changed:
the reports are uploaded once, each aggregator runs one ``prep_init`` over the
batch, the GPU decides every report, and the out shares are folded on the GPU.
A report that fails verification (the reference would raise at
``prep_shares_to_prep``) or replays a nonce is dropped, which is what a
deployed aggregator does.

A deployed aggregator also keeps one agg share per *batch bucket* (the
collector's time intervals, a task's fixed-size batches).  With ``groups`` the
driver returns the breakdown per bucket, from one grouped fold per aggregator
(``Mastic.aggregate_grouped``): the out shares are read once however many
buckets there are.
"""
import numpy as np

from .rounds import Round, admit, on_device, resident, unshard_raw
from .vdaf import MAX_GROUPS, NO_GROUP, Mastic


def compute_attribute_metrics(mastic: Mastic, ctx: bytes, attributes, reports, verify_key: bytes = None,
                              level: int = None, nonce_set=None, groups=None, n_groups: int = None):
    """poc/examples.py:222-260 on the GPU.

    ``attributes`` are the candidate prefixes (tuples of bools, all of length
    ``level + 1``; ``level`` defaults to ``BITS - 1``, whole attributes).
    ``reports`` is the reference's list of ``(nonce, public_share,
    input_shares)`` tuples or a device-resident
    :class:`~mastic_amd.vdaf.Reports` batch holding both input shares.
    ``verify_key`` defaults to 16 fresh random bytes (examples.py:176).
    ``nonce_set`` is the aggregator's replay protection, as in
    :func:`~mastic_amd.heavy_hitters.compute_heavy_hitters`: the batch is
    admitted first and a replayed report is dropped.

    ``groups[r]`` (one entry per report) is report r's bucket, 0 ..
    ``n_groups - 1``, or :data:`~mastic_amd.NO_GROUP` for a report outside
    every bucket; ``n_groups`` defaults to the largest bucket named, plus one.
    Without ``groups`` all reports form a single bucket.

    Returns one ``(agg_result, num_measurements)`` per bucket: ``agg_result``
    in the order of ``attributes``, unsharded with the bucket's own count.
    Rejected and replayed reports count in no bucket.
    """
    attributes = [tuple(a) for a in attributes]
    if level is None:
        level = mastic.vidpf.BITS - 1
    agg_param = (level, tuple(attributes), True)
    if not mastic.is_valid(agg_param, []):
        raise ValueError("invalid aggregation parameter")
    if verify_key is None:
        import os
        verify_key = os.urandom(16)  # gen_rand(16), examples.py:176
    (dev, n) = resident(mastic, reports)
    if groups is None:
        ids = np.zeros(n, np.uint32)
        n_groups = 1
    else:
        ids = np.ascontiguousarray(np.asarray(groups, dtype=np.uint32))
        if ids.ndim != 1 or ids.size != n:
            raise ValueError("groups has %d entries, the batch has %d reports" % (ids.size, n))
        if n_groups is None:
            named = ids[ids != NO_GROUP]
            n_groups = int(named.max()) + 1 if named.size else 1
    if not 1 <= n_groups <= MAX_GROUPS:
        raise ValueError("n_groups must be 1 .. %d" % MAX_GROUPS)

    alive = admit(nonce_set, dev, n)
    fast = on_device(mastic)
    enc = mastic.encode_agg_param(agg_param)
    if n == 0:
        empty = mastic.unshard(agg_param, [mastic.agg_init(agg_param) for _ in range(2)], 0)
        return [(list(empty), 0) for _ in range(n_groups)]
    Round(mastic, ctx, verify_key)(dev, enc, alive, weight_check=True)
    mask = alive.astype(np.uint8)
    folds = [mastic.aggregate_grouped(agg_id, enc, ids, n_groups, mask, raw=fast) for agg_id in range(2)]
    counts = np.asarray(folds[0][1])
    if not np.array_equal(counts, np.asarray(folds[1][1])):
        raise RuntimeError("the two aggregators' bucket counts differ")
    out = []
    for g in range(n_groups):
        pair = [folds[0][0][g], folds[1][0][g]]
        num = int(counts[g])
        out.append((unshard_raw(mastic, pair, num) if fast else mastic.unshard(agg_param, pair, num), num))
    return out
