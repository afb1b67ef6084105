"""Weighted heavy-hitters level sweep.

Mirrors the reference driver ``compute_heavy_hitters`` (poc/examples.py:37-91)
and ``get_threshold`` (poc/examples.py:26-34): walk the prefix tree level by
level, keep the children of every candidate whose aggregate reaches its
threshold, report the surviving full-length prefixes.

Differences from the reference loop, all in how the work is batched, not in
what is computed:
  * the reports are uploaded to HBM once and every level runs as one batched
    ``prep_init`` per aggregator (GPU), one ``decide_batch`` and one GPU fold
    per aggregator, instead of a Python loop over reports;
  * a report that fails verification at some level (the reference would raise
    at ``prep_shares_to_prep``) is dropped from that level's aggregate and
    from every later level, which is what a deployed aggregator does.  With
    only honest reports the output is identical to the reference's.
  * multi-GPU: every rank sweeps its own shard of
    the reports and passes ``merge`` (e.g. :func:`mastic_amd.merge.merge_field_shares`:
    RCCL all-gather + GPU mod-p fold), so each level's pruning decision is
    taken on the job-wide aggregate and all ranks walk the same frontier.
"""
import contextlib

import numpy as np

# joint_rand_confirmed and _encode_reports lived here once and stay importable from here
from .rounds import (PhaseClock, Round, admit, encode_reports as _encode_reports,  # noqa: F401
                     joint_rand_confirmed, on_device, resident, unshard_raw as _unshard_raw)
from .vdaf import Mastic


def get_threshold(thresholds, prefix):
    """poc/examples.py:26-34: the threshold of the longest proper prefix of
    ``prefix`` listed in ``thresholds`` (the prefix itself excluded), else
    ``thresholds['default']``."""
    if len(thresholds) == 1:  # only 'default' (common case: skips the O(len) walk)
        return thresholds['default']
    for level in reversed(range(len(prefix) - 1)):
        if prefix[:level + 1] in thresholds:
            return thresholds[prefix[:level + 1]]
    return thresholds['default']


def _child_packed(packed: bytes, level: int, bit: bool) -> bytes:
    """MSB-first packing (vidpf.py:33-39) of ``prefix + (bit,)`` from the
    packing of the length-``level`` ``prefix``."""
    if level % 8 == 0:
        packed += b"\x00"
    if bit:
        packed = packed[:-1] + bytes([packed[-1] | (0x80 >> (level % 8))])
    return packed


def _unpack_prefix(packed: bytes, length: int):
    """The tuple of bools of an MSB-first packed prefix (vidpf.py:33-39)."""
    return tuple(bool((packed[i // 8] >> (7 - i % 8)) & 1) for i in range(length))


class SweepLevel:
    """What one level of the sweep did (for callers that want the trace)."""

    def __init__(self, level, prefixes, agg_result, n_valid):
        self.level = level
        self.prefixes = prefixes
        self.agg_result = agg_result
        self.n_valid = n_valid


class Frontier:
    """The sweep's candidate prefixes, level by level: both one-bit prefixes
    at level 0, then the two children of every candidate whose aggregate
    reached its threshold (:func:`get_threshold`).

    The candidates are kept in the forms the sweep needs, decided here, once.
    The device form (``device``) takes the encoded aggregation parameter from
    the candidates' MSB-first packings (``packed``), each extended from its
    parent's instead of re-packed bit by bit; the wire form encodes the bool
    tuples (``prefixes``).  The tuples are left out altogether (``lazy``, and
    then ``prefixes`` is None) when nothing asks for them: the device form, no
    ``trace``, one default threshold, and no ``merge`` that is told the
    level's candidates (``begin_level``) or folds field-object shares (one
    without ``total``)."""

    def __init__(self, bits: int, thresholds, device: bool, trace=None, merge=None):
        self.bits = bits
        self.thresholds = thresholds
        self.lazy = (device and trace is None and len(thresholds) == 1
                     and (merge is None or (hasattr(merge, "total") and not hasattr(merge, "begin_level"))))
        self.packed = [b"\x00", b"\x80"] if device else None
        self.prefixes = None if self.lazy else [(False,), (True,)]
        self.heavy_hitters = []

    @property
    def n_cand(self):
        return len(self.prefixes if self.packed is None else self.packed)

    def agg_param(self, level: int):
        """The level's aggregation parameter for ``is_valid``, ``agg_init`` and
        ``unshard`` (lazy: without the prefixes)."""
        return (level, () if self.lazy else tuple(self.prefixes), level == 0)

    def encode(self, mastic, agg_param) -> bytes:
        """``agg_param`` encoded, once per level (the batch calls take the bytes)."""
        if self.packed is None:
            return mastic.encode_agg_param(agg_param)
        (level, _prefixes, weight_check) = agg_param
        return (level.to_bytes(2, "big") + len(self.packed).to_bytes(4, "big") + b"".join(self.packed)
                + bytes([int(weight_check)]))

    def prune(self, level: int, agg_result):
        """Keep the candidates whose aggregate reaches their threshold: their
        children are the next level's candidates, and at the last level they
        are the heavy hitters."""
        if self.lazy:
            th = self.thresholds['default']
            keep = [i for (i, count) in enumerate(agg_result) if count >= th]
        else:
            keep = [i for (i, (prefix, count)) in enumerate(zip(self.prefixes, agg_result))
                    if count >= get_threshold(self.thresholds, prefix)]
        if level == self.bits - 1:
            self.heavy_hitters = [_unpack_prefix(self.packed[i], self.bits) if self.lazy else self.prefixes[i]
                                  for i in keep]
            return
        if not self.lazy:
            self.prefixes = [self.prefixes[i] + (bit,) for i in keep for bit in (False, True)]
        if self.packed is not None:
            self.packed = [_child_packed(self.packed[i], level + 1, bit) for i in keep for bit in (False, True)]


def _folds(mastic, merge, device: bool, lazy: bool):
    """``(fold, fold_empty)``: how a level's aggregate is made after a round
    and without one (no reports, or no candidates).  Each is a pair
    ``(shares, unshard)``: ``shares(enc, mask, agg_param, n_cand)`` gives the
    level's agg shares (``mask``: the round's accept mask, None without a
    round, and then agg_init's zeros for every candidate), and
    ``unshard(agg_param, shares, num_measurements)`` the aggregate."""
    n_elems = 1 + mastic.OUTPUT_LEN  # per candidate

    def merged(enc, mask, agg_param, n_cand):
        # both shares folded, gathered and merged in HBM (one RCCL call); a rank
        # without a round still calls, so that every rank issues the same collectives
        if mask is None:
            return [merge.total(n_cand * n_elems, have_results=False)]
        return [merge.total(n_cand * n_elems, mask)]

    def raw(enc, mask, agg_param, n_cand):
        if mask is None:
            return [bytes(n_cand * n_elems * mastic.field.ENCODED_SIZE)]
        return [mastic.aggregate_device(agg_id, enc, mask, raw=True) for agg_id in range(2)]

    def fields(enc, mask, agg_param, n_cand):
        if mask is None:
            return [mastic.agg_init(agg_param) for _ in range(2)]
        return [mastic.aggregate_device(agg_id, enc, mask) for agg_id in range(2)]

    def unshard_raw(agg_param, shares, num_measurements):
        return _unshard_raw(mastic, shares, num_measurements)

    def unshard_fields(agg_param, shares, num_measurements):
        if merge is not None:
            shares = [merge(a) for a in shares]
        return mastic.unshard(agg_param, shares, num_measurements)

    if device and merge is not None and hasattr(merge, "total"):
        return ((merged, unshard_raw), (merged, unshard_raw))
    # without a round the lazy agg param carries no prefix tuples for agg_init to count
    return ((raw, unshard_raw) if device and merge is None else (fields, unshard_fields),
            (raw, unshard_raw) if lazy else (fields, unshard_fields))


@contextlib.contextmanager
def _cache_nodes(mastic, mode):
    """The frontier cache's node format set to ``mode`` and left as found
    afterwards; None leaves the mastic's mode alone."""
    found = None if mode is None else mastic.set_frontier_cache_nodes(mode)
    try:
        yield
    finally:
        if found is not None:
            mastic.set_frontier_cache_nodes(found)


def compute_heavy_hitters(mastic: Mastic, ctx: bytes, thresholds, reports, verify_key: bytes = None,
                          trace=None, merge=None, timing=None, frontier_cache=None, cached_levels=None,
                          phase_times=None, level_hook=None, cache_nodes=None, nonce_set=None, compact=None):
    """poc/examples.py:37-91 on the GPU.

    ``reports`` is either the reference's list of
    ``(nonce, public_share, input_shares)`` tuples or a device-resident
    :class:`~mastic_amd.vdaf.Reports` batch holding both input shares
    (``Mastic.reports_shard`` / ``reports_upload``).  ``verify_key`` defaults
    to 16 fresh random bytes, as in the reference (examples.py:38).  If ``trace`` is a list, one
    :class:`SweepLevel` per level is appended to it.  ``merge`` maps this
    rank's agg share (list of field elements) to the job-wide one (all
    ranks call it at every level, in the same order).  If ``timing`` is a
    list, ``mastic.last_timing3()`` of every prep_init is appended to it.
    ``frontier_cache`` (True/False) switches the GPU frontier cache
    (``Mastic.set_frontier_cache``): each level then evaluates only its new
    tree level when the previous level's tree is unchanged; if
    ``cached_levels`` is a list, the levels that took that path are appended.
    If ``phase_times`` is a dict, the host wall time of each phase of a level
    (enqueueing both prep_inits, decide, aggregate + merge, unshard + prune) is
    accumulated into it (seconds).  ``level_hook(level, enc_agg_param, reports)``
    (if given) runs after each level's decide, while both aggregators' prep_init
    results of the level are still in HBM (e.g. to read sampled prep shares).

    ``nonce_set`` (a :class:`~mastic_amd.nonce_set.NonceSet`, or any object
    with ``admit(reports) -> mask``) is the aggregator's replay protection:
    the sweep begins by admitting the batch, and a report whose nonce the set
    already held, or that occurs earlier in the batch, is dropped from every
    level exactly like a report that fails verification, so the counts and
    ``num_measurements`` cover fresh reports only.  Afterwards the set holds
    the batch's nonces, so sweeping the same reports again with the same set
    keeps none of them.  Multi-rank: each rank's set sees only its own shard,
    so a job gets job-wide protection only if it routes every report to a rank
    by its nonce (copies of a report then meet in one set); the routing is the
    job's business.

    ``compact`` (None, or a float t in [0, 1]) drops dead reports from the
    resident batch itself (``Reports.compact``), so that later levels do not
    evaluate them: None, the default, never does.  With t, the batch is
    compacted when the dead share of the current batch is at least t, at
    exactly two points: after the replay admit, before level 0, and after
    level 0's fold.  That is where almost all rejections happen (replays, the
    weight check, malformed shares), and the frontier-cache miss a compaction
    forces re-evaluates a tree of 2 nodes there; later rejections stay masked,
    because compacting then would turn a cache hit into a whole-tree miss.
    Every level's aggregate, ``n_valid`` and ``num_measurements`` are the same
    either way.  If ``reports`` is the caller's own :class:`Reports` batch,
    compaction mutates it: afterwards it holds the surviving reports only, in
    their order, and ``reports.n`` is their number.

    ``cache_nodes`` (``'seeds'``, ``'payloads'`` or ``'auto'``:
    ``Mastic.set_frontier_cache_nodes``) is the frontier cache's node format
    for the sweep; the mastic's mode is left as found afterwards, and None
    leaves it alone.
    """
    if compact is not None and not 0.0 <= compact <= 1.0:
        raise ValueError("compact must be None or a share in [0, 1]")
    with _cache_nodes(mastic, cache_nodes):
        if frontier_cache is not None:
            mastic.set_frontier_cache(frontier_cache)
        if verify_key is None:
            import os
            verify_key = os.urandom(16)  # gen_rand(16), examples.py:38
        (dev, n) = resident(mastic, reports)
        alive = admit(nonce_set, dev, n)

        def drop_dead():
            # the dead rows leave the batch; the survivors keep their order
            nonlocal n, alive
            dead = n - int(alive.sum())
            if compact is not None and dead and dead >= compact * n:
                n = dev.compact(alive)
                alive = np.ones(n, dtype=bool)

        drop_dead()

        device = on_device(mastic)
        clock = PhaseClock(phase_times)
        frontier = Frontier(mastic.vidpf.BITS, thresholds, device, trace, merge)
        verify = Round(mastic, ctx, verify_key, timing, clock, cached_levels if frontier_cache else None)
        (fold, fold_empty) = _folds(mastic, merge, device, frontier.lazy)
        begin_level = getattr(merge, "begin_level", None)  # merges that need the level's candidates
        prev_agg_params = []
        for level in range(frontier.bits):
            agg_param = frontier.agg_param(level)
            assert mastic.is_valid(agg_param, prev_agg_params)
            enc = frontier.encode(mastic, agg_param)
            n_cand = frontier.n_cand
            if begin_level is not None:
                begin_level(level, frontier.prefixes)
            clock.start()
            ((shares, unshard), mask) = (fold_empty, None)
            if n and n_cand:
                verify(dev, enc, alive, level == 0, level)
                if level_hook is not None:
                    level_hook(level, enc, dev)
                ((shares, unshard), mask) = (fold, alive.astype(np.uint8))
            agg_shares = shares(enc, mask, agg_param, n_cand)
            clock.mark("aggregate_merge")
            agg_result = unshard(agg_param, agg_shares, int(alive.sum()))
            prev_agg_params.append(agg_param)
            if trace is not None:
                trace.append(SweepLevel(level, list(frontier.prefixes), agg_result, int(alive.sum())))
            if level == 0:
                drop_dead()
            frontier.prune(level, agg_result)
            if level < frontier.bits - 1:
                clock.mark("unshard_prune")
        return frontier.heavy_hitters
