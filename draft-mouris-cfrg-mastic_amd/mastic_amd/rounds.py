"""The steps every batched driver shares (the heavy-hitters sweep,
:mod:`~mastic_amd.heavy_hitters`, and the attribute metrics,
:mod:`~mastic_amd.metrics`): the resident batch, the replay admit, one
verification round of the batch for an aggregation parameter, and the
collector's ``unshard`` on encoded agg shares.

A round exists in two forms.  The *device form*, taken for a real
:class:`~mastic_amd.vdaf.Mastic`, decides on the GPU: the prep shares stay in
HBM and only the accept mask comes back.  The *wire form*, taken for anything
else (the plaintext stand-ins of the CPU tests), fetches both aggregators'
wire results and decides from them, as two aggregators on two machines would.
"""
import time

import numpy as np

from .vdaf import Mastic


def on_device(mastic) -> bool:
    """Whether drivers take the device form with ``mastic``."""
    return isinstance(mastic, Mastic)


def encode_reports(mastic, reports):
    nonces = b"".join(r[0] for r in reports)
    pubs = b"".join(mastic.encode_public_share(r[1]) for r in reports)
    in0 = b"".join(mastic.test_vec_encode_input_share(r[2][0]) for r in reports)
    in1 = b"".join(mastic.test_vec_encode_input_share(r[2][1]) for r in reports)
    return (nonces, pubs, in0, in1)


def resident(mastic, reports):
    """``(batch, n)`` for a driver's ``reports``: the reference's list of
    ``(nonce, public_share, input_shares)`` tuples is uploaded once, a
    :class:`~mastic_amd.vdaf.Reports` batch is used as it is, and an empty
    list gives ``(None, 0)``."""
    if isinstance(reports, (list, tuple)):
        reports = mastic.reports_upload(*encode_reports(mastic, reports)) if len(reports) else None
    return (reports, 0 if reports is None else reports.n)


def admit(nonce_set, dev, n):
    """The ``alive`` mask (bool, one per report) the batch starts with: all of
    it, or what ``nonce_set`` (replay protection) admits."""
    if nonce_set is not None and n:
        return np.asarray(nonce_set.admit(dev)) == 1
    return np.ones(n, dtype=bool)


def unshard_raw(mastic, raw_shares, num_measurements):
    """``mastic.unshard`` (mastic.py:399-411) on encode_vec agg shares (the
    two aggregators', or one already-merged total), summed as integers mod p
    (same result, without a field object per share element; Field64 in
    numpy: 2^64 = 2^32 - 1 mod p)."""
    f = mastic.field
    enc = f.ENCODED_SIZE
    p = f.MODULUS
    k = 1 + mastic.OUTPUT_LEN
    if enc == 8:
        acc = None
        for r in raw_shares:
            v = np.frombuffer(r, dtype="<u8")
            if v.size and int(v.max()) >= p:
                raise ValueError("encoded element out of range")
            if acc is None:
                acc = v.copy()
                continue
            t = acc + v  # wraps mod 2^64
            t += (t < acc).astype(np.uint64) * np.uint64(0xFFFFFFFF)
            acc = np.where(t >= np.uint64(p), t - np.uint64(p), t)
        ints = [] if acc is None else acc.tolist()
    else:
        vecs = [[int.from_bytes(r[i:i + enc], "little") for i in range(0, len(r), enc)] for r in raw_shares]
        for v in vecs:
            if v and max(v) >= p:
                raise ValueError("encoded element out of range")
        ints = [sum(col) % p for col in zip(*vecs)]
    if mastic.circuit in ("Count", "Sum"):  # Mastic.decode_result: the one output element
        return ints[1::k]
    return [ints[i + 1:i + k] for i in range(0, len(ints), k)]


def joint_rand_confirmed(msgs: bytes, jr_seeds_0: bytes, jr_seeds_1: bytes, n: int):
    """Per report: ``prep_next``'s joint-rand confirmation (mastic.py:369-375)
    for both aggregators -- the prep message (the seed recomputed from both
    parts, ``prep_shares_to_prep``) equals each aggregator's own seed."""
    if n == 0:
        return np.ones(0, dtype=bool)
    m = np.frombuffer(msgs, np.uint8, count=32 * n).reshape(n, 32)
    j0 = np.frombuffer(jr_seeds_0, np.uint8, count=32 * n).reshape(n, 32)
    j1 = np.frombuffer(jr_seeds_1, np.uint8, count=32 * n).reshape(n, 32)
    return (m == j0).all(axis=1) & (m == j1).all(axis=1)


class PhaseClock:
    """Host wall time per phase, accumulated into the dict ``times`` (seconds);
    with None nothing is measured."""

    def __init__(self, times=None):
        self.times = times
        self.t = 0.0

    def start(self):
        if self.times is not None:
            self.t = time.perf_counter()

    def mark(self, phase):
        """The time since ``start`` or the last mark goes to ``phase``."""
        if self.times is not None:
            t1 = time.perf_counter()
            self.times[phase] = self.times.get(phase, 0.0) + t1 - self.t
            self.t = t1


class Round:
    """One verification round of a resident batch: ``round(dev, enc, alive,
    weight_check)`` enqueues both aggregators' ``prep_init_device`` for the
    encoded aggregation parameter ``enc``, decides every report, and clears
    the rejected ones in ``alive`` (in place).  Both aggregators' results of
    the round are still in HBM afterwards, for the fold.

    ``timing`` (a list) collects ``last_timing3()`` of every prep_init,
    ``clock`` the host time of the enqueue (``prep_init_enqueue``) and, in the
    device form, of the decide (``decide_wait``; reading the timings is not
    clocked).  ``cached_levels`` (a list) collects the ``level`` of every round
    whose prep_init took the frontier cache's hit path."""

    def __init__(self, mastic, ctx: bytes, verify_key: bytes, timing=None, clock=None, cached_levels=None):
        (self.mastic, self.ctx, self.verify_key) = (mastic, ctx, verify_key)
        (self.timing, self.cached_levels) = (timing, cached_levels)
        self.clock = PhaseClock() if clock is None else clock
        self.decide = self._decide_on_device if on_device(mastic) else self._decide_on_wire

    def __call__(self, dev, enc: bytes, alive, weight_check: bool, level=None):
        # both aggregators' prep_init are queued before either result is
        # fetched, so the host work of the second overlaps the GPU run of
        # the first (stream-ordered; results and timings are per agg_id)
        for agg_id in range(2):
            self.mastic.prep_init_device(dev, self.verify_key, self.ctx, agg_id, enc)
            if self.cached_levels is not None and agg_id == 0 and self.mastic.last_prep_was_cached():
                self.cached_levels.append(level)
        self.clock.mark("prep_init_enqueue")
        self.decide(dev, enc, alive, weight_check)

    def _decide_on_device(self, dev, enc, alive, weight_check):
        # both aggregators' prep_shares_to_prep + prep_next on the GPU:
        # the prep shares stay in HBM, only the accept mask comes back
        m = self.mastic
        (accept, _codes) = m.decide_results(self.ctx, alive.size)
        alive &= accept == 1
        self.clock.mark("decide_wait")
        if self.timing is not None:
            for agg_id in range(2):
                m.select_timing(agg_id)
                self.timing.append(m.last_timing3())
        self.clock.start()

    def _decide_on_wire(self, dev, enc, alive, weight_check):
        m = self.mastic
        shares = []
        for agg_id in range(2):
            shares.append(m.prep_result(dev, agg_id, enc))
            if self.timing is not None:
                self.timing.append(m.last_timing3())
        (msgs, valid) = m.decide_batch(self.ctx, enc, shares[0][0], shares[1][0])
        alive &= (valid == 1) & (shares[0][3] == 0) & (shares[1][3] == 0)
        if weight_check and m.JOINT_RAND_LEN > 0:
            # prep_next (mastic.py:364-377, called at examples.py:67): each
            # aggregator's joint-rand seed must equal the prep message
            alive &= joint_rand_confirmed(msgs, shares[0][1], shares[1][1], alive.size)
