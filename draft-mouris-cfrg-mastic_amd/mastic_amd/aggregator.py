"""One aggregator of two: the messages that cross between the aggregators in
a verification round, and one aggregator's state machine.

:mod:`~mastic_amd.rounds` and :func:`~mastic_amd.heavy_hitters.compute_heavy_hitters`
drive both aggregators on one GPU, over a batch that holds both input shares.
A deployed aggregator holds one input share per report and its peer is another
party: :class:`Aggregator` runs ``prep_init`` for its own ``agg_id`` only,
offers its prep shares to the peer, decides against the peer's offer where its
own result lies in HBM (``Mastic.decide_peer``) and folds what both accepted.

The module is sans-IO: it produces and consumes ``bytes``, and whoever deploys
it owns the transport.  A round is four messages, two each way::

    offer   = b"MOF1" | agg_id u8 | weight_check u8 | n u32 | psz u32 | sha256(enc_agg_param) [32]
              | ok [ceil(n/8)] | rows [n*psz]
    verdict = b"MVD1" | agg_id u8 | n u32 | accept [ceil(n/8)]

Integers are little-endian.  In a bitmap report i is bit ``i % 8`` of byte
``i // 8`` and the padding bits are zero.  ``ok[i]`` says that the sender still
holds report i as alive and its ``prep_init`` status is 0; ``rows`` are the
sender's prep shares in wire encoding (mastic.py:543-552), ``psz`` bytes each,
zero-filled where ``ok[i]`` is 0 (a result with a nonzero status has unspecified
bytes, which never cross the wire).  ``accept[i]`` is the sender's
``prep_shares_to_prep`` + ``prep_next`` outcome.  The verdicts are always
exchanged: a report stays alive only if both aggregators accepted it, so both
fold the same set even when only one side's ``prep_next`` fails.

:func:`run_round` and :func:`sweep_lockstep` pass the messages between two
aggregators in one process, for tests and as the worked example.

Out of scope: a multi-rank aggregator (a ``CommMerge`` under an
:class:`Aggregator`), a one-aggregator ``compute_attribute_metrics``, and any
transport.
"""
import hashlib
import struct
from collections import namedtuple

import numpy as np

from .heavy_hitters import Frontier, SweepLevel
from .rounds import admit, on_device, unshard_raw

OFFER_MAGIC = b"MOF1"
VERDICT_MAGIC = b"MVD1"
_OFFER_HEAD = struct.Struct("<4sBBII32s")
_VERDICT_HEAD = struct.Struct("<4sBI")

Offer = namedtuple("Offer", "agg_id weight_check n psz digest ok rows")
Verdict = namedtuple("Verdict", "agg_id n accept")


def _pack_mask(mask) -> bytes:
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little").tobytes()


def _unpack_mask(data: bytes, n: int):
    bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")
    if bits[n:].any():
        raise ValueError("nonzero padding bits in a bitmap")
    return bits[:n].astype(bool)


def _expect(what: str, got, want):
    if want is not None and got != want:
        raise ValueError("%s is %r, this round has %r" % (what, got, want))


def _sender(agg_id: int, own_agg_id):
    if agg_id not in (0, 1):
        raise ValueError("invalid aggregator ID %d" % agg_id)
    if own_agg_id is not None and agg_id == own_agg_id:
        raise ValueError("a message of aggregator %d reached aggregator %d" % (agg_id, own_agg_id))


def encode_offer(agg_id: int, weight_check: bool, enc_agg_param: bytes, ok, rows, psz: int) -> bytes:
    """The offer of aggregator ``agg_id`` for one round: ``ok`` is the mask of
    the reports it offers, ``rows`` its ``len(ok) * psz`` bytes of prep shares.
    The rows of reports that are not ok are zero-filled here."""
    _sender(agg_id, None)
    ok = np.asarray(ok, dtype=bool)
    n = ok.size
    rows = np.frombuffer(rows, np.uint8)
    if not 0 < psz < 2 ** 32 or n >= 2 ** 32 or rows.size != n * psz:
        raise ValueError("prep shares have incorrect length")
    if n and not ok.all():
        rows = rows.reshape(n, psz) * ok[:, None].astype(np.uint8)
    head = _OFFER_HEAD.pack(OFFER_MAGIC, agg_id, int(bool(weight_check)), n, psz,
                            hashlib.sha256(enc_agg_param).digest())
    return head + _pack_mask(ok) + rows.tobytes()


def decode_offer(data: bytes, own_agg_id=None, n=None, psz=None, weight_check=None, enc_agg_param=None) -> Offer:
    """Parse an offer.  Every expectation that is given (the receiver's own
    ``agg_id`` and its round's ``n``, ``psz``, ``weight_check`` and encoded
    aggregation parameter) is checked; ValueError for a mismatch and for a
    malformed message."""
    data = bytes(data)
    if len(data) < _OFFER_HEAD.size:
        raise ValueError("truncated offer")
    (magic, agg_id, wc, n_got, psz_got, digest) = _OFFER_HEAD.unpack_from(data)
    if magic != OFFER_MAGIC:
        raise ValueError("not an offer (wrong magic)")
    _sender(agg_id, own_agg_id)
    if wc not in (0, 1):
        raise ValueError("weight_check is neither 0 nor 1")
    _expect("weight_check", bool(wc), None if weight_check is None else bool(weight_check))
    _expect("n", n_got, n)
    _expect("psz", psz_got, psz)
    if psz_got == 0:
        raise ValueError("psz is 0")
    if enc_agg_param is not None and digest != hashlib.sha256(enc_agg_param).digest():
        raise ValueError("the offer is for another aggregation parameter")
    nb = (n_got + 7) // 8
    want = _OFFER_HEAD.size + nb + n_got * psz_got
    if len(data) < want:
        raise ValueError("truncated offer")
    if len(data) > want:
        raise ValueError("trailing bytes after the offer")
    ok = _unpack_mask(data[_OFFER_HEAD.size:_OFFER_HEAD.size + nb], n_got)
    return Offer(agg_id, bool(wc), n_got, psz_got, digest, ok, data[_OFFER_HEAD.size + nb:])


def encode_verdict(agg_id: int, accept) -> bytes:
    _sender(agg_id, None)
    accept = np.asarray(accept, dtype=bool)
    if accept.size >= 2 ** 32:
        raise ValueError("too many reports")
    return _VERDICT_HEAD.pack(VERDICT_MAGIC, agg_id, accept.size) + _pack_mask(accept)


def decode_verdict(data: bytes, own_agg_id=None, n=None) -> Verdict:
    """Parse a verdict, checked against the receiver's own ``agg_id`` and its
    round's ``n`` where given; ValueError as for :func:`decode_offer`."""
    data = bytes(data)
    if len(data) < _VERDICT_HEAD.size:
        raise ValueError("truncated verdict")
    (magic, agg_id, n_got) = _VERDICT_HEAD.unpack_from(data)
    if magic != VERDICT_MAGIC:
        raise ValueError("not a verdict (wrong magic)")
    _sender(agg_id, own_agg_id)
    _expect("n", n_got, n)
    want = _VERDICT_HEAD.size + (n_got + 7) // 8
    if len(data) < want:
        raise ValueError("truncated verdict")
    if len(data) > want:
        raise ValueError("trailing bytes after the verdict")
    return Verdict(agg_id, n_got, _unpack_mask(data[_VERDICT_HEAD.size:], n_got))


class Aggregator:
    """Aggregator ``agg_id`` of two over one batch of reports.

    ``reports`` is a :class:`~mastic_amd.vdaf.Reports` batch that holds this
    aggregator's input share (the other may be missing), or a list of
    ``(nonce, public_share, input_share)`` tuples with this aggregator's input
    share, which is uploaded once.  ``nonce_set`` is this aggregator's replay
    protection: the batch is admitted at construction, and what the set
    rejects is never offered.  ``frontier_cache`` (True / False) switches the
    GPU frontier cache.

    One round is ``offer(enc_agg_param)``, ``decide(peer_offer)``,
    ``settle(peer_verdict)``, in this order (RuntimeError otherwise); the bytes
    each returns go to the peer.  After ``settle`` the round's result is still
    in HBM: ``agg_share`` and ``aggregate_grouped`` fold it over the reports
    both aggregators accepted.

    ``compact`` (None, or a share t in [0, 1]) drops dead reports from the
    batch itself (``Reports.compact``) as ``compute_heavy_hitters`` does: after
    the admit, and after the first round (the one with the weight check),
    which here means when the next ``offer`` begins, so that the first round's
    folds still see its numbering; each time only if the dead share is at
    least t.  After the first round both aggregators hold the same ``alive``
    and compact identically; after the admit they do if their nonce sets
    reject the same reports, which they do when both parties admitted the same
    batches.  Compaction mutates a caller's ``Reports`` batch."""

    def __init__(self, mastic, agg_id: int, ctx: bytes, verify_key: bytes, reports, nonce_set=None,
                 frontier_cache=None, compact=None):
        if agg_id not in (0, 1):
            raise ValueError("invalid aggregator ID")
        if compact is not None and not 0.0 <= compact <= 1.0:
            raise ValueError("compact must be None or a share in [0, 1]")
        (self.mastic, self.agg_id, self.ctx, self.verify_key) = (mastic, agg_id, ctx, verify_key)
        self.compact = compact
        if frontier_cache is not None:
            mastic.set_frontier_cache(frontier_cache)
        if isinstance(reports, (list, tuple)):
            reports = self._upload(reports) if len(reports) else None
        self.reports = reports
        self.n = 0 if reports is None else reports.n
        self.alive = admit(nonce_set, reports, self.n)
        self._drop_dead()
        self.prev_agg_params = []  # (level, (), weight_check) of the rounds so far, for is_valid
        self.last_was_cached = False
        self._state = "idle"
        self._settled = False  # a settled round's result is in HBM
        self._compact_due = False
        (self._enc, self._weight_check, self._n_cand) = (None, False, 0)
        (self._own_ok, self._peer_ok, self._own_accept) = (None, None, None)
        self._mask = None  # the settled round's accept mask, in that round's numbering

    def _upload(self, reports):
        m = self.mastic
        nonces = b"".join(r[0] for r in reports)
        pubs = b"".join(m.encode_public_share(r[1]) for r in reports)
        ins = b"".join(m.test_vec_encode_input_share(r[2]) for r in reports)
        return m.reports_upload(nonces, pubs, ins if self.agg_id == 0 else None, ins if self.agg_id == 1 else None)

    def _drop_dead(self):
        dead = self.n - int(self.alive.sum())
        if self.compact is not None and dead and dead >= self.compact * self.n:
            self.n = self.reports.compact(self.alive)
            self.alive = np.ones(self.n, dtype=bool)

    def _enter(self, state: str, call: str):
        if self._state != state:
            raise RuntimeError("%s() called out of order: a round is offer, decide, settle" % call)

    @property
    def n_valid(self) -> int:
        """Reports still alive (after the last settled round)."""
        return int(self.alive.sum())

    def offer(self, enc_agg_param: bytes) -> bytes:
        """Begin a round: ``prep_init`` for the own ``agg_id`` and the offer for the peer."""
        self._enter("idle", "offer")
        m = self.mastic
        enc = bytes(enc_agg_param)
        (level, prefixes, weight_check) = m.decode_agg_param(enc)
        agg_param = (level, (), bool(weight_check))  # is_valid reads the level and the weight check only
        if not m.is_valid(agg_param, self.prev_agg_params):
            raise ValueError("the aggregation parameter is not valid after the earlier rounds")
        if self._compact_due:
            self._compact_due = False
            self._drop_dead()
        self._settled = False
        (self._enc, self._weight_check, self._n_cand) = (enc, bool(weight_check), len(prefixes))
        psz = m.prep_share_size(self._weight_check)
        if self.n:
            m.prep_init_device(self.reports, self.verify_key, self.ctx, self.agg_id, enc)
            self.last_was_cached = bool(m.last_prep_was_cached())
            # the joint-rand seeds stay in HBM: decide_peer confirms against them there
            (rows, _jr_seeds, _out, status) = m.prep_result(self.reports, self.agg_id, enc, want_jr_seeds=False)
            self._own_ok = self.alive & (np.asarray(status) == 0)
        else:
            (rows, self._own_ok, self.last_was_cached) = (b"", np.zeros(0, dtype=bool), False)
        self.prev_agg_params.append(agg_param)
        self._state = "offered"
        return encode_offer(self.agg_id, self._weight_check, enc, self._own_ok, rows, psz)

    def decide(self, peer_offer: bytes) -> bytes:
        """Decide against the peer's offer (``Mastic.decide_peer``); returns the own verdict."""
        self._enter("offered", "decide")
        m = self.mastic
        peer = decode_offer(peer_offer, self.agg_id, self.n, m.prep_share_size(self._weight_check),
                            self._weight_check, self._enc)
        both = self._own_ok & peer.ok
        if self.n:
            (accept, _codes, _msgs) = m.decide_peer(self.agg_id, self.ctx, peer.rows, both)
            self._own_accept = (np.asarray(accept) == 1) & both
        else:
            self._own_accept = both
        self._peer_ok = peer.ok
        self._state = "decided"
        return encode_verdict(self.agg_id, self._own_accept)

    def settle(self, peer_verdict: bytes):
        """End the round: a report stays alive iff both aggregators offered
        and accepted it.  Returns ``alive`` (bool, one per report)."""
        self._enter("decided", "settle")
        peer = decode_verdict(peer_verdict, self.agg_id, self.n)
        self.alive &= self._own_accept & peer.accept & self._own_ok & self._peer_ok
        self._mask = self.alive.astype(np.uint8)
        self._compact_due = len(self.prev_agg_params) == 1
        self._settled = True
        self._state = "idle"
        return self.alive

    def _need_settled(self, call: str):
        if not self._settled:
            raise RuntimeError("%s() needs a settled round" % call)

    def agg_share(self, raw=True):
        """This aggregator's agg share of the settled round over the reports
        still alive: encode_vec bytes (``raw``) or field elements."""
        self._need_settled("agg_share")
        m = self.mastic
        if self.n == 0:
            zeros = bytes(self._n_cand * (1 + m.OUTPUT_LEN) * m.field.ENCODED_SIZE)
            return zeros if raw else m.field.decode_vec(zeros)
        return m.aggregate_device(self.agg_id, self._enc, self._mask, raw=raw)

    def aggregate_grouped(self, groups, n_groups: int, raw=False):
        """``Mastic.aggregate_grouped`` of the settled round under its accept mask."""
        self._need_settled("aggregate_grouped")
        if self.n == 0:  # no round ran on the GPU: agg_init's zeros per bucket, nothing folded
            zeros = bytes(self._n_cand * (1 + self.mastic.OUTPUT_LEN) * self.mastic.field.ENCODED_SIZE)
            share = zeros if raw else self.mastic.field.decode_vec(zeros)
            return ([share for _ in range(int(n_groups))], np.zeros(int(n_groups), np.uint64))
        return self.mastic.aggregate_grouped(self.agg_id, self._enc, groups, n_groups, valid=self._mask, raw=raw)


def run_round(agg0: Aggregator, agg1: Aggregator, enc_agg_param: bytes):
    """One round of two aggregators in one process: the two offers and the two
    verdicts cross as bytes.  Returns the mask both settled on."""
    (offer0, offer1) = (agg0.offer(enc_agg_param), agg1.offer(enc_agg_param))
    (verdict0, verdict1) = (agg0.decide(offer1), agg1.decide(offer0))
    (alive0, alive1) = (agg0.settle(verdict1), agg1.settle(verdict0))
    if not np.array_equal(alive0, alive1):
        raise RuntimeError("the aggregators settled on different reports")
    return alive0


def sweep_lockstep(agg0: Aggregator, agg1: Aggregator, thresholds, trace=None):
    """The weighted heavy-hitters sweep of ``compute_heavy_hitters`` with the
    collector's part played here and each aggregator's by its own
    :class:`Aggregator`: per level one :func:`run_round`, the two raw agg
    shares unsharded, the frontier pruned.  Returns the heavy hitters; if
    ``trace`` is a list, one :class:`~mastic_amd.heavy_hitters.SweepLevel` per
    level is appended."""
    mastic = agg0.mastic
    frontier = Frontier(mastic.vidpf.BITS, thresholds, on_device(mastic), trace)
    n_elems = 1 + mastic.OUTPUT_LEN
    for level in range(frontier.bits):
        agg_param = frontier.agg_param(level)
        enc = frontier.encode(mastic, agg_param)
        n_cand = frontier.n_cand
        if agg0.n and n_cand:
            run_round(agg0, agg1, enc)
            shares = [agg0.agg_share(raw=True), agg1.agg_share(raw=True)]
        else:
            shares = [bytes(n_cand * n_elems * mastic.field.ENCODED_SIZE)]
        agg_result = unshard_raw(mastic, shares, agg0.n_valid)
        if trace is not None:
            trace.append(SweepLevel(level, list(frontier.prefixes), agg_result, agg0.n_valid))
        frontier.prune(level, agg_result)
    return frontier.heavy_hitters
