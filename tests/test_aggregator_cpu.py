"""mastic_amd/aggregator.py on the CPU: the offer / verdict codec, one
aggregator's state machine over a plaintext stand-in for ``Mastic`` (it
implements exactly the calls the class may use), and the C boundary of
``mastic_decide_peer``.  The GPU runs are tests/test_gpu_decide_peer.py and
tests/test_gpu_one_aggregator.py."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mastic_amd import _lib
from mastic_amd.aggregator import (Aggregator, decode_offer, decode_verdict, encode_offer, encode_verdict, run_round,
                                   sweep_lockstep)
from mastic_amd.field import Field64
from mastic_amd.vdaf import Mastic
from test_sweep import index, plain_heavy_hitters, plain_sums

ENC = Mastic.encode_agg_param(None, (0, ((False,), (True,)), True))
SIZES = [0, 1, 7, 8, 9, 65]


# ------------------------------------------------------------------ codec
def _offer(n, psz=40, agg_id=0, wc=True, seed=0):
    rng = np.random.default_rng(seed + n)
    ok = rng.integers(0, 2, n).astype(bool)
    rows = rng.integers(1, 256, n * psz, dtype=np.uint8).tobytes()
    return (ok, rows, encode_offer(agg_id, wc, ENC, ok, rows, psz))


@pytest.mark.parametrize("n", SIZES)
def test_offer_round_trips(n):
    (ok, rows, data) = _offer(n)
    assert len(data) == 4 + 1 + 1 + 4 + 4 + 32 + (n + 7) // 8 + n * 40
    assert data[:4] == b"MOF1" and data[4:6] == b"\x00\x01"
    assert data[6:10] == n.to_bytes(4, "little") and data[10:14] == (40).to_bytes(4, "little")
    assert data[14:46] == hashlib.sha256(ENC).digest()
    o = decode_offer(data, own_agg_id=1, n=n, psz=40, weight_check=True, enc_agg_param=ENC)
    assert (o.agg_id, o.weight_check, o.n, o.psz) == (0, True, n, 40)
    assert np.array_equal(o.ok, ok)
    got = np.frombuffer(o.rows, np.uint8).reshape(n, 40)
    want = np.frombuffer(rows, np.uint8).reshape(n, 40)
    assert np.array_equal(got[ok], want[ok]) and not got[~ok].any()
    for i in range(n):  # report i is bit i % 8 of byte i // 8
        assert bool(data[46 + i // 8] >> (i % 8) & 1) == bool(ok[i])


@pytest.mark.parametrize("n", SIZES)
def test_verdict_round_trips(n):
    acc = np.random.default_rng(n).integers(0, 2, n).astype(bool)
    data = encode_verdict(1, acc)
    assert data[:4] == b"MVD1" and data[4] == 1 and data[5:9] == n.to_bytes(4, "little")
    assert len(data) == 9 + (n + 7) // 8
    v = decode_verdict(data, own_agg_id=0, n=n)
    assert (v.agg_id, v.n) == (1, n) and np.array_equal(v.accept, acc)


def test_malformed_offers_raise():
    (_ok, _rows, data) = _offer(9)
    want = dict(own_agg_id=1, n=9, psz=40, weight_check=True, enc_agg_param=ENC)
    decode_offer(data, **want)
    bad = {
        "magic": b"MOF2" + data[4:],
        "verdict magic": b"MVD1" + data[4:],
        "own agg_id": data[:4] + b"\x01" + data[5:],
        "agg_id 2": data[:4] + b"\x02" + data[5:],
        "weight_check": data[:5] + b"\x00" + data[6:],
        "weight_check 2": data[:5] + b"\x02" + data[6:],
        "truncated head": data[:20],
        "truncated rows": data[:-1],
        "truncated bitmap": data[:47],
        "trailing": data + b"\x00",
        "padding": data[:47] + bytes([data[47] | 0x80]) + data[48:],
        "empty": b"",
    }
    for (what, msg) in bad.items():
        with pytest.raises(ValueError):
            decode_offer(msg, **want)
            pytest.fail("accepted an offer with: " + what)
    for other in (dict(n=8), dict(n=10), dict(psz=32), dict(weight_check=False),
                  dict(enc_agg_param=ENC[:-1] + b"\x00")):
        with pytest.raises(ValueError):
            decode_offer(data, **{**want, **other})
    # a header that claims more reports than the message holds
    with pytest.raises(ValueError):
        decode_offer(data[:6] + (10).to_bytes(4, "little") + data[10:], own_agg_id=1)
    with pytest.raises(ValueError):
        encode_offer(0, True, ENC, np.ones(3, bool), bytes(3 * 40 - 1), 40)
    with pytest.raises(ValueError):
        encode_offer(2, True, ENC, np.ones(1, bool), bytes(40), 40)


def test_malformed_verdicts_raise():
    data = encode_verdict(0, np.ones(9, bool))
    decode_verdict(data, own_agg_id=1, n=9)
    for msg in (b"MOF1" + data[4:], data[:4] + b"\x01" + data[5:], data[:4] + b"\x03" + data[5:], data[:-1],
                data[:6], data + b"\x00", data[:-1] + b"\x03", b""):
        with pytest.raises(ValueError):
            decode_verdict(msg, own_agg_id=1, n=9)
    for n in (8, 10):
        with pytest.raises(ValueError):
            decode_verdict(data, own_agg_id=1, n=n)


# ------------------------------------------------------------ the stand-in
class FakeReports:
    def __init__(self, meas, nonces=None):
        self.meas = list(meas)
        self.nonces = list(nonces) if nonces is not None else [i.to_bytes(16, "big") for i in range(len(meas))]
        self.n = len(self.meas)
        self.compactions = 0

    def compact(self, keep):
        keep = np.asarray(keep).astype(bool)
        assert keep.shape == (self.n,)
        self.meas = [m for (m, k) in zip(self.meas, keep) if k]
        self.nonces = [m for (m, k) in zip(self.nonces, keep) if k]
        self.n = len(self.meas)
        self.compactions += 1
        return self.n


class FakeMastic:
    """The calls an Aggregator may make, in plaintext.  A prep share is a hash
    of the report's nonce and the level, the same on both sides (plus 8 bytes
    with the weight check); ``tamper`` reports get another hash on this side,
    ``bad_status`` reports status -3 and garbage bytes, ``reject`` reports
    fail this side's own prep_next although the shares agree (each a set of
    indices into the batch as the first round sees it; they follow their
    reports through a later compaction).  Aggregator 0's
    agg share is the plaintext (count, weight) per prefix, aggregator 1's is
    zeros."""
    OUTPUT_LEN = 1
    JOINT_RAND_LEN = 0
    circuit = "Count"
    field = Field64
    encode_agg_param = Mastic.encode_agg_param
    decode_agg_param = Mastic.decode_agg_param
    _agg_param_header = staticmethod(Mastic._agg_param_header)
    is_valid = Mastic.is_valid

    def __init__(self, bits, tamper=(), bad_status=(), reject=(), reject_level=0):
        class V:
            BITS = bits
        self.vidpf = V()
        (self.tamper, self.bad_status, self.reject) = (set(tamper), set(bad_status), set(reject))
        self.reject_level = reject_level
        self.marked = None
        self.calls = []
        self.uploads = []

    def prep_share_size(self, weight_check):
        return 40 if weight_check else 32

    def set_frontier_cache(self, on):
        self.calls.append(("set_frontier_cache", on))

    def last_prep_was_cached(self):
        return False

    def encode_public_share(self, pub):
        return pub

    def test_vec_encode_input_share(self, share):
        return share

    def reports_upload(self, nonces, pubs, in0=None, in1=None):
        self.uploads.append((nonces, pubs, in0, in1))
        ins = in0 if in0 is not None else in1
        n = len(nonces) // 16
        meas = [(index(ins[2 * i], self.vidpf.BITS), ins[2 * i + 1]) for i in range(n)]
        return FakeReports(meas, [nonces[16 * i:16 * (i + 1)] for i in range(n)])

    def _rows(self, agg_id):
        (level, _prefixes, wc) = self._ap
        psz = self.prep_share_size(wc)
        out = bytearray()
        for (i, nonce) in enumerate(self._dev.nonces):
            salt = b"tampered" if i in self.tamper else b""
            out += hashlib.shake_128(nonce + bytes([level]) + salt).digest(psz)
        return bytes(out)

    def prep_init_device(self, dev, vk, ctx, agg_id, enc):
        self.calls.append(("prep_init", agg_id, enc))
        if self.marked is None:
            self.marked = [{dev.nonces[i] for i in s} for s in (self.tamper, self.bad_status, self.reject)]
        (self.tamper, self.bad_status, self.reject) = (
            {i for (i, nonce) in enumerate(dev.nonces) if nonce in s} for s in self.marked)
        (self._dev, self._ap, self._agg) = (dev, self.decode_agg_param(enc), agg_id)

    def prep_result(self, dev, agg_id, enc, want_jr_seeds=True):
        assert agg_id == self._agg and dev is self._dev
        psz = self.prep_share_size(self._ap[2])
        rows = bytearray(self._rows(agg_id))
        st = np.zeros(dev.n, np.int32)
        for i in self.bad_status:
            st[i] = -3
            rows[psz * i:psz * (i + 1)] = b"\xAA" * psz
        return (bytes(rows), bytes(32 * dev.n) if want_jr_seeds else None, None, st)

    def decide_peer(self, agg_id, ctx, peer_rows, peer_ok=None):
        assert agg_id == self._agg
        psz = self.prep_share_size(self._ap[2])
        n = self._dev.n
        assert len(peer_rows) == n * psz
        own = self._rows(agg_id)
        acc = np.zeros(n, np.uint8)
        code = np.full(n, 3, np.uint8)
        for i in range(n):
            if i in self.bad_status or (peer_ok is not None and not peer_ok[i]):
                continue
            code[i] = int(own[psz * i:psz * (i + 1)] == peer_rows[psz * i:psz * (i + 1)])
            acc[i] = code[i] == 1 and not (i in self.reject and self._ap[0] >= self.reject_level)
        self.calls.append(("decide_peer", agg_id, code.copy(), acc.copy()))
        return (acc, code, None)

    def _fold(self, agg_id, prefixes, meas):
        vec = []
        for p in prefixes:
            hit = [w for (a, w) in meas if a[:len(p)] == p]
            vec += [len(hit), sum(hit)] if agg_id == 0 else [0, 0]
        return vec

    def aggregate_device(self, agg_id, enc, valid=None, raw=False):
        assert self.decode_agg_param(enc) == self._ap
        meas = [m for (m, k) in zip(self._dev.meas, valid) if k]
        vec = self._fold(agg_id, self._ap[1], meas)
        return b"".join(v.to_bytes(8, "little") for v in vec) if raw else vec

    def aggregate_grouped(self, agg_id, enc, groups, n_groups, valid=None, raw=False):
        shares = [self._fold(agg_id, self._ap[1], [m for (m, g, k) in zip(self._dev.meas, groups, valid) if k and g == b])
                  for b in range(n_groups)]
        return (shares, np.array([sum(1 for (g, k) in zip(groups, valid) if k and g == b) for b in range(n_groups)]))


class ModelNonceSet:
    """First occurrence wins, by index."""

    def __init__(self, seen=()):
        self.seen = set(seen)

    def admit(self, reports):
        fresh = np.zeros(reports.n, np.uint8)
        for (i, nonce) in enumerate(reports.nonces):
            if nonce not in self.seen:
                self.seen.add(nonce)
                fresh[i] = 1
        return fresh


BITS = 4


def _meas(values, weight=1):
    return [(index(v, BITS), weight) for v in values]


def _enc(level, prefixes=None, wc=None):
    prefixes = prefixes if prefixes is not None else [index(v, level + 1) for v in range(2 ** (level + 1))]
    return Mastic.encode_agg_param(None, (level, tuple(prefixes), level == 0 if wc is None else wc))


def _pair(meas, kw0=None, kw1=None, **agg_kw):
    m0, m1 = FakeMastic(BITS, **(kw0 or {})), FakeMastic(BITS, **(kw1 or {}))
    a0 = Aggregator(m0, 0, b"ctx", bytes(16), FakeReports(meas), **agg_kw)
    a1 = Aggregator(m1, 1, b"ctx", bytes(16), FakeReports(meas), **agg_kw)
    return (a0, a1)


# ------------------------------------------------------------ state machine
def test_call_order_errors():
    (a0, a1) = _pair(_meas([1, 2, 3]))
    for early in (lambda: a0.decide(b""), lambda: a0.settle(b""), a0.agg_share,
                  lambda: a0.aggregate_grouped([0, 0, 0], 1)):
        with pytest.raises(RuntimeError):
            early()
    o0 = a0.offer(_enc(0))
    o1 = a1.offer(_enc(0))
    for wrong in (lambda: a0.offer(_enc(1)), lambda: a0.settle(b""), a0.agg_share):
        with pytest.raises(RuntimeError):
            wrong()
    v0 = a0.decide(o1)
    v1 = a1.decide(o0)
    for wrong in (lambda: a0.offer(_enc(1)), lambda: a0.decide(o1), a0.agg_share):
        with pytest.raises(RuntimeError):
            wrong()
    assert a0.settle(v1).all() and a1.settle(v0).all()
    for wrong in (lambda: a0.decide(o1), lambda: a0.settle(v1)):
        with pytest.raises(RuntimeError):
            wrong()
    assert a0.agg_share(raw=False) == [3, 3, 0, 0] and a1.agg_share(raw=False) == [0, 0, 0, 0]
    assert a0.n_valid == 3 and a0.last_was_cached is False


def test_messages_of_the_wrong_round_or_sender_are_refused():
    (a0, a1) = _pair(_meas([1, 2, 3]))
    (o0, o1) = (a0.offer(_enc(0)), a1.offer(_enc(0)))
    with pytest.raises(ValueError):
        a0.decide(o0)  # its own offer
    other = Aggregator(FakeMastic(BITS), 1, b"ctx", bytes(16), FakeReports(_meas([1, 2])))
    with pytest.raises(ValueError):
        a0.decide(other.offer(_enc(0)))  # n differs
    third = Aggregator(FakeMastic(BITS), 1, b"ctx", bytes(16), FakeReports(_meas([1, 2, 3])))
    with pytest.raises(ValueError):
        a0.decide(third.offer(_enc(0, [index(0, 1)])))  # another agg param
    v0 = a0.decide(o1)
    with pytest.raises(ValueError):
        a0.settle(v0)  # its own verdict
    a0.settle(a1.decide(o0))


def test_is_valid_violations_raise():
    (a0, _a1) = _pair(_meas([1]))
    with pytest.raises(ValueError):
        a0.offer(_enc(0, wc=False))  # the first round must carry the weight check
    (a0, a1) = _pair(_meas([1]))
    run_round(a0, a1, _enc(0))
    for enc in (_enc(0), _enc(1, wc=True)):  # the level must increase; one weight check only
        with pytest.raises(ValueError):
            a0.offer(enc)
    run_round(a0, a1, _enc(2))
    with pytest.raises(ValueError):
        a0.offer(_enc(1))
    with pytest.raises(ValueError):
        a0.offer(_enc(3)[:-2])  # decode_agg_param refuses it


def test_rows_that_are_not_ok_are_zero_on_the_wire():
    (a0, _a1) = _pair(_meas([1, 2, 3, 4, 5]), kw0=dict(bad_status=(1, 3)))
    o = decode_offer(a0.offer(_enc(0)))
    assert o.ok.tolist() == [True, False, True, False, True]
    rows = np.frombuffer(o.rows, np.uint8).reshape(5, 40)
    assert not rows[[1, 3]].any() and rows[[0, 2, 4]].any(axis=1).all()
    assert b"\xAA" * 8 not in o.rows


def test_peer_verdict_drops_a_report_the_own_side_accepted():
    (a0, a1) = _pair(_meas([5, 5, 5, 9]), kw1=dict(reject=(2,)))
    (o0, o1) = (a0.offer(_enc(0)), a1.offer(_enc(0)))
    (v0, v1) = (a0.decide(o1), a1.decide(o0))
    assert decode_verdict(v0).accept.tolist() == [True] * 4  # the own accept of report 2 is 1
    assert a0.mastic.calls[-1][3].tolist() == [1, 1, 1, 1]
    assert decode_verdict(v1).accept.tolist() == [True, True, False, True]
    assert a0.settle(v1).tolist() == a1.settle(v0).tolist() == [True, True, False, True]
    assert a0.agg_share(raw=False) == [2, 2, 1, 1] and a0.n_valid == a1.n_valid == 3


def test_tampered_and_bad_status_reports_drop_on_both_sides():
    (a0, a1) = _pair(_meas([1, 1, 1, 1, 1]), kw0=dict(tamper=(0,)), kw1=dict(bad_status=(4,)))
    alive = run_round(a0, a1, _enc(0))
    assert alive.tolist() == [False, True, True, True, False]
    assert a0.mastic.calls[-1][2].tolist() == [0, 1, 1, 1, 3]  # the peer did not offer report 4
    assert a1.mastic.calls[-1][2].tolist() == [0, 1, 1, 1, 3]  # its own status is nonzero
    # dead reports are neither offered nor decided in the next round
    (o0, o1) = (a0.offer(_enc(1)), a1.offer(_enc(1)))
    assert decode_offer(o0).ok.tolist() == decode_offer(o1).ok.tolist() == [False, True, True, True, False]
    (v0, v1) = (a0.decide(o1), encode_verdict(1, [False, True, True, True, False]))
    assert a0.mastic.calls[-1][2].tolist() == [3, 1, 1, 1, 3]
    assert a0.settle(v1).sum() == 3 and v0


def test_replay_is_dropped_by_one_set_and_through_ok_on_the_other_side():
    meas = _meas([3, 3, 3, 3])
    nonces = [bytes([i]) * 16 for i in range(4)]
    ns0 = ModelNonceSet(seen=[nonces[2]])  # aggregator 0 has seen report 2 before; aggregator 1 has not
    ns1 = ModelNonceSet()
    a0 = Aggregator(FakeMastic(BITS), 0, b"ctx", bytes(16), FakeReports(meas, nonces), nonce_set=ns0)
    a1 = Aggregator(FakeMastic(BITS), 1, b"ctx", bytes(16), FakeReports(meas, nonces), nonce_set=ns1)
    assert a0.alive.tolist() == [True, True, False, True] and a1.alive.all()
    (o0, o1) = (a0.offer(_enc(0)), a1.offer(_enc(0)))
    assert decode_offer(o0).ok.tolist() == [True, True, False, True] and decode_offer(o1).ok.all()
    assert not np.frombuffer(decode_offer(o0).rows, np.uint8).reshape(4, 40)[2].any()
    (v0, v1) = (a0.decide(o1), a1.decide(o0))
    assert a1.mastic.calls[-1][2].tolist() == [1, 1, 3, 1]
    assert a0.settle(v1).tolist() == a1.settle(v0).tolist() == [True, True, False, True]
    assert a0.agg_share(raw=False) == [3, 3, 0, 0]
    assert nonces[2] in ns1.seen and all(x in ns0.seen for x in nonces)


def test_a_list_is_uploaded_once_with_the_own_share_only():
    reports = [(bytes([i]) * 16, b"pub%d" % i, bytes([v, 2])) for (i, v) in enumerate([7, 7, 8])]
    aggs = []
    for agg_id in range(2):
        m = FakeMastic(BITS)
        aggs.append(Aggregator(m, agg_id, b"ctx", bytes(16), reports, frontier_cache=True))
        (nonces, pubs, in0, in1) = m.uploads[0]
        assert len(m.uploads) == 1 and nonces == b"".join(r[0] for r in reports) and pubs == b"pub0pub1pub2"
        assert (in0, in1)[agg_id] == bytes([7, 2, 7, 2, 8, 2]) and (in0, in1)[1 - agg_id] is None
        assert ("set_frontier_cache", True) in m.calls
    run_round(aggs[0], aggs[1], _enc(0))
    assert aggs[0].agg_share(raw=False) == [2, 4, 1, 2]
    (shares, counts) = aggs[0].aggregate_grouped([0, 1, 0], 2)
    assert shares == [[1, 2, 1, 2], [1, 2, 0, 0]] and counts.tolist() == [2, 1]
    empty = Aggregator(FakeMastic(BITS), 0, b"ctx", bytes(16), [])
    assert empty.n == 0 and empty.reports is None


def test_compaction_after_admit_and_after_the_first_round():
    meas = _meas([2, 2, 2, 2, 2, 13])
    nonces = [bytes([i]) * 16 for i in (0, 1, 1, 2, 3, 4)]  # report 2 repeats report 1's nonce
    aggs = []
    for agg_id in range(2):
        m = FakeMastic(BITS, tamper=(3,) if agg_id == 0 else ())  # index 3 of the compacted batch
        aggs.append(Aggregator(m, agg_id, b"ctx", bytes(16), FakeReports(meas, nonces), nonce_set=ModelNonceSet(),
                               compact=0.0))
        assert aggs[-1].n == 5 and aggs[-1].reports.compactions == 1
    alive = run_round(aggs[0], aggs[1], _enc(0))
    assert alive.tolist() == [True, True, True, False, True]
    assert aggs[0].agg_share(raw=False) == [3, 3, 1, 1] and aggs[0].n == 5  # the fold sees the round's numbering
    alive = run_round(aggs[0], aggs[1], _enc(1))
    assert alive.tolist() == [True] * 4 and aggs[0].n == aggs[1].n == 4 and aggs[0].reports.compactions == 2
    run_round(aggs[0], aggs[1], _enc(2))
    assert aggs[0].reports.compactions == 2  # later rejections stay masked
    with pytest.raises(ValueError):
        Aggregator(FakeMastic(BITS), 0, b"ctx", bytes(16), FakeReports(meas), compact=1.5)


@pytest.mark.parametrize("compact", [None, 0.0])
def test_lockstep_sweep_matches_plaintext(compact):
    import random
    rng = random.Random(5)
    bits = 6
    heavy = [rng.randrange(2 ** bits) for _ in range(3)]
    meas = [(index(rng.choice(heavy) if rng.random() < 0.6 else rng.randrange(2 ** bits), bits), rng.randrange(1, 3))
            for _ in range(150)]
    th = {'default': 10, index(0b1, 1): 14}
    good = [m for (i, m) in enumerate(meas) if i not in (4, 77)]
    trace = []
    a0 = Aggregator(FakeMastic(bits, tamper=(4,)), 0, b"ctx", bytes(16), FakeReports(meas), compact=compact)
    a1 = Aggregator(FakeMastic(bits, bad_status=(77,)), 1, b"ctx", bytes(16), FakeReports(meas), compact=compact)
    got = sweep_lockstep(a0, a1, th, trace)
    assert got == plain_heavy_hitters(good, th, bits) and got
    assert [t.agg_result for t in trace] == [plain_sums(good, t.prefixes) for t in trace]
    assert all(t.n_valid == 148 for t in trace) and [t.level for t in trace] == list(range(bits))
    assert a0.n == (148 if compact is not None else 150)
    # an empty batch sweeps to nothing without a round
    e0, e1 = (Aggregator(FakeMastic(bits), i, b"ctx", bytes(16), []) for i in range(2))
    assert sweep_lockstep(e0, e1, th) == [] and e0.mastic.calls == []


# ---------------------------------------------------------------- boundary
def test_header_declares_the_entry_point_and_the_code():
    text = open(os.path.join(ROOT, "include", "mastic_hip.h")).read()
    assert re.search(r"\bint\s+mastic_decide_peer\s*\(\s*mastic_ctx\s*\*\s*ctx,\s*int agg_id,", text)
    assert re.search(r"#define\s+MASTIC_DECIDE_SKIPPED\s+3\b", text)
    assert "mastic_decide_peer" in _lib.EXPORTS


def test_library_exports_it_and_refuses_a_null_ctx():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mastic_decide_peer")
    fn = lib.mastic_decide_peer
    fn.restype = ctypes.c_int
    P = ctypes.c_void_p
    fn.argtypes = [P, ctypes.c_int, P, ctypes.c_size_t, P, P, ctypes.c_size_t, P, P, P]
    assert fn(None, 0, None, 0, None, None, 0, None, None, None) == -22
    import mastic_amd
    assert mastic_amd.Aggregator is Aggregator


def test_an_empty_batch_rounds_and_folds_to_zeros():
    e0, e1 = (Aggregator(FakeMastic(BITS), i, b"ctx", bytes(16), []) for i in range(2))
    assert run_round(e0, e1, _enc(0)).size == 0
    assert e0.agg_share(raw=False) == Field64.zeros(4) and e0.agg_share(raw=True) == bytes(32)
    (shares, counts) = e0.aggregate_grouped([], 3, raw=True)
    assert shares == [bytes(32)] * 3 and counts.tolist() == [0, 0, 0]
    assert e0.aggregate_grouped([], 2)[0] == [Field64.zeros(4)] * 2
    assert e0.mastic.calls == [] and e0.n_valid == 0
