"""``Mastic.decide_peer`` (mastic_decide_peer, k_decide_peer): one aggregator
decides where its own result lies in HBM, against the other's wire prep shares.

Every expectation comes from a path that is pinned elsewhere: the golden
vectors, ``decide_batch`` on the two host wire shares plus the joint-rand
confirmation against the own seed and the own status (the ``_decide_on_wire``
formula of mastic_amd/rounds.py, one side at a time), and ``decide_results``
of a third ctx that ran both aggregators.

Three ctxs per circuit: A holds only aggregator 0's input shares, B only
aggregator 1's, C both.  A wire edit exists only between the two parties (the
peer's rows as the deciding side receives them), so C, which never sees it, is
compared on the rows that carry none: honest reports, the report with the
non-canonical public share, and a report whose helper key was flipped before
the upload.
"""
import functools
import json
import os
import random

import numpy as np
import pytest

from conftest import golden_files
from mastic_amd.rounds import joint_rand_confirmed
from test_gpu_parity import CTX, _random_reports, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

VIDPF_FAIL, OK, FLP_FAIL, SKIPPED = 0, 1, 2, 3
EINVAL = -22
CIRCUITS = [
    ("Count", dict()),
    ("Sum", dict(max_measurement=255)),
    ("SumVec", dict(length=5, sum_vec_bits=3, chunk_length=4)),
    ("Histogram", dict(length=7, chunk_length=3)),
    ("MultihotCountVec", dict(length=6, max_measurement=3, chunk_length=2)),
    # a row too wide for the kernel's LDS staging: every lane loads its own row (DECIDE_PEER_LDS_WORDS in csrc/)
    ("Histogram-wide", dict(length=12, chunk_length=6)),
]
LDS_ROW_BYTES = 63 * 4  # rows up to this size are staged through LDS, wider ones are not
WIDE = ("Histogram-wide",)
BITS = 4
N_MAX = 257
BUDGET = 1 << 30  # HBM work budget per ctx: several ctxs are alive at once, and the default is most of the free HBM
SIZES = [1, 63, 64, 65, 257]  # the wave edge, the stride padding, a second 256-thread block


# ------------------------------------------------------------ golden vectors
@pytest.mark.parametrize("path", golden_files(), ids=os.path.basename)
def test_golden_vectors_one_share_per_ctx(mastic_amd, path):  # noqa: F811
    tv = json.load(open(path))
    (ctx, vk, enc) = (bytes.fromhex(tv["ctx"]), bytes.fromhex(tv["verify_key"]), bytes.fromhex(tv["agg_param"]))
    reps = tv["prep"]
    n = len(reps)
    nonces = b"".join(bytes.fromhex(r["nonce"]) for r in reps)
    pub = b"".join(bytes.fromhex(r["public_share"]) for r in reps)
    ins = [b"".join(bytes.fromhex(r["input_shares"][a]) for r in reps) for a in range(2)]
    ms = [mastic_amd.from_test_vec(tv) for _ in range(2)]
    for m in ms:
        m.set_memory_budget(BUDGET)
    devs = [ms[0].reports_upload(nonces, pub, ins[0], None), ms[1].reports_upload(nonces, pub, None, ins[1])]
    rows = []
    for a in range(2):
        with pytest.raises(ValueError, match="no input shares"):
            ms[a].prep_init_device(devs[a], vk, ctx, 1 - a, enc)
        ms[a].prep_init_device(devs[a], vk, ctx, a, enc)
        (ps, _js, _out, st) = ms[a].prep_result(devs[a], a, enc)
        assert ps == b"".join(bytes.fromhex(r["prep_shares"][0][a]) for r in reps) and not st.any()
        rows.append(ps)
    has_msg = any(r["prep_messages"][0] for r in reps)
    for a in range(2):
        (accept, codes, msgs) = ms[a].decide_peer(a, ctx, rows[1 - a])
        assert accept.dtype == codes.dtype == np.uint8
        assert accept.tolist() == [1] * n and codes.tolist() == [OK] * n
        assert (msgs is not None) == has_msg
        for (i, r) in enumerate(reps):
            if r["prep_messages"][0]:
                assert msgs[32 * i:32 * (i + 1)].tobytes().hex() == r["prep_messages"][0]
        # the same with an explicit all-ones peer_ok
        (accept, codes, _m) = ms[a].decide_peer(a, ctx, rows[1 - a], np.ones(n, np.uint8))
        assert accept.tolist() == [1] * n and codes.tolist() == [OK] * n


# ------------------------------------------------------- tampered batches
class _Trio:
    """Ctxs A, B, C of one circuit and N_MAX sharded reports."""

    def __init__(self, mastic_amd, circuit):  # noqa: F811
        kw = dict(CIRCUITS)[circuit]
        self.ms = [mastic_amd.Mastic(BITS, circuit.split("-")[0], **kw) for _ in range(3)]
        for m in self.ms:
            m.set_memory_budget(BUDGET)
        rng = random.Random(4000 + sum(map(ord, circuit)))
        (self.alphas, weights, self.nonces, rands) = _random_reports(m, rng, N_MAX)
        (self.pub, self.in0, self.in1) = m.shard_batch(CTX, self.alphas, weights, self.nonces, rands)
        self.vk = bytes(rng.getrandbits(8) for _ in range(32))
        self.jr = m.JOINT_RAND_LEN > 0
        self.p = m.field.MODULUS
        self.enc = m.field.ENCODED_SIZE
        self.vlen = m.VERIFIER_LEN
        assert self.jr == (circuit.split("-")[0] in ("SumVec", "Histogram", "MultihotCountVec"))
        # both sides of the kernel's dispatch on the row size are pinned
        assert m.prep_share_size(False) == 32
        assert (m.prep_share_size(True) > LDS_ROW_BYTES) == (circuit in WIDE), m.prep_share_size(True)
        assert self.enc == (16 if self.jr else 8)

    def agg_param(self, level):
        if level == 0:
            return (0, ((False,), (True,)), True)
        return (level, tuple(dict.fromkeys(a[:level + 1] for a in self.alphas))[:3], False)


@functools.lru_cache(maxsize=1)  # the cases of one circuit run together
def _trio(mastic_amd, circuit):  # noqa: F811
    return _Trio(mastic_amd, circuit)


@pytest.fixture(scope="module", autouse=True)
def _drop_trios():
    yield
    _trio.cache_clear()


def _kinds(wc, jr):
    """The edits, in the order they rotate over the marked indices."""
    if not wc:  # the share is the eval proof alone
        return ["proof-bit", "peer-not-ok", "own-status", "proof-bit-last"]
    return ["proof-bit", "verifier-bit", "verifier-p"] + (["jr-part-bit"] if jr else []) + ["peer-not-ok", "own-status"]


def _edit_row(t, row, kind):
    """Apply a wire edit to the peer's row (bytearray view), in place."""
    ver = 32 + (32 if t.jr else 0)
    if kind == "proof-bit":
        row[5] ^= 0x10
    elif kind == "proof-bit-last":
        row[31] ^= 0x80
    elif kind == "verifier-bit":
        row[ver + t.enc * (t.vlen // 2) + 3] ^= 0x04
    elif kind == "verifier-p":
        at = ver + t.enc * (t.vlen - 1)
        row[at:at + t.enc] = t.p.to_bytes(t.enc, "little")
    elif kind == "jr-part-bit":
        row[32 + 17] ^= 0x01
    else:
        raise AssertionError(kind)


def _run_rotation(t, ap, n, marks, status_at, key_at):
    """One upload of the first n reports on A, B and C (report ``status_at``
    with a non-canonical payload correction word, report ``key_at`` with a bit
    of its helper key flipped), prep_init, and each side's decide_peer against
    the other's rows with the wire edits ``marks`` ({index: kind})."""
    (mA, mB, mC) = t.ms
    m = mC
    wc = ap[2]
    enc_ap = m.encode_agg_param(ap)
    psz = m.prep_share_size(wc)
    pub = bytearray(t.pub[:m.public_share_size() * n])
    in0 = t.in0[:m.input_share_size(0) * n]
    in1 = bytearray(t.in1[:m.input_share_size(1) * n])
    if status_at is not None:  # payload correction word of level 0, first element := p
        at = m.public_share_size() * status_at + (2 * BITS + 7) // 8 + 16 * BITS
        pub[at:at + t.enc] = t.p.to_bytes(t.enc, "little")
    if key_at is not None:
        in1[m.input_share_size(1) * key_at + 2] ^= 0x08
    (pub, in1, nonces) = (bytes(pub), bytes(in1), t.nonces[:16 * n])
    devs = [mA.reports_upload(nonces, pub, in0, None), mB.reports_upload(nonces, pub, None, in1),
            mC.reports_upload(nonces, pub, in0, in1)]
    res = []
    for a in range(2):
        t.ms[a].prep_init_device(devs[a], t.vk, CTX, a, enc_ap)
        mC.prep_init_device(devs[2], t.vk, CTX, a, enc_ap)
        res.append(t.ms[a].prep_result(devs[a], a, enc_ap))
    (acc_c, _codes_c) = mC.decide_results(CTX, n)
    for a in range(2):
        want_status = np.zeros(n, np.int32)
        if status_at is not None:
            want_status[status_at] = -3
        assert res[a][3].tolist() == want_status.tolist()
    accepts = []
    for a in range(2):
        (own_rows, own_seeds, _out, own_status) = res[a]
        peer = bytearray(res[1 - a][0])
        peer_ok = np.ones(n, np.uint8)
        for (i, kind) in marks.items():
            if kind == "peer-not-ok":
                peer_ok[i] = 0
                peer[psz * i:psz * (i + 1)] = bytes(psz)  # as it crosses the wire
            elif kind != "own-status":
                row = peer[psz * i:psz * (i + 1)]
                _edit_row(t, row, kind)
                peer[psz * i:psz * (i + 1)] = row
        peer = bytes(peer)
        # expected: decide_batch on the pair in aggregator order, then this side's prep_next
        pair = (own_rows, peer) if a == 0 else (peer, own_rows)
        (want_msgs, want_codes) = mC.decide_batch(CTX, ap, pair[0], pair[1])
        skipped = (own_status != 0) | (peer_ok == 0)
        want_codes = np.where(skipped, SKIPPED, want_codes)
        want_accept = (want_codes == OK)
        want_msgs = np.frombuffer(want_msgs, np.uint8).reshape(n, 32) * (~skipped)[:, None]
        if wc and t.jr:
            want_accept &= joint_rand_confirmed(want_msgs.tobytes(), own_seeds, own_seeds, n)
        (accept, codes, msgs) = t.ms[a].decide_peer(a, CTX, peer, peer_ok)
        assert codes.tolist() == want_codes.tolist()
        assert accept.tolist() == want_accept.astype(np.uint8).tolist()
        if wc and t.jr:
            assert msgs.reshape(n, 32).tolist() == want_msgs.tolist()
            assert not msgs.reshape(n, 32)[skipped].any()
        else:
            assert msgs is None
        # what each kind must give, whatever the formula says
        for (i, kind) in marks.items():
            if kind in ("peer-not-ok", "own-status"):
                assert (codes[i], accept[i]) == (SKIPPED, 0), (i, kind)
            elif kind.startswith("proof-bit"):
                assert (codes[i], accept[i]) == (VIDPF_FAIL, 0), (i, kind)
            elif kind.startswith("verifier"):
                assert (codes[i], accept[i]) == (FLP_FAIL, 0), (i, kind)
            else:
                assert (codes[i], accept[i]) == (OK, 0), (i, kind)
        if key_at is not None:
            assert (codes[key_at], accept[key_at]) == (VIDPF_FAIL, 0)
        accepts.append(accept)
    # rows both sides offer and no wire edit touches: both verdicts together are C's decide_results
    wire_edited = np.zeros(n, bool)
    for (i, kind) in marks.items():
        wire_edited[i] = kind != "own-status"
    both = (accepts[0] & accepts[1])[~wire_edited]
    assert both.tolist() == acc_c[~wire_edited].tolist()
    honest = ~wire_edited
    for i in (status_at, key_at):
        if i is not None:
            honest[i] = False
            assert acc_c[i] == 0
    assert acc_c[honest].all() and accepts[0][honest].all() and accepts[1][honest].all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("circuit", [c for (c, _) in CIRCUITS])
def test_parity_on_tampered_batches(mastic_amd, circuit, level, n):  # noqa: F811
    """Both agg_ids in every case.  The edits rotate over the indices 0, 63,
    64 and n-1, so each of those lanes carries each kind once."""
    t = _trio(mastic_amd, circuit)
    ap = t.agg_param(level)
    kinds = _kinds(ap[2], t.jr)
    at = sorted({i for i in (0, 63, 64, n - 1) if i < n})
    key_at = n // 2 if n // 2 not in at else None
    for k in range(len(kinds)):
        marks = {i: kinds[(j + k) % len(kinds)] for (j, i) in enumerate(at)}
        status_at = next((i for (i, kind) in marks.items() if kind == "own-status"), None)
        _run_rotation(t, ap, n, marks, status_at, key_at)


# ----------------------------------------------------------------- errors
def _raw_decide_peer(m, agg_id, rows, n):
    from mastic_amd import _lib
    return _lib.lib().mastic_decide_peer(m._ctx, agg_id, CTX, len(CTX), _lib.buf(rows), None, n, None, None, None)


def test_errors_are_einval(mastic_amd):  # noqa: F811
    t = _trio(mastic_amd, "Sum")
    mC = t.ms[2]
    n = 5
    ap = t.agg_param(0)
    m = mC
    (pub, in0, in1) = (t.pub[:m.public_share_size() * n], t.in0[:m.input_share_size(0) * n],
                       t.in1[:m.input_share_size(1) * n])
    dev = mC.reports_upload(t.nonces[:16 * n], pub, in0, in1)
    mC.prep_init_device(dev, t.vk, CTX, 1, ap)
    rows1 = mC.prep_result(dev, 1, ap)[0]
    fresh = mastic_amd.MasticSum(BITS, 255)
    fresh.set_memory_budget(BUDGET)
    devf = fresh.reports_upload(t.nonces[:16 * n], pub, in0, None)
    fresh.prep_init_device(devf, t.vk, CTX, 0, ap)
    psz = fresh.prep_share_size(True)
    assert fresh.decide_peer(0, CTX, rows1)[0].tolist() == [1] * n
    # n off by one, either way (the buffer is large enough for both)
    big = rows1 + bytes(psz)
    assert _raw_decide_peer(fresh, 0, big, n - 1) == EINVAL
    assert _raw_decide_peer(fresh, 0, big, n + 1) == EINVAL
    assert _raw_decide_peer(fresh, 0, big, n) == 0
    for rows in (rows1[:-psz], big):
        with pytest.raises(ValueError):
            fresh.decide_peer(0, CTX, rows)
    with pytest.raises(ValueError):
        fresh.decide_peer(0, CTX, rows1[:-1])
    with pytest.raises(ValueError):
        fresh.decide_peer(0, CTX, rows1, np.ones(n + 1, np.uint8))
    # a slot that is not ready, and an agg_id that is none
    assert _raw_decide_peer(fresh, 1, big, n) == EINVAL
    assert _raw_decide_peer(fresh, 2, big, n) == EINVAL
    assert _raw_decide_peer(fresh, -1, big, n) == EINVAL
    for agg_id in (1, 2):
        with pytest.raises(ValueError):
            fresh.decide_peer(agg_id, CTX, rows1)
    # the ctx is as good as before
    assert fresh.decide_peer(0, CTX, rows1)[1].tolist() == [OK] * n


@pytest.mark.parametrize("circuit", ["Sum", "Histogram", "Histogram-wide"])
def test_the_other_aggregators_slot_is_untouched(mastic_amd, circuit):  # noqa: F811
    t = _trio(mastic_amd, circuit)
    m = t.ms[2]
    n = 70
    ap = t.agg_param(0)
    dev = m.reports_upload(t.nonces[:16 * n], t.pub[:m.public_share_size() * n], t.in0[:m.input_share_size(0) * n],
                           t.in1[:m.input_share_size(1) * n])
    for a in range(2):
        m.prep_init_device(dev, t.vk, CTX, a, ap)
    before = [m.prep_result(dev, a, ap, want_out_shares=True) for a in range(2)]
    (want_acc, want_codes) = m.decide_results(CTX, n)
    for a in range(2):
        (accept, codes, _msgs) = m.decide_peer(a, CTX, before[1 - a][0])
        assert accept.tolist() == want_acc.tolist() == [1] * n and codes.tolist() == want_codes.tolist()
        after = [m.prep_result(dev, b, ap, want_out_shares=True) for b in range(2)]
        for b in range(2):
            assert after[b][:3] == before[b][:3] and after[b][3].tolist() == before[b][3].tolist()
    aggs = [m.aggregate_device(a, ap, raw=True) for a in range(2)]
    assert aggs[0] != aggs[1]
