"""The reject side of prep_shares_to_prep (k_decide / flp_decide) and of the
accept mask (k_accept), per circuit and per element.  Honest reports cannot
show a decide that is too lenient, so every case here edits honest prep
shares and compares each GPU code with the oracle's prep_shares_to_prep on
the same bytes (decode_prep_share, then 'VIDPF verification failed' -> 0,
'FLP verification failed' -> 2, a prep message -> 1).

One batch per kind of edit, report i carrying edit i, the last two reports of
every batch unedited (controls: code 1, message equal to the oracle's).  The
honest prep_init runs once per circuit and is shared by its cases.
"""
import functools
import random

import numpy as np
import pytest

from test_gpu_parity import CASES, CTX, _oracle_for, _random_reports, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

IDS = [c for (c, _) in CASES]
VIDPF_FAIL, OK, FLP_FAIL = 0, 1, 2


class _Honest:
    def __init__(self, mastic_amd, circuit):
        kw = dict(dict(CASES)[circuit])
        bits = kw.pop("bits")
        self.m = m = mastic_amd.Mastic(bits, circuit, **kw)
        self.o = o = _oracle_for(m)
        rng = random.Random(1000 + sum(map(ord, circuit)))
        self.vlen = o.flp.VERIFIER_LEN
        self.n = n = max(self.vlen, 32) + 2
        (self.alphas, weights, self.nonces, rands) = _random_reports(m, rng, n)
        (self.pub, self.in0, self.in1) = m.shard_batch(CTX, self.alphas, weights, self.nonces, rands)
        self.vk = bytes(rng.getrandbits(8) for _ in range(32))
        self.ap = (0, ((False,), (True,)), True)
        self.res = [m.prep_init_batch(self.vk, CTX, a, self.ap, self.nonces, self.pub, self.in0 if a == 0 else self.in1)
                    for a in range(2)]
        assert all(not np.any(r[3]) for r in self.res)
        self.psz = m.prep_share_size(True)
        self.jr = 32 if o.flp.JOINT_RAND_LEN > 0 else 0
        self.enc = o.field.ENCODED_SIZE
        self.p = o.field.MODULUS

    def shares(self, a, k):
        """The first k reports' prep shares of aggregator a, one bytearray each."""
        return [bytearray(self.res[a][0][self.psz * i:self.psz * (i + 1)]) for i in range(k)]

    def ver_at(self, e):
        return 32 + self.jr + e * self.enc

    def oracle(self, s0, s1, ap=None):
        """The oracle's verdict on one pair of encoded prep shares: (code, message or None)."""
        o = self.o
        ap = ap or self.ap
        try:
            shares = [o.decode_prep_share(ap[2], bytes(s0)), o.decode_prep_share(ap[2], bytes(s1))]
        except ValueError as e:
            return ("decode: %s" % e, None)
        try:
            return (OK, o.prep_shares_to_prep(CTX, ap, shares))
        except Exception as e:  # the reference raises plain Exception for both verdicts
            return ({"VIDPF verification failed": VIDPF_FAIL, "FLP verification failed": FLP_FAIL}[str(e)], None)

    def decide(self, sh0, sh1, ap=None):
        (msgs, codes) = self.m.decide_batch(CTX, ap or self.ap, b"".join(bytes(s) for s in sh0),
                                            b"".join(bytes(s) for s in sh1))
        return (msgs, list(codes))

    def check_controls(self, sh0, sh1, msgs, codes):
        k = len(sh0)
        for i in (k - 2, k - 1):
            (code, msg) = self.oracle(sh0[i], sh1[i])
            assert code == OK and codes[i] == OK, "control %d" % i
            if msg is not None:
                assert msgs[32 * i:32 * (i + 1)] == msg


@functools.lru_cache(maxsize=None)
def _honest(mastic_amd, circuit):  # noqa: F811
    return _Honest(mastic_amd, circuit)


@pytest.fixture(scope="module", autouse=True)
def _drop_honest():
    yield
    _honest.cache_clear()  # the contexts go with the module, not at interpreter exit


@pytest.mark.parametrize("circuit", IDS)
def test_every_verifier_element_is_looked_at(mastic_amd, circuit):  # noqa: F811
    """Verifier element e of report e becomes element + 1 mod p, for every e:
    a decide that ignores any one element accepts that report."""
    h = _honest(mastic_amd, circuit)
    k = h.vlen + 2
    (sh0, sh1) = (h.shares(0, k), h.shares(1, k))
    for e in range(h.vlen):
        at = h.ver_at(e)
        x = int.from_bytes(sh0[e][at:at + h.enc], "little")
        sh0[e][at:at + h.enc] = ((x + 1) % h.p).to_bytes(h.enc, "little")
    honest = h.shares(0, k)
    edited = [i for i in range(k) if sh0[i] != honest[i]]
    assert edited == list(range(h.vlen)), "one report per verifier element"
    assert h.ver_at(h.vlen) == h.psz
    (msgs, codes) = h.decide(sh0, sh1)
    want = [h.oracle(sh0[i], sh1[i])[0] for i in range(k)]
    assert want == [FLP_FAIL] * h.vlen + [OK, OK]
    assert codes == want
    h.check_controls(sh0, sh1, msgs, codes)


@pytest.mark.parametrize("both", [False, True], ids=["proof-only", "proof-and-verifier"])
@pytest.mark.parametrize("circuit", IDS)
def test_eval_proof_bits_and_vidpf_precedence(mastic_amd, circuit, both):  # noqa: F811
    """One bit flipped in each of the 32 eval-proof bytes: code 0.  With a
    verifier element edited as well the code stays 0: the reference raises the
    VIDPF error before it looks at the FLP."""
    h = _honest(mastic_amd, circuit)
    k = 34
    (sh0, sh1) = (h.shares(0, k), h.shares(1, k))
    for b in range(32):
        sh0[b][b] ^= 1 << (b % 8)
        if both:
            at = h.ver_at(b % h.vlen)
            x = int.from_bytes(sh0[b][at:at + h.enc], "little")
            sh0[b][at:at + h.enc] = ((x + 1) % h.p).to_bytes(h.enc, "little")
    (msgs, codes) = h.decide(sh0, sh1)
    want = [h.oracle(sh0[i], sh1[i])[0] for i in range(k)]
    assert want == [VIDPF_FAIL] * 32 + [OK, OK]
    assert codes == want
    h.check_controls(sh0, sh1, msgs, codes)


@pytest.mark.parametrize("circuit", IDS)
def test_out_of_range_verifier_element(mastic_amd, circuit):  # noqa: F811
    """A verifier element set to p or to all-ones, first and last element, in
    either aggregator's share (both fields over the five circuits).  The
    oracle's decoder raises for such a share; the GPU's answer is code 2.
    In the second half of the batch the other aggregator's element is adjusted
    so that the two still sum to the honest value mod p: there only the range
    test itself can tell (a decide that adds first and looks at the sum
    accepts)."""
    h = _honest(mastic_amd, circuit)
    edits = [(a, e, v, comp) for comp in (False, True) for a in range(2) for e in (0, h.vlen - 1)
             for v in (h.p, (1 << (8 * h.enc)) - 1)]
    k = len(edits) + 2
    assert k <= h.n
    sh = [h.shares(0, k), h.shares(1, k)]
    for (i, (a, e, v, comp)) in enumerate(edits):
        at = h.ver_at(e)
        honest = sum(int.from_bytes(sh[b][i][at:at + h.enc], "little") for b in range(2)) % h.p
        sh[a][i][at:at + h.enc] = v.to_bytes(h.enc, "little")
        if comp:
            sh[1 - a][i][at:at + h.enc] = ((honest - v) % h.p).to_bytes(h.enc, "little")
    (msgs, codes) = h.decide(sh[0], sh[1])
    for i in range(len(edits)):
        (verdict, _msg) = h.oracle(sh[0][i], sh[1][i])
        assert verdict == "decode: encoded element out of range", (i, verdict)
    assert codes == [FLP_FAIL] * len(edits) + [OK, OK]
    h.check_controls(sh[0], sh[1], msgs, codes)


JR_IDS = [c for c in IDS if c in ("SumVec", "Histogram", "MultihotCountVec")]


@pytest.mark.parametrize("agg", [0, 1])
@pytest.mark.parametrize("circuit", JR_IDS)
def test_joint_rand_part_bits(mastic_amd, circuit, agg):  # noqa: F811
    """A bit flipped in each of the 32 joint-rand-part bytes of one
    aggregator's prep share: decide still says 1 (the parts are not checked
    there), the prep message equals the oracle's, and the confirmation against
    the aggregators' own seeds fails.  The same flip applied to the *uploaded*
    peer part in the other aggregator's input share is refused by the accept
    mask of decide_results."""
    from mastic_amd.heavy_hitters import joint_rand_confirmed
    h = _honest(mastic_amd, circuit)
    assert h.jr == 32
    k = 34
    sh = [h.shares(0, k), h.shares(1, k)]
    for b in range(32):
        sh[agg][b][32 + b] ^= 1 << (b % 8)
    (msgs, codes) = h.decide(sh[0], sh[1])
    assert codes == [OK] * k
    for i in range(k):
        (code, msg) = h.oracle(sh[0][i], sh[1][i])
        assert code == OK and msgs[32 * i:32 * (i + 1)] == msg, i
    conf = joint_rand_confirmed(msgs, h.res[0][1][:32 * k], h.res[1][1][:32 * k], k)
    assert list(conf) == [False] * 32 + [True, True]
    # aggregator `agg`'s part travels to the other aggregator inside its input share (the last 32 bytes)
    m = h.m
    ins = [bytearray(h.in0[:m.input_share_size(0) * k]), bytearray(h.in1[:m.input_share_size(1) * k])]
    other = 1 - agg
    isz = m.input_share_size(other)
    for b in range(32):
        ins[other][isz * b + isz - 32 + b] ^= 1 << (b % 8)
    dev = m.reports_upload(h.nonces[:16 * k], h.pub[:m.public_share_size() * k], bytes(ins[0]), bytes(ins[1]))
    enc_ap = m.encode_agg_param(h.ap)
    for a in range(2):
        m.prep_init_device(dev, h.vk, CTX, a, enc_ap)
    (acc, _codes) = m.decide_results(CTX, k)
    assert list(acc) == [0] * 32 + [1, 1]


@pytest.mark.parametrize("circuit", IDS)
def test_without_weight_check_at_a_middle_level(mastic_amd, circuit):  # noqa: F811
    """weight_check=False: the share is the eval proof alone, so only proof
    bytes can be edited; shares of any other length are refused."""
    h = _honest(mastic_amd, circuit)
    (m, o) = (h.m, h.o)
    level = m.BITS // 2
    k = 34
    ap = (level, tuple(dict.fromkeys(a[:level + 1] for a in h.alphas[:k]))[:5], False)
    res = [m.prep_init_batch(h.vk, CTX, a, ap, h.nonces[:16 * k], h.pub[:m.public_share_size() * k],
                             (h.in0 if a == 0 else h.in1)[:m.input_share_size(a) * k])[0] for a in range(2)]
    assert m.prep_share_size(False) == 32 and len(res[0]) == 32 * k
    sh = [[bytearray(r[32 * i:32 * (i + 1)]) for i in range(k)] for r in res]
    for b in range(32):
        sh[b % 2][b][b] ^= 0x80 >> (b % 8)
    (_msgs, codes) = h.decide(sh[0], sh[1], ap)
    want = [h.oracle(sh[0][i], sh[1][i], ap)[0] for i in range(k)]
    assert want == [VIDPF_FAIL] * 32 + [OK, OK]
    assert codes == want
    # wrong lengths: the weight-check share for this agg param, a truncated batch, unequal batches
    with_wc = bytes(h.shares(0, 1)[0])
    assert h.oracle(with_wc, with_wc, ap)[0] == "decode: prep share has incorrect length"
    for (s0, s1) in [(res[0] + b"\0", res[1] + b"\0"), (res[0][:-1], res[1][:-1]), (res[0], res[1] + bytes(32)),
                     (with_wc + b"\0", with_wc + b"\0")]:
        with pytest.raises(ValueError, match="incorrect length"):
            m.decide_batch(CTX, ap, s0, s1)
