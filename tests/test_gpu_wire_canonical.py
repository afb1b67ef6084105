"""Non-canonical wire field elements (>= p) in a report's public share or
leader proof share.  The reference's decoders raise ValueError("encoded
element out of range") for such a report (vdaf_poc field.py decode_vec, via
Vidpf.decode_public_share over the *whole* share and the input-share decoder),
so the expected behaviour is: that report is rejected -- by every aggregator
whose input holds the element, at every level, also when the element sits
deeper than the call's level -- and nothing else changes.

Each case builds 65 honest reports (one full wave and a one-report tail),
overwrites one encoded element of report 3 or of report 64 with p, p + 1 or
the all-ones pattern, and runs both aggregators through upload ->
prep_init -> decide_results -> aggregate.  The shapes cover both fields and
the three unpack paths (byte-wise rows, 8-byte-aligned rows, row tiles).
The honest oracle results are computed once per shape and shared.
"""
import functools
import random

import numpy as np
import pytest

from test_gpu_parity import CTX, _oracle_for, _random_agg_param, _random_reports, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

N = 65
STATUS_NONCANONICAL = -3

# name -> (constructor, args, level of the call)
SHAPES = {
    "sum5-bytewise": ("MasticSum", (5, 13), 2),                   # rows not 8-byte aligned: unpack_report<1>
    "sum32-aligned": ("MasticSum", (32, 255), 1),                 # unpack_report<8>
    "hist8-field128": ("MasticHistogram", (8, 4, 2), 3),          # Field128, one lane per report
    "sumvec32-rowtiles": ("MasticSumVec", (32, 64, 1, 8), 15),    # >= 16 KB per row: k_rows_to_planes
}
POSITIONS = ["cw0-first", "cw0-last", "cwL-first", "cwL-last", "cwdeep-first", "cwdeep-last", "lps-first",
             "lps-last"]


def _bad_values(field):
    p = field.MODULUS
    return [p, p + 1, (1 << (8 * field.ENCODED_SIZE)) - 1]


class _Shape:
    """Honest reports of one shape and the oracle's results for them."""

    def __init__(self, mastic_amd, name, levels=None):
        (cls, args, level) = SHAPES[name]
        self.m = m = getattr(mastic_amd, cls)(*args)
        self.o = o = _oracle_for(m)
        rng = random.Random(sum(map(ord, name)))
        (self.alphas, weights, self.nonces, rands) = _random_reports(m, rng, N)
        (self.pub, self.in0, self.in1) = m.shard_batch(CTX, self.alphas, weights, self.nonces, rands)
        self.vk = bytes(rng.getrandbits(8) for _ in range(32))
        self.level = level
        if levels is None:
            # prefixes of reports 3 and 64 among them, so the edited reports' out shares are not all zero shares
            cand = [self.alphas[3][:level + 1], self.alphas[64][:level + 1]]
            ap = _random_agg_param(m, rng, self.alphas[:1], level, 3, True)
            self.aps = [(level, tuple(dict.fromkeys(cand + list(ap[1])))[:3], True)]
        else:  # a sweep with no path pruned: every level extends the previous one's tree (frontier-cache hits)
            self.aps = [(lv, tuple(tuple(bool((k >> (lv - b)) & 1) for b in range(lv + 1)) for k in range(2 ** (lv + 1))),
                         lv == 0) for lv in levels]
        self.psz = m.public_share_size()
        self.isz = [m.input_share_size(0), m.input_share_size(1)]
        # oracle: [ap][agg] -> (list of prep share bytes, list of out share vectors)
        self.want = []
        for ap in self.aps:
            per = []
            for a in range(2):
                ins = self.in0 if a == 0 else self.in1
                shares, outs = [], []
                for i in range(N):
                    cws = o.vidpf.decode_public_share(self.pub[self.psz * i:self.psz * (i + 1)])
                    isd = o.decode_input_share(a, ins[self.isz[a] * i:self.isz[a] * (i + 1)])
                    (st, sh) = o.prep_init(self.vk, CTX, a, ap, self.nonces[16 * i:16 * (i + 1)], cws, isd)
                    shares.append(o.test_vec_encode_prep_share(sh))
                    outs.append(st[0])
                per.append((shares, outs))
            self.want.append(per)

    def offset(self, position):
        """(which buffer, byte offset within a report) of the element a position names."""
        o = self.o
        enc, vl = o.field.ENCODED_SIZE, o.vidpf.VALUE_LEN
        (where, which) = position.split("-")
        if where == "lps":
            e = 0 if which == "first" else o.flp.PROOF_LEN - 1
            return ("in0", 16 + e * enc)
        lv = {"cw0": 0, "cwL": self.aps[-1][0], "cwdeep": o.vidpf.BITS - 1}[where]
        assert where != "cwdeep" or lv > self.aps[-1][0]
        e = 0 if which == "first" else vl - 1
        nctrl = (2 * o.vidpf.BITS + 7) // 8
        return ("pub", nctrl + 16 * o.vidpf.BITS + (lv * vl + e) * enc)

    def edited(self, position, report, value):
        """(pub, in0) with one element of one report overwritten; checks that the
        oracle's decoder rejects exactly that share."""
        o = self.o
        enc = o.field.ENCODED_SIZE
        (buf, off) = self.offset(position)
        pub, in0 = bytearray(self.pub), bytearray(self.in0)
        if buf == "pub":
            at = self.psz * report + off
            pub[at:at + enc] = value.to_bytes(enc, "little")
            with pytest.raises(ValueError, match="out of range"):
                o.vidpf.decode_public_share(bytes(pub[self.psz * report:self.psz * (report + 1)]))
        else:
            at = self.isz[0] * report + off
            in0[at:at + enc] = value.to_bytes(enc, "little")
            with pytest.raises(ValueError, match="out of range"):
                o.decode_input_share(0, bytes(in0[self.isz[0] * report:self.isz[0] * (report + 1)]))
        return (bytes(pub), bytes(in0), buf)


@functools.lru_cache(maxsize=None)
def _shape(mastic_amd, name, levels=None):  # noqa: F811
    return _Shape(mastic_amd, name, levels)


@pytest.fixture(scope="module", autouse=True)
def _drop_shapes():
    yield
    _shape.cache_clear()  # the contexts go with the module, not at interpreter exit


def _check_level(s, dev, k, report, buf, expect_cached=None):
    """Both aggregators' prep_init of s.aps[k] over the uploaded (edited) batch."""
    (m, o) = (s.m, s.o)
    ap = s.aps[k]
    enc_ap = m.encode_agg_param(ap)
    for a in range(2):
        m.prep_init_device(dev, s.vk, CTX, a, enc_ap)
        if expect_cached is not None:
            assert m.last_prep_was_cached() == expect_cached, (ap[0], a)
    (acc, _codes) = m.decide_results(CTX, N)
    want_acc = [0 if i == report else 1 for i in range(N)]
    assert list(acc) == want_acc, "accept mask at level %d" % ap[0]
    p = o.field.MODULUS
    for a in range(2):
        (ps, _js, out, st) = m.prep_result(dev, a, enc_ap, want_out_shares=True)
        flagged = buf == "pub" or a == 0  # the leader proof share is in the leader's input only
        assert [i for i in range(N) if st[i] != 0] == ([report] if flagged else []), (ap[0], a, list(st))
        if flagged:
            assert st[report] == STATUS_NONCANONICAL
        (shares, outs) = s.want[k][a]
        pss, osz = len(ps) // N, len(out) // N
        total = o.field.zeros(len(outs[0]))
        for i in range(N):
            if i == report:
                continue
            assert ps[pss * i:pss * (i + 1)] == shares[i], "prep share %d agg %d level %d" % (i, a, ap[0])
            assert out[osz * i:osz * (i + 1)] == o.field.encode_vec(outs[i]), "out share %d agg %d" % (i, a)
            total = [x + y for (x, y) in zip(total, outs[i])]
        agg = m.aggregate_device(a, enc_ap, valid=acc, raw=True)
        assert agg == o.field.encode_vec(total), "agg share of agg %d at level %d" % (a, ap[0])
        esz = o.field.ENCODED_SIZE
        assert all(int.from_bytes(agg[j:j + esz], "little") < p for j in range(0, len(agg), esz))


@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_noncanonical_element_rejects_exactly_that_report(mastic_amd, name, position):  # noqa: F811
    s = _shape(mastic_amd, name)
    for report in (3, 64):
        for value in _bad_values(s.o.field):
            (pub, in0, buf) = s.edited(position, report, value)
            dev = s.m.reports_upload(s.nonces, pub, in0, s.in1)
            _check_level(s, dev, 0, report, buf)
    # the one-shot host-buffer entry point sees the same verdict
    (_ps, _js, _out, st) = s.m.prep_init_batch(s.vk, CTX, 0, s.aps[0], s.nonces, pub, in0)
    assert [i for i in range(N) if st[i] != 0] == [64] and st[64] == STATUS_NONCANONICAL


@pytest.mark.parametrize("position", POSITIONS)
def test_noncanonical_element_with_frontier_cache_walk(mastic_amd, position):  # noqa: F811
    """Mastic(32, Sum 255), levels 0 -> 1 -> 2 with the frontier cache on: a hit
    unpacks only one level of correction words, and the report must still be
    rejected at every level of the walk ("cwL" is the walk's last level)."""
    s = _shape(mastic_amd, "sum32-aligned", (0, 1, 2))
    s.m.set_frontier_cache(True)
    try:
        for report in (3, 64):
            for value in _bad_values(s.o.field):
                (pub, in0, buf) = s.edited(position, report, value)
                dev = s.m.reports_upload(s.nonces, pub, in0, s.in1)
                for k in range(len(s.aps)):
                    _check_level(s, dev, k, report, buf, expect_cached=(k > 0))
    finally:
        s.m.set_frontier_cache(False)


def test_view_sees_its_slice_of_the_verdicts(mastic_amd):  # noqa: F811
    """A view of reports 60..64 of a batch whose report 64 is bad flags its own
    report 4; a view of reports 0..9 flags nothing; a fresh upload of honest
    shares into the batch clears the verdict."""
    s = _shape(mastic_amd, "sum5-bytewise")
    (m, o) = (s.m, s.o)
    (pub, in0, _buf) = s.edited("cwdeep-last", 64, o.field.MODULUS)
    dev = m.reports_upload(s.nonces, pub, in0, s.in1)
    enc_ap = m.encode_agg_param(s.aps[0])
    for (first, count, bad) in [(60, 5, [4]), (0, 10, [])]:
        v = dev.view(first, count)
        for a in range(2):
            m.prep_init_device(v, s.vk, CTX, a, enc_ap)
            (ps, _js, _out, st) = m.prep_result(v, a, enc_ap)
            assert [i for i in range(count) if st[i] != 0] == bad
            pss = len(ps) // count
            for i in set(range(count)) - set(bad):
                assert ps[pss * i:pss * (i + 1)] == s.want[0][a][0][first + i]
    dev2 = m.reports_upload(s.nonces, s.pub, s.in0, s.in1)
    for a in range(2):
        m.prep_init_device(dev2, s.vk, CTX, a, enc_ap)
        assert not np.any(m.prep_result(dev2, a, enc_ap)[3])


def test_per_report_api_raises_the_reference_error(mastic_amd):  # noqa: F811
    """Mastic.prep_init (batch of one) raises the reference's ValueError text."""
    s = _shape(mastic_amd, "sum5-bytewise")
    (m, o) = (s.m, s.o)
    (pub, _in0, _buf) = s.edited("cwdeep-first", 3, o.field.MODULUS + 1)
    (_ps, _js, _out, st) = m.prep_init_batch(s.vk, CTX, 1, s.aps[0], s.nonces[48:64], pub[s.psz * 3:s.psz * 4],
                                             s.in1[s.isz[1] * 3:s.isz[1] * 4])
    assert list(st) == [STATUS_NONCANONICAL]
    from mastic_amd import vdaf
    assert vdaf.STATUS_NONCANONICAL == STATUS_NONCANONICAL
