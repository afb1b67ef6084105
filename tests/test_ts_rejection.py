"""Rejection sampling in the TurboSHAKE next_vec sampler on real data
(sponge_squeeze_vec, keccak.hpp: query rand, helper proof share and joint rand
in k_flp_rand; prove rand and helper proof share in k_shard).  For Field64 a
candidate >= p turns up once per 2^32 elements, which no reference vector and
no random test reaches; tests/golden/ts_rejection_f64.json
(tests/rejection/make_ts_fixture.py) holds brute-forced inputs that do:

  query_rand             a nonce; MasticSum(4, 1023), QUERY_RAND_LEN 22
  query_rand_full_block  a nonce; MasticSum(4, 2^20 - 1), QUERY_RAND_LEN 42 =
                         exactly two 168-byte squeeze blocks, so the rejected
                         candidate costs that one lane a third permutation
                         (a Sum circuit's 2 * bits + 2 query-rand elements are
                         never 21; 42 is the first multiple)
  proof_share            a helper seed; PROOF_LEN 64
  prove_rand             a prove-rand seed; PROVE_RAND_LEN 1

The fixture holds only the search results; every expected output is
recomputed by the oracle here.  GPU batches have 65 reports with the found
nonce or seed in report 3 only: wave 0 has one lane that consumes one
candidate more than the rest, wave 1 has none.

A real Field128 rejection (probability 2^-59 per candidate) cannot be found by
search; tests/test_gpu_xof_ops.py (part C) runs sponge_squeeze_vec from chosen
sponge states instead, whose first block holds rejected candidates at every
position for both fields.
"""
import functools
import json
import os
import random

import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "ts_rejection_f64.json")
FINDINGS = ["query_rand", "query_rand_full_block", "proof_share", "prove_rand"]
N = 65
AT = 3


@functools.lru_cache(maxsize=None)
def _fx():
    return json.load(open(FIXTURE))


def _oracle(f):
    from oracle import mastic as om
    return om.MasticSum(_fx()["bits"], f["max_measurement"])


def _stream(o, f):
    """(xof arguments, number of elements next_vec is asked for) of a finding's stream."""
    from oracle.common import to_le_bytes
    from oracle.dst import USAGE_PROOF_SHARE, USAGE_PROVE_RAND, USAGE_QUERY_RAND, dst_alg
    fx = _fx()
    ctx = bytes.fromhex(fx["ctx"])
    if f["stream"] == "query_rand":
        return ((bytes.fromhex(fx["verify_key"]), dst_alg(ctx, USAGE_QUERY_RAND, o.ID),
                 bytes.fromhex(f["nonce"]) + to_le_bytes(fx["level"], 2)), o.flp.QUERY_RAND_LEN)
    if f["stream"] == "proof_share":
        return ((bytes.fromhex(f["helper_seed"]), dst_alg(ctx, USAGE_PROOF_SHARE, o.ID), b""), o.flp.PROOF_LEN)
    return ((bytes.fromhex(f["prove_rand_seed"]), dst_alg(ctx, USAGE_PROVE_RAND, o.ID), b""), o.flp.PROVE_RAND_LEN)


def test_fixture_is_complete():
    fx = _fx()
    assert sorted(fx["findings"]) == sorted(FINDINGS)
    o = _oracle(fx["findings"]["query_rand"])
    assert (o.flp.QUERY_RAND_LEN, o.flp.PROOF_LEN, o.flp.PROVE_RAND_LEN) == (22, 64, 1)
    o2 = _oracle(fx["findings"]["query_rand_full_block"])
    assert o2.flp.QUERY_RAND_LEN == 42 and 42 * 8 == 2 * 168, "exactly two squeeze blocks"


@pytest.mark.parametrize("name", FINDINGS)
def test_oracle_reproduces_the_stream_and_next_vec_skips_the_candidate(name):
    f = _fx()["findings"][name]
    o = _oracle(f)
    (args, count) = _stream(o, f)
    p = o.field.MODULUS
    xof = o.xof(*args)
    raw = [int.from_bytes(xof.next(8), "little") for _ in range(count + 2)]
    c = f["candidate"]
    assert c < count, "the rejected candidate is one next_vec reads"
    assert raw[c] >= p and raw[c] >> 32 == 0xFFFFFFFF
    assert all(x < p for x in raw[:c]), "the recorded candidate is the first one rejected"
    got = [x.int() for x in o.xof.expand_into_vec(o.field, *args, count)]
    assert got == [x for x in raw if x < p][:count]
    assert got != raw[:count] and got[c:] == [x for x in raw[c + 1:] if x < p][:count - c]
    # and the stream is the one the protocol uses for this report
    if f["stream"] == "query_rand":
        fx = _fx()
        want = o.query_rand(bytes.fromhex(fx["verify_key"]), bytes.fromhex(fx["ctx"]), bytes.fromhex(f["nonce"]),
                            fx["level"])
    elif f["stream"] == "proof_share":
        want = o.helper_proof_share(bytes.fromhex(_fx()["ctx"]), bytes.fromhex(f["helper_seed"]))
    else:
        want = o.prove_rand(bytes.fromhex(_fx()["ctx"]), bytes.fromhex(f["prove_rand_seed"]))
    assert [x.int() for x in want] == got


@pytest.mark.gpu
@pytest.mark.parametrize("name", FINDINGS)
def test_gpu_matches_oracle_with_one_rejecting_lane(name):
    import mastic_amd
    fx = _fx()
    f = fx["findings"][name]
    o = _oracle(f)
    m = mastic_amd.MasticSum(fx["bits"], f["max_measurement"])
    (ctx, vk, level) = (bytes.fromhex(fx["ctx"]), bytes.fromhex(fx["verify_key"]), fx["level"])
    rng = random.Random(sum(map(ord, name)))
    alphas = [tuple(bool(rng.getrandbits(1)) for _ in range(m.BITS)) for _ in range(N)]
    weights = [rng.randrange(f["max_measurement"] + 1) for _ in range(N)]
    nonces = bytearray(rng.randbytes(16 * N))
    rands = bytearray(rng.randbytes(m.RAND_SIZE * N))
    assert m.RAND_SIZE == o.RAND_SIZE == o.vidpf.RAND_SIZE + 64  # vidpf rand || prove-rand seed || helper seed
    if f["stream"] == "query_rand":
        nonces[16 * AT:16 * (AT + 1)] = bytes.fromhex(f["nonce"])
    elif f["stream"] == "proof_share":
        at = m.RAND_SIZE * AT + o.vidpf.RAND_SIZE + 32
        rands[at:at + 32] = bytes.fromhex(f["helper_seed"])
    else:
        at = m.RAND_SIZE * AT + o.vidpf.RAND_SIZE
        rands[at:at + 32] = bytes.fromhex(f["prove_rand_seed"])
    (nonces, rands) = (bytes(nonces), bytes(rands))
    (pub, in0, in1) = m.shard_batch(ctx, alphas, weights, nonces, rands)
    psz, isz = m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)]
    ins = [in0, in1]
    # k_shard's copy of the sampler: the client's shares of the report with the found seed (and two others)
    for i in (0, AT, N - 1):
        (cws, oins) = o.shard(ctx, (alphas[i], weights[i]), nonces[16 * i:16 * (i + 1)],
                              rands[m.RAND_SIZE * i:m.RAND_SIZE * (i + 1)])
        assert pub[psz * i:psz * (i + 1)] == o.test_vec_encode_public_share(cws), i
        for a in range(2):
            assert ins[a][isz[a] * i:isz[a] * (i + 1)] == o.test_vec_encode_input_share(oins[a]), (i, a)
    prefixes = tuple(dict.fromkeys([alphas[0][:level + 1], alphas[AT][:level + 1], alphas[N - 1][:level + 1]]))
    ap = (level, prefixes, True)
    shares = []
    for a in range(2):
        (ps, _js, out, st) = m.prep_init_batch(vk, ctx, a, ap, nonces, pub, ins[a])
        assert list(st) == [0] * N
        pss, osz = len(ps) // N, len(out) // N
        for i in (0, AT, N - 1):
            cws = o.vidpf.decode_public_share(pub[psz * i:psz * (i + 1)])
            isd = o.decode_input_share(a, ins[a][isz[a] * i:isz[a] * (i + 1)])
            (ost, osh) = o.prep_init(vk, ctx, a, ap, nonces[16 * i:16 * (i + 1)], cws, isd)
            assert ps[pss * i:pss * (i + 1)] == o.test_vec_encode_prep_share(osh), "prep share %d agg %d" % (i, a)
            assert out[osz * i:osz * (i + 1)] == o.field.encode_vec(ost[0]), "out share %d agg %d" % (i, a)
        shares.append(ps)
    (_msgs, valid) = m.decide_batch(ctx, ap, shares[0], shares[1])
    assert list(valid) == [1] * N
