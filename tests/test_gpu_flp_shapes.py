"""The C ABI over the FLP shape grid of tests/flp_grid.py and over dishonest
clients.  The other GPU suites run the FLP kernels (k_shard's prove,
k_flp_rand, k_flp_query, k_decide) at a handful of small parameter sets; the
grid reaches P = 2 with ParallelSum, weights of 63 bits, truncation groups
wider than 32 bits, query and joint randomness beyond the first TurboSHAKE
block, chunk lengths larger than the measurement and call counts on either
side of a power of two.  Everything is compared with the CPU oracle bit for
bit, and the aggregates with the plaintext sums.
"""
import random

import pytest

import flp_grid as G
from test_gpu_configs import _plaintext
from test_gpu_parity import CTX, _check_against_oracle, _oracle_for, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

BITS = 3


def _mastic(mastic_amd, shape):  # noqa: F811
    (circuit, kw) = shape
    m = mastic_amd.Mastic(BITS, circuit, **kw)
    # a new work arena is min(48 GiB, budget): 1.4 to 2.9 s of hipMalloc per
    # context at the default, for batches here that need a few megabytes
    m.set_memory_budget(1 << 30)
    return m


def _alpha(rng):
    return tuple(bool(rng.getrandbits(1)) for _ in range(BITS))


def _pack_alphas(alphas):
    return bytes(sum(int(b) << (7 - i) for (i, b) in enumerate(a)) for a in alphas)


def _unique(xs):
    return tuple(dict.fromkeys(xs))


def _grid_reports(shape, rng):
    """Three reports: the two boundary measurements and a random one."""
    (circuit, kw) = shape
    bm = G.boundary_measurements(shape)
    (lo, hi) = (bm[0], bm[min(1, len(bm) - 1)])
    width = {"Sum": kw.get("max_measurement", 0).bit_length(), "SumVec": kw.get("sum_vec_bits", 0)}.get(circuit, 0)
    alphas = [_alpha(rng) for _ in range(3)]
    if width >= 62:
        # the maximum in one report only and the others below 2^61, under
        # another first bit: every prefix total stays below Field64's p
        third = rng.randrange(2 ** 61) if circuit == "Sum" else [rng.randrange(2 ** 61) for _ in range(kw["length"])]
        alphas[1] = (not alphas[0][0],) + alphas[1][1:]
    else:
        third = G.random_measurement(shape, rng)
        alphas[1] = alphas[0]  # one prefix aggregates two reports
    return (alphas, [hi, lo, third])


def _check_aggregates(m, o, ap, gpu, alphas, weights, valid=None):
    """aggregate_device of both aggregators equals the oracle's agg_update
    chain over the (oracle-checked) out shares, and unshard the plaintext."""
    n = len(alphas)
    keep = [i for i in range(n) if valid is None or valid[i]]
    aggs = []
    for a in range(2):
        agg = m.aggregate_device(a, ap, valid=valid)
        out = gpu[a][2]
        ow = len(out) // n
        want = o.agg_init(ap)
        for r in keep:
            want = o.agg_update(ap, want, o.field.decode_vec(out[ow * r:ow * (r + 1)]))
        assert m.field.encode_vec(agg) == o.field.encode_vec(want), "agg %d level %d" % (a, ap[0])
        aggs.append(agg)
    assert m.unshard(ap, aggs, len(keep)) == _plaintext(m, [alphas[i] for i in keep], [weights[i] for i in keep], ap[1])


@pytest.mark.parametrize("shape", G.GRID, ids=G.shape_id)
def test_grid_shape_matches_oracle(mastic_amd, shape):  # noqa: F811
    rng = random.Random("gpu flp shapes " + G.shape_id(shape))
    m = _mastic(mastic_amd, shape)
    o = _oracle_for(m)
    (alphas, weights) = _grid_reports(shape, rng)
    n = len(alphas)
    nonces = bytes(rng.getrandbits(8) for _ in range(16 * n))
    rands = bytes(rng.getrandbits(8) for _ in range(m.RAND_SIZE * n))
    vk = bytes(rng.getrandbits(8) for _ in range(32))
    params = [(0, ((False,), (True,)), True),
              (2, _unique(alphas), True),
              (1, _unique(a[:2] for a in alphas), False)]
    for ap in params:
        gpu = _check_against_oracle(m, o, CTX, vk, ap, alphas, weights, nonces, rands, check_shard=(ap[0] == 0))
        _check_aggregates(m, o, ap, gpu, alphas, weights)


BEYOND_ONE_WAVE = [("Sum", dict(max_measurement=2047)),
                   ("MultihotCountVec", dict(length=9, max_measurement=4, chunk_length=2))]


@pytest.mark.parametrize("shape", BEYOND_ONE_WAVE, ids=G.shape_id)
def test_sharded_bytes_beyond_the_first_wave(mastic_amd, shape):  # noqa: F811
    """65 reports: k_shard's second wave and a partly filled stride, every
    report's public share and input shares against the oracle's."""
    assert shape in G.GRID
    rng = random.Random("gpu flp shapes 65 " + G.shape_id(shape))
    m = _mastic(mastic_amd, shape)
    o = _oracle_for(m)
    n = 65
    alphas = [_alpha(rng) for _ in range(n)]
    weights = G.boundary_measurements(shape)[:2] + [G.random_measurement(shape, rng) for _ in range(n - 2)]
    nonces = bytes(rng.getrandbits(8) for _ in range(16 * n))
    rands = bytes(rng.getrandbits(8) for _ in range(m.RAND_SIZE * n))
    ap = (0, ((False,), (True,)), True)
    _check_against_oracle(m, o, CTX, bytes(range(32)), ap, alphas, weights, nonces, rands, check_shard=True)


# one shape per circuit, none of them among test_gpu_parity.CASES
DISHONEST = [
    ("Count", dict()),
    ("Sum", dict(max_measurement=4)),
    ("SumVec", dict(length=2, sum_vec_bits=33, chunk_length=5)),
    ("Histogram", dict(length=33, chunk_length=3)),
    ("MultihotCountVec", dict(length=9, max_measurement=4, chunk_length=2)),
]


@pytest.mark.parametrize("shape", DISHONEST, ids=G.shape_id)
def test_dishonest_clients_rejected_end_to_end(mastic_amd, shape):  # noqa: F811
    """Dishonest encodings sharded by the GPU client (shard_encoded) beside
    two honest controls: the sharded bytes and both prep shares equal the
    oracle's on the same encodings, decide_batch gives code 2 for exactly the
    dishonest reports, as the oracle's prep_shares_to_prep does, and the
    aggregate over the accepted reports is the plaintext of the honest ones."""
    rng = random.Random("gpu flp shapes dishonest " + G.shape_id(shape))
    m = _mastic(mastic_amd, shape)
    o = _oracle_for(m)
    F = o.field
    controls = G.boundary_measurements(shape)[:2]
    encs = [enc for (_name, enc) in G.dishonest_encodings(shape)]
    honest = [False] * len(encs) + [True] * len(controls)
    encs += [G.encode(shape, w) for w in controls]
    weights = [None] * (len(encs) - len(controls)) + controls
    n = len(encs)
    alphas = [_alpha(rng) for _ in range(n)]
    nonces = bytes(rng.getrandbits(8) for _ in range(16 * n))
    rands = bytes(rng.getrandbits(8) for _ in range(m.RAND_SIZE * n))
    vk = bytes(rng.getrandbits(8) for _ in range(32))
    betas = b"".join(F.encode_vec([F(x) for x in enc]) for enc in encs)
    (pub, in0, in1) = m.shard_encoded(CTX, n, _pack_alphas(alphas), betas, nonces, rands)
    ap = (0, ((False,), (True,)), True)
    gpu = [m.prep_init_batch(vk, CTX, a, ap, nonces, pub, in0 if a == 0 else in1) for a in range(2)]
    (_msgs, codes) = m.decide_batch(CTX, ap, gpu[0][0], gpu[1][0])

    (psz, isz, pss) = (m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)], m.prep_share_size(True))
    for i in range(n):
        nonce = nonces[16 * i:16 * (i + 1)]
        # the oracle shards a pre-encoded measurement while its encode is the identity
        o.flp.encode = lambda encoded: encoded
        try:
            (cws, ins) = o.shard(CTX, (alphas[i], [F(x) for x in encs[i]]), nonce,
                                 rands[m.RAND_SIZE * i:m.RAND_SIZE * (i + 1)])
        finally:
            del o.flp.encode
        assert o.test_vec_encode_public_share(cws) == pub[psz * i:psz * (i + 1)], "report %d" % i
        assert o.test_vec_encode_input_share(ins[0]) == in0[isz[0] * i:isz[0] * (i + 1)], "report %d" % i
        assert o.test_vec_encode_input_share(ins[1]) == in1[isz[1] * i:isz[1] * (i + 1)], "report %d" % i
        shares = []
        for a in range(2):
            assert gpu[a][3][i] == 0
            (_st, sh) = o.prep_init(vk, CTX, a, ap, nonce, cws, ins[a])
            assert gpu[a][0][pss * i:pss * (i + 1)] == o.test_vec_encode_prep_share(sh), "report %d agg %d" % (i, a)
            shares.append(sh)
        try:
            o.prep_shares_to_prep(CTX, ap, shares)
            accepted = True
        except Exception as e:
            assert str(e) == "FLP verification failed"
            accepted = False
        assert accepted == honest[i], "report %d: oracle verdict" % i
        assert codes[i] == (1 if honest[i] else 2), "report %d: decide code %d" % (i, codes[i])
    _check_aggregates(m, o, ap, gpu, alphas, weights, valid=[int(h) for h in honest])
