"""The Keccak paths of small chunks against the oracle, bit for bit.

A chunk below the one-lane sponge threshold runs the 2-lane binder sponges
(k_absorb_pair) and, beside them, the 104-VGPR level kernel (k_eval_aes_wide)
whose proof waves run the fused-theta permutation and load the proof
correction word after it.  Every case compares both aggregators' prep shares,
out shares and status of every report with ``oracle.mastic``:

* Count (Field64) and Histogram (Field128, the same proof waves), 65 and 130
  reports (a partial last report group, odd pair counts), on two trees: level
  7 with 6 scattered prefixes (most levels under one sponge block) and level 5
  with all 64 prefixes (64 to 128 nodes per level: many blocks per level, both
  sponge launches mid-block);
* ctx lengths 0, 1, 2, 3 and 19: the binder sponges start at byte 15 +
  len(ctx), so their fill position mod 4 takes all four values (the shifted
  absorb sends one word per lane pair and block word) and the block boundary
  falls at different words of the level messages;
* a ctx long enough that the node-proof body crosses the rate boundary (the
  two-permutation path of node_proof_one);
* the exact payload stream forced from block 0 (mastic_set_test_hooks).

The oracle's results are computed once per (circuit, tree, ctx) and shared:
the 65-report batch is the first half of the 130-report one.
"""
import random

import pytest

from test_gpu_parity import _oracle_for, _random_reports, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

BITS = 8
N_MAX = 130
CIRCUITS = {"Count": {}, "Histogram": dict(length=4, chunk_length=2)}
BENCH_CTX_LEN = 19


def _bits(v, n):
    return tuple(bool((v >> (n - 1 - b)) & 1) for b in range(n))


TREES = {
    # 6 prefixes scattered over the 256 leaves
    "level7_6pfx": (7, tuple(_bits(v, 8) for v in (3, 64, 65, 130, 201, 255)), True),
    # every 6-bit prefix
    "level5_all64": (5, tuple(_bits(v, 6) for v in range(64)), False),
}


def _ctx(n):
    return bytes((37 * i + 11) & 0xff for i in range(n))


def _node_proof_cross_ctx_len():
    """Smallest ctx whose node-proof prefix (le16(len(dst)) || dst ||
    u8(16), then the body: 16-byte seed, le16(BITS), le16(level), path)
    reaches the end of the 168-byte block: f + 20 + path_bytes >= 168."""
    from oracle.dst import USAGE_NODE_PROOF, dst
    path_bytes = (BITS + 7) // 8
    for n in range(400):
        f = (2 + len(dst(_ctx(n), USAGE_NODE_PROOF)) + 1) % 168
        if f + 20 + path_bytes >= 168:
            return n
    raise AssertionError("no crossing ctx length")


_REF = {}  # (circuit, tree, ctx_len) -> shards and the oracle's per-report results


def _reference(mastic_amd, circuit, tree, ctx_len, n):
    key = (circuit, tree, ctx_len)
    ref = _REF.get(key)
    if ref is None:
        m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
        rng = random.Random("%s/%s" % (circuit, tree))  # the same reports for every ctx
        (alphas, weights, nonces, rands) = _random_reports(m, rng, N_MAX)
        vk = bytes(rng.getrandbits(8) for _ in range(16))
        (pub, in0, in1) = m.shard_batch(_ctx(ctx_len), alphas, weights, nonces, rands)
        ref = _REF[key] = dict(vk=vk, nonces=nonces, pub=pub, ins=(in0, in1), want=[[], []])
        del m
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    o = _oracle_for(m)
    psz, isz = m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)]
    ap = TREES[tree]
    for i in range(len(ref["want"][0]), n):
        cws = o.vidpf.decode_public_share(ref["pub"][psz * i:psz * (i + 1)])
        for a in range(2):
            ish = o.decode_input_share(a, ref["ins"][a][isz[a] * i:isz[a] * (i + 1)])
            (ost, osh) = o.prep_init(ref["vk"], _ctx(ctx_len), a, ap, ref["nonces"][16 * i:16 * (i + 1)], cws, ish)
            ref["want"][a].append((o.test_vec_encode_prep_share(osh), o.field.encode_vec(ost[0])))
    return ref


def _check(mastic_amd, circuit, tree, ctx_len, n, force_slow_blk=-1):
    ref = _reference(mastic_amd, circuit, tree, ctx_len, n)
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    if force_slow_blk >= 0:
        m.set_test_hooks(force_slow_blk=force_slow_blk)
    psz, isz = m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)]
    ap = TREES[tree]
    for a in range(2):
        (ps, _js, out, st) = m.prep_init_batch(ref["vk"], _ctx(ctx_len), a, ap, ref["nonces"][:16 * n],
                                               ref["pub"][:psz * n], ref["ins"][a][:isz[a] * n])
        assert list(st) == [0] * n, "status, agg %d" % a
        want = ref["want"][a][:n]
        assert ps == b"".join(w[0] for w in want), "prep shares, agg %d" % a
        assert out == b"".join(w[1] for w in want), "out shares, agg %d" % a


@pytest.mark.parametrize("n", [65, N_MAX])
@pytest.mark.parametrize("tree", sorted(TREES))
@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_circuits_trees_and_report_counts(mastic_amd, circuit, tree, n):
    _check(mastic_amd, circuit, tree, BENCH_CTX_LEN, n)


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
@pytest.mark.parametrize("ctx_len", [0, 1, 2, 3, BENCH_CTX_LEN], ids=lambda n: "ctx%d_fill%d" % (n, (15 + n) % 4))
def test_shifted_absorb_fill_positions(mastic_amd, ctx_len, circuit):
    _check(mastic_amd, circuit, "level5_all64", ctx_len, 65)


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_node_proof_crossing_the_rate_boundary(mastic_amd, circuit):
    from oracle.dst import USAGE_NODE_PROOF, dst
    n = _node_proof_cross_ctx_len()
    f = (2 + len(dst(_ctx(n), USAGE_NODE_PROOF)) + 1) % 168
    assert f < 168 <= f + 20 + (BITS + 7) // 8
    _check(mastic_amd, circuit, "level7_6pfx", n, 65)


@pytest.mark.parametrize("circuit,tree", [("Count", "level5_all64"), ("Histogram", "level7_6pfx")])
def test_exact_payload_stream_from_block_0(mastic_amd, circuit, tree):
    _check(mastic_amd, circuit, tree, BENCH_CTX_LEN, 65, force_slow_blk=0)
