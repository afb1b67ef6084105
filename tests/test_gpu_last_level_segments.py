"""The segmented last level (Mastic.set_last_level_segments) against the
oracle, bit for bit.

A prep_init with no frontier cache that runs as one stream of chunks beside
the 2-lane sponges may evaluate its last level in K parent ranges: one level-
kernel launch per range, the node proofs of a range computed by the next
launch's proof waves (k_node_proof keeps the last range's), and both binder
sponges absorbing the level's messages piece by piece.  Every case compares
both aggregators' prep shares, out shares and status of every report with
``oracle.mastic``, on the shapes of tests/test_gpu_keccak_paths.py (whose
references are shared: computed once per (circuit, tree, ctx)):

* Count (Field64) and Histogram (Field128, which runs the split sponge
  schedule anyway), 65 and 130 reports, the trees level5_all64 (32 last-level
  parents) and level7_6pfx (6), forced K = 1, 2, 3, 5 and 32: 3 and 5 give
  uneven ranges, 32 one parent per range (64-byte one-hot pieces, well under
  a 168-byte sponge block) and clamps to 6 on the small tree;
* ctx lengths 0, 1, 2, 3 and 19 at K = 3: the sponges' fill position mod 4
  takes all four values at the piece boundaries;
* a tree with a single last-level parent (K clamps to 1);
* the exact payload stream forced from block 0 at K = 3;
* a memory budget that splits the batch into chunks, K = 3 forced;
* the measurement schedule (every sponge piece alone) at K = 3;
* auto (k = 0), which keeps one launch on levels this small.
"""
import ctypes
import random

import pytest

from test_gpu_keccak_paths import BENCH_CTX_LEN, BITS, CIRCUITS, TREES, _bits, _ctx, _reference
from test_gpu_parity import _oracle_for, _random_reports, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu


def _run(m, ref, ap, ctx_len, n):
    """Both aggregators' (prep shares, out shares) of the first n reports,
    checked against the oracle's."""
    psz, isz = m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)]
    got = []
    for a in range(2):
        (ps, _js, out, st) = m.prep_init_batch(ref["vk"], _ctx(ctx_len), a, ap, ref["nonces"][:16 * n],
                                               ref["pub"][:psz * n], ref["ins"][a][:isz[a] * n])
        assert list(st) == [0] * n, "status, agg %d" % a
        want = ref["want"][a][:n]
        assert ps == b"".join(w[0] for w in want), "prep shares, agg %d" % a
        assert out == b"".join(w[1] for w in want), "out shares, agg %d" % a
        got.append((ps, out))
    return got


def _check(mastic_amd, circuit, tree, ctx_len, n, k, setup=None):
    ref = _reference(mastic_amd, circuit, tree, ctx_len, n)
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    assert m.set_last_level_segments(k) == 0  # the default is auto
    assert m.set_last_level_segments(k) == k
    if setup:
        setup(m)
    return _run(m, ref, TREES[tree], ctx_len, n)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 32])
@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("tree", sorted(TREES))
@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_forced_segments(mastic_amd, circuit, tree, n, k):
    _check(mastic_amd, circuit, tree, BENCH_CTX_LEN, n, k)


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
@pytest.mark.parametrize("ctx_len", [0, 1, 2, 3, BENCH_CTX_LEN], ids=lambda n: "ctx%d_fill%d" % (n, (15 + n) % 4))
def test_fill_positions_at_piece_boundaries(mastic_amd, ctx_len, circuit):
    _check(mastic_amd, circuit, "level5_all64", ctx_len, 65, 3)


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_single_last_level_parent(mastic_amd, circuit):
    """One prefix at level 3: one parent per level, so K = 3 clamps to 1."""
    n = 65
    ap = (3, (_bits(11, 4),), True)
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    o = _oracle_for(m)
    rng = random.Random("single/%s" % circuit)
    (alphas, weights, nonces, rands) = _random_reports(m, rng, n)
    vk = bytes(rng.getrandbits(8) for _ in range(16))
    ctx = _ctx(BENCH_CTX_LEN)
    (pub, in0, in1) = m.shard_batch(ctx, alphas, weights, nonces, rands)
    psz, isz = m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)]
    m.set_last_level_segments(3)
    for (a, ins) in enumerate((in0, in1)):
        (ps, _js, out, st) = m.prep_init_batch(vk, ctx, a, ap, nonces, pub, ins)
        assert list(st) == [0] * n
        want_ps, want_out = [], []
        for i in range(n):
            cws = o.vidpf.decode_public_share(pub[psz * i:psz * (i + 1)])
            ish = o.decode_input_share(a, ins[isz[a] * i:isz[a] * (i + 1)])
            (ost, osh) = o.prep_init(vk, ctx, a, ap, nonces[16 * i:16 * (i + 1)], cws, ish)
            want_ps.append(o.test_vec_encode_prep_share(osh))
            want_out.append(o.field.encode_vec(ost[0]))
        assert ps == b"".join(want_ps), "prep shares, agg %d" % a
        assert out == b"".join(want_out), "out shares, agg %d" % a


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_exact_payload_stream_from_block_0(mastic_amd, circuit):
    _check(mastic_amd, circuit, "level5_all64", BENCH_CTX_LEN, 65, 3,
           setup=lambda m: m.set_test_hooks(force_slow_blk=0))


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_memory_budget_chunks(mastic_amd, circuit):
    """130 reports under a budget of 128 reports' work buffers: at least two
    chunks, one after the other on the main stream, with K = 3 forced."""
    from mastic_amd import _lib
    ms = []

    def budget(m):
        enc = m.encode_agg_param(TREES["level5_all64"])
        per = ctypes.c_uint64()
        assert _lib.lib().mastic_work_bytes(m._ctx, enc, len(enc), ctypes.byref(per)) == 0
        m.set_memory_budget((64 + 64) * per.value + 1000)
        ms.append(m)

    _check(mastic_amd, circuit, "level5_all64", BENCH_CTX_LEN, 130, 3, setup=budget)
    # every chunk launches each of the 6 levels and k_node_proof at least once
    assert ms[0].last_timing3()[1] >= 2 * (6 + 1)


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_serial_sponges(mastic_amd, circuit):
    """Every sponge piece running alone (the measurement schedule) gives the
    same results, and the timing marks of every launch and piece resolve."""
    m_ref = []

    def serial(m):
        m.set_serial_sponges(True)
        m_ref.append(m)

    got = _check(mastic_amd, circuit, "level5_all64", BENCH_CTX_LEN, 65, 3, setup=serial)
    (aes_ms, n_aes, proof_ms, _np, absorb_ms, _nb, total_ms) = m_ref[0].last_timing3()
    # levels 0..5, two more launches for level 5's ranges, k_node_proof, and the
    # payload pieces' own marks: level 4's (Field64 only, moved to the third
    # stream) and the three ranges'
    assert n_aes == 6 + 2 + 1 + 3 + (1 if circuit == "Count" else 0)
    assert aes_ms > 0 and proof_ms > 0 and absorb_ms > 0 and total_ms >= aes_ms
    assert got == _check(mastic_amd, circuit, "level5_all64", BENCH_CTX_LEN, 65, 3)


@pytest.mark.parametrize("tree", sorted(TREES))
@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
def test_auto_keeps_one_launch_on_small_levels(mastic_amd, circuit, tree):
    """k = 0: a level that cannot fill the device twice per range is not
    segmented -- as many launches as with K = 1, and the same results."""
    ref = _reference(mastic_amd, circuit, tree, BENCH_CTX_LEN, 65)
    runs = []
    for k in (0, 1):
        m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
        m.set_last_level_segments(k)
        got = _run(m, ref, TREES[tree], BENCH_CTX_LEN, 65)
        runs.append((got, m.last_timing3()[1]))
    assert runs[0] == runs[1]
    assert runs[0][1] == TREES[tree][0] + 2  # levels 0..L and k_node_proof
