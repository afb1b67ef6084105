"""The launch plan's small-tree corners on the GPU against the oracle, bit for
bit (csrc/schedule.hpp plan_chunk, executed by prep.hpp struct Chunk).

Trees of depth L = 0, 1, 2 and 3 -- no sponge before the final step at L = 0,
the first reuse of a level-buffer ring slot at L = 3, every level but the last
a split level -- for Count (Field64), and L = 3 for Histogram (Field128, which
runs the split-sponge schedule by default), each crossed with:

* the plain schedule;
* the last level forced into 3 parent ranges (clamped to the level's 1, 2, 3
  and 5 parents);
* the frontier cache on: a miss at L - 1, then the hit at L (L = 0: the miss);
* a memory budget of 192 reports' work buffers, under which a call runs as
  pipelined chunks of 64 reports.

70 reports (two report groups, the last one partial), except under the memory
budget: chunks are only pipelined when a call has more than 192 reports, so
that row runs 200 (four chunks, the last one of 8 reports), of which the 70
are the first.  The step count of mastic_last_timing3 tells how each call was
cut.  The oracle's results are computed once per (circuit, L) and shared.
tests/test_gpu_keccak_paths.py and tests/test_gpu_last_level_segments.py run
the same comparisons on deeper trees (L = 5 and 7).
"""
import random

import pytest

from test_gpu_parity import _oracle_for, _random_reports, mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

BITS = 8
N, N_CHUNKED = 70, 200
CTX = bytes((37 * i + 11) & 0xff for i in range(19))
CIRCUITS = {"Count": {}, "Histogram": dict(length=4, chunk_length=2)}
LEAVES = (0x03, 0x14, 0x37, 0x64, 0xC8, 0xFF)
CASES = [("Count", 0), ("Count", 1), ("Count", 2), ("Count", 3), ("Histogram", 3)]
N_PARENTS = {0: 1, 1: 2, 2: 3, 3: 5}  # of the last level


def _tree(L):
    """The leaves' (L + 1)-bit prefixes; the weight check only at level 0 (a hit has none)."""
    pfx = sorted({tuple(bool((v >> (7 - b)) & 1) for b in range(L + 1)) for v in LEAVES})
    return (L, tuple(pfx), L == 0)


_REF = {}


def _reference(mastic_amd, circuit, L, n):
    ref = _REF.get((circuit, L))
    if ref is None:
        m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
        rng = random.Random("small/%s/%d" % (circuit, L))
        (alphas, weights, nonces, rands) = _random_reports(m, rng, N_CHUNKED)
        vk = bytes(rng.getrandbits(8) for _ in range(16))
        (pub, in0, in1) = m.shard_batch(CTX, alphas, weights, nonces, rands)
        ref = _REF[(circuit, L)] = dict(vk=vk, nonces=nonces, pub=pub, ins=(in0, in1), want=[[], []])
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    o = _oracle_for(m)
    psz, isz = m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)]
    for i in range(len(ref["want"][0]), n):
        cws = o.vidpf.decode_public_share(ref["pub"][psz * i:psz * (i + 1)])
        for a in range(2):
            ish = o.decode_input_share(a, ref["ins"][a][isz[a] * i:isz[a] * (i + 1)])
            (ost, osh) = o.prep_init(ref["vk"], CTX, a, _tree(L), ref["nonces"][16 * i:16 * (i + 1)], cws, ish)
            ref["want"][a].append((o.test_vec_encode_prep_share(osh), o.field.encode_vec(ost[0])))
    return ref


def _equal(got, ref, a, n):
    (ps, _js, out, st) = got
    assert list(st) == [0] * n, "status, agg %d" % a
    want = ref["want"][a][:n]
    assert ps == b"".join(w[0] for w in want), "prep shares, agg %d" % a
    assert out == b"".join(w[1] for w in want), "out shares, agg %d" % a


def _batch(m, ref, L, a, n):
    psz, isz = m.public_share_size(), m.input_share_size(a)
    return m.prep_init_batch(ref["vk"], CTX, a, _tree(L), ref["nonces"][:16 * n], ref["pub"][:psz * n],
                             ref["ins"][a][:isz * n])


@pytest.mark.parametrize("circuit,L", CASES)
def test_plain(mastic_amd, circuit, L):
    ref = _reference(mastic_amd, circuit, L, N)
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    for a in range(2):
        _equal(_batch(m, ref, L, a, N), ref, a, N)
        assert m.last_timing3()[1] == L + 2  # levels 0..L and k_node_proof


@pytest.mark.parametrize("circuit,L", CASES)
def test_three_segments(mastic_amd, circuit, L):
    ref = _reference(mastic_amd, circuit, L, N)
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    m.set_last_level_segments(3)
    k = min(3, N_PARENTS[L])
    # one more launch and one timed payload piece per range; Field64 also times
    # level L-1's payload sponge on its own once it moves to the third stream
    # (a segmented level of a tree with L >= 2; Field128 runs that form anyway)
    early = 1 if (k > 1 and L >= 2 and circuit == "Count") else 0
    for a in range(2):
        _equal(_batch(m, ref, L, a, N), ref, a, N)
        assert m.last_timing3()[1] == (L + 2 if k == 1 else L + k + 1 + k + early)


@pytest.mark.parametrize("circuit,L", CASES)
def test_cache_miss_then_hit(mastic_amd, circuit, L):
    ref = _reference(mastic_amd, circuit, L, N)
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    psz, isz = m.public_share_size(), [m.input_share_size(0), m.input_share_size(1)]
    dev = m.reports_upload(ref["nonces"][:16 * N], ref["pub"][:psz * N], ref["ins"][0][:isz[0] * N],
                           ref["ins"][1][:isz[1] * N])
    m.set_frontier_cache(True)
    try:
        for a in range(2):
            if L > 0:
                (pl, ppfx, _wc) = _tree(L - 1)
                m.prep_init_device(dev, ref["vk"], CTX, a, (pl, ppfx, False))
                assert not m.last_prep_was_cached()
            m.prep_init_device(dev, ref["vk"], CTX, a, _tree(L))
            assert m.last_prep_was_cached() == (L > 0)
            _equal(m.prep_result(dev, a, _tree(L), want_out_shares=True), ref, a, N)
            # a hit: level L's kernel (proofs fused) and the final step; the miss at level 0 likewise
            assert m.last_timing3()[1] == 2
    finally:
        m.set_frontier_cache(False)


@pytest.mark.parametrize("circuit,L", CASES)
def test_pipelined_chunks(mastic_amd, circuit, L):
    ref = _reference(mastic_amd, circuit, L, N_CHUNKED)
    m = mastic_amd.Mastic(BITS, circuit, **CIRCUITS[circuit])
    m.set_memory_budget((192 + 64) * m.work_bytes(_tree(L)) + 1000)
    for a in range(2):
        _equal(_batch(m, ref, L, a, N_CHUNKED), ref, a, N_CHUNKED)
        assert m.last_timing3()[1] == 4 * (L + 2)  # chunks of 64, 64, 64 and 8 reports
