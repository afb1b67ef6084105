"""tests/xof_ref.py is pinned before tests/test_gpu_xof_ops.py trusts it: its
sponge against oracle._prims.turboshake128, its next_vec against
oracle.xof.XofTurboShake128.next_vec, both fields.  Then every case list of
tests/xof_cases.py is held to its intended class: the reference rejects
exactly the candidates a squeeze case plans (counted per lane), every edge
class named for the sponge, node-proof and absorb grids is non-empty (the
census, printed), and no case is dropped: the counts are asserted."""
import random

import numpy as np
import pytest

import xof_cases as XC
import xof_ref as R
from oracle import _prims
from oracle.field import Field64, Field128
from oracle.xof import XofTurboShake128

MSG_LENS = [0, 1, 167, 168, 169, 335, 336, 337, 1000]
OUT_LENS = [16, 32, 168, 169, 400]


def test_round_constants_and_offsets_are_the_specifications():
    # FIPS 202 section 3.2.5 (last twelve of Keccak-f's) and table 2
    assert R.RC12[0] == 0x000000008000808B and R.RC12[-1] == 0x8000000080008008 and len(R.RC12) == 12
    assert R.RHO[1] == 1 and R.RHO[2] == 62 and R.RHO[5] == 36 and R.RHO[24] == 14 and sorted(R.RHO)[:2] == [0, 1]


@pytest.mark.parametrize("domain", [1, 2])
def test_sponge_equals_turboshake128(domain):
    rng = random.Random(domain)
    for n in MSG_LENS:
        msg = bytes(rng.randrange(256) for _ in range(n))
        for out_len in OUT_LENS:
            assert R.turboshake128(msg, domain, out_len) == _prims.turboshake128(msg, domain, out_len), (n, out_len)


def test_absorb_in_pieces_and_per_lane_positions():
    """absorb with per-lane f and nbytes equals lane-by-lane absorption, and
    continuing at the returned f equals absorbing the concatenation"""
    rng = np.random.default_rng(5)
    n = 40
    st = rng.integers(0, 2 ** 64, size=(n, 25), dtype=np.uint64)
    f = rng.integers(0, 168, size=n)
    nb = rng.integers(0, 400, size=n)
    data = rng.integers(0, 256, size=(n, 400), dtype=np.uint8)
    (got, gf) = R.absorb(st, f, data, nb)
    for i in range(n):
        (one, of) = R.absorb(st[i:i + 1], int(f[i]), data[i:i + 1, :nb[i]])
        assert np.array_equal(one[0], got[i]) and of[0] == gf[i]
        cut = int(nb[i]) // 3
        (a, af) = R.absorb(st[i:i + 1], int(f[i]), data[i:i + 1, :cut])
        (b, bf) = R.absorb(a, int(af[0]), data[i:i + 1, cut:nb[i]])
        assert np.array_equal(b[0], got[i]) and bf[0] == gf[i]


@pytest.mark.parametrize("field", [Field64, Field128])
def test_next_vec_equals_the_oracle(field):
    rng = random.Random(field.ENCODED_SIZE)
    for trial in range(20):
        seed = bytes(rng.randrange(256) for _ in range(32))
        dst = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40)))
        binder = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 200)))
        count = rng.choice([1, 10, 21, 22, 43, 100])
        want = [x.val for x in XofTurboShake128(seed, dst, binder).next_vec(field, count)]
        msg = len(dst).to_bytes(2, "little") + dst + bytes([len(seed)]) + seed + binder
        (st, f) = R.absorb(np.zeros((1, 25), np.uint64), 0, np.frombuffer(msg, np.uint8).reshape(1, -1))
        ((got, rejected),) = R.next_vec_from_states(R.pad(st, f, 1), field.MODULUS, field.ENCODED_SIZE, count)
        assert got == want and rejected == []


def test_next_vec_rejects_on_a_byte_stream():
    p = XC.F64_P
    stream = b"".join(v.to_bytes(8, "little") for v in [p, 5, p - 1, 2 ** 64 - 1, p + 1, 7, 9])
    assert R.next_vec(stream, p, 8, 3) == ([5, p - 1, 7], [0, 3, 4])
    with pytest.raises(IndexError):
        R.next_vec(stream, p, 8, 5)


@pytest.mark.parametrize("bits", [64, 128])
def test_squeeze_cases_reject_what_they_plan(bits):
    (p, enc, k) = XC.FIELDS[bits]
    assert (p == Field64.MODULUS) if bits == 64 else (p == Field128.MODULUS)
    cases = XC.squeeze_cases(bits)
    st = XC.squeeze_states(bits, cases)
    census = XC.squeeze_census(bits, cases)
    print("squeeze census, Field%d: %s" % (bits, census))
    assert len(cases) >= XC.LANES and len(cases) > 64
    assert all(v > 0 for v in census.values()), census
    for count in XC.squeeze_counts(bits):
        res = R.next_vec_from_states(st, p, enc, count)
        per_count = {"0": 0, "1": 0, "many": 0}
        for (c, (vals, rejected)) in zip(cases, res):
            plan = c.planned_rejections(count, k)
            assert len(vals) == count and all(v < p for v in vals)
            # exactly the planned candidates, and none by chance in the later blocks
            assert rejected == sorted(c.plan)[:plan], (bits, count, c.name, rejected)
            per_count["0" if plan == 0 else "1" if plan == 1 else "many"] += 1
        print("  count %d: lanes with 0 / 1 / many rejections: %s" % (count, per_count))
        assert all(v > 0 for v in per_count.values()), (count, per_count)


def test_squeeze_cases_first_k_rejected_cost_what_they_should():
    """a whole rejected block costs the lane a further permutation: its values come from block 1"""
    for bits in (64, 128):
        (p, enc, k) = XC.FIELDS[bits]
        cases = XC.squeeze_cases(bits)
        st = XC.squeeze_states(bits, cases)
        i = [c.name for c in cases].index("first %d rejected" % k)
        ((vals, rejected),) = R.next_vec_from_states(st[i:i + 1], p, enc, 1)
        assert rejected == list(range(k))
        nxt = R.squeeze(st[i:i + 1], 336)[0].tobytes()
        if bits == 64:
            assert vals == [int.from_bytes(nxt[168:176], "little")]
        else:  # candidate 10 straddles words 40, 41 of block 0 and 0, 1 of block 1
            assert vals == [int.from_bytes(nxt[160:176], "little")]


def test_sponge_grid_census():
    cfgs = XC.sponge_cfgs()
    census = XC.sponge_census(cfgs)
    print("sponge census:", census)
    assert census["fill positions"] == 168
    assert census["prefix crosses a block"] > 0 and census["prefix fills a block exactly"] > 0
    for end in XC.SPONGE_ENDS:
        # every f that can reach the end with a body of at least one byte does
        # (168 fill positions; the prefix lengths 168..170 repeat f = 0, 1, 2)
        assert census["f + nbytes == %d" % end] == min(end, 168) + sum(1 for f in (0, 1, 2) if end - f > 0), end
    for nb in XC.SPONGE_FIXED:
        assert census["nbytes == %d" % nb] >= len(XC.SPONGE_PREFIX_LENS)
    assert len(set(cfgs)) == len(cfgs)


def test_node_proof_grid_census():
    cfgs = XC.node_proof_cfgs()
    census = XC.node_proof_census(cfgs)
    print("node proof census:", census)
    assert len(cfgs) == 168 * 9 and len(set(cfgs)) == len(cfgs)
    assert census["q values"] == 42 and census["shifts"] == 4
    assert all(v > 0 for v in census.values()), census
    assert census["path 1: f + nbytes == 167"] == 1 and census["path 32: f + nbytes == 168"] == 1


def test_absorb_grid_census():
    items = XC.absorb_items()
    census = XC.absorb_census(items)
    print("absorb census:", census)
    assert census["fill positions"] == 168 and len(set(items)) == len(items)
    for nb in XC.AB_FIXED:
        assert census["nbytes == %d" % nb] == 168
    for d in (42, 43, 44):
        assert census["second block: nw - base == %d" % d] >= 168
    assert census["ends on a block boundary"] > 0 and census["three or more blocks"] > 0
    assert all(n % 4 == 0 and n > 0 for (_, n) in items)
    launches = XC.absorb_launches(items)
    assert len(launches) == (len(items) + 1) // 2 and {l[4] for l in launches} == {0, 3}
    assert {(l[0], l[1]) for l in launches} | {(l[2], l[3]) for l in launches} == set(items)
    plane = XC.absorb_items(XC.AB_PLANE_FS)
    assert {f & 3 for (f, _) in plane} == {0, 1, 2, 3} and len({f >> 2 for (f, _) in plane}) == 3
    chains = XC.absorb_chain_launches()
    assert len(XC.AB_CHAINS) == 12 and len(chains) == 18
    for j in range(0, len(chains), 3):
        (a, b, c) = chains[j:j + 3]
        for w in (0, 1):
            assert b[2 * w] == (a[2 * w] + a[2 * w + 1]) % 168 and c[2 * w + 1] == a[2 * w + 1] + b[2 * w + 1]


def test_aes_group_ops_stay_inside_their_groups():
    for (kind, ha, hb, ca, cb) in XC.AES_GROUP_OPS:
        if kind != 3:
            assert ha >> 8 == ca >> 8
        if kind == 1:
            assert ha >> 8 == cb >> 8
        if kind in (2, 4):
            assert hb >> 8 == cb >> 8
    assert any(ha & 0xff for (_, ha, _, _, _) in XC.AES_GROUP_OPS)
    assert {0, 1, 2, 3, 4} == {k for (k, *_) in XC.AES_GROUP_OPS}
