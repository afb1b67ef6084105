"""The XOF layer's device code alone, bit for bit against a plain reference.
tests/host/xof_ops.hip (a test-only library built by build()) runs csrc/keccak.hpp,
csrc/aes.hpp and the sponge and node-proof code of csrc/absorb_kernels.hpp,
finish_kernels.hpp, planes.hpp and node_proof.hpp on chosen
inputs; end to end those functions only see what an honest client's randomness
and a handful of ctx lengths produce.  The reference is tests/xof_ref.py
(pinned by tests/test_xof_ref.py, which also holds the case lists of
tests/xof_cases.py to their classes) and oracle._prims.

A  the four permutation variants (fused / unfused theta, the two-lane form
   with DPP and with LDS-crossbar exchange) on the zero state, the all-ones
   state, the 1600 one-bit states and 200 random states.
B  sponge_absorb_bytes_slow (through k_prefix_states), sponge_absorb_words,
   sponge_pad and sponge_squeeze_words: prefixes of every length 0..170, so f
   takes all 168 values and the slow absorb crosses a block, times the body
   lengths of xof_cases.sponge_cfgs; domain 0x01 / 32 bytes and 0x02 / 16
   bytes.  sponge_absorb_words requires the bytes of the last word past
   nbytes to be zero; the harness's loader masks them.
C  sponge_squeeze_vec through squeeze_elems + pl_store_lane from chosen
   states, both fields: every rejection position and run of block 0, the
   boundary values of both moduli, counts around one and two blocks.  The
   output planes are pre-filled and compared whole.
D  node_proof_one<true> and <false>: every f in 0..167 times path_bytes 1, 2,
   3, 4, 5, 8, 16, 31, 32 (all 42 switch cases, all 4 shifts, the crossing
   path, the domain byte beside the 0x80 pad), t mixed inside each wave.
E  k_absorb and k_absorb_pair, the product kernels, with the product's grid
   shapes: every f, independent lengths on the two sponges of one launch,
   the lengths at which the second block's in-range test flips, a sponge with
   nbytes = 0, chained launches, tiled and plane layouts; stride 128 with 70
   reports, all 50 planes of both sponges compared, padding lanes included.
   nbytes are multiples of 4: that is what the host passes (32 bytes per node
   proof, whole field elements).
F  fixed-key AES on the AesLds path (k_setup's) and the AesPerm path (the
   level kernel's, table at LDS address 0): per lane its own key, every
   table entry of the lane's copy, counters around every byte carry, the
   counter groups (ctr_blocks_n<4>, which has no caller, included).

Every launch has more than 64 lanes (70: a partly filled second wave).

Host-side reference times on the CPU (one core), measured: A 0.3 s, B 1.8 s
(431,000 TurboSHAKE calls of the oracle), C 0.02 s, D 0.5 s (106,000 calls),
E 3.5 s for the tiled grid (about 400,000 lane permutations in numpy, computed
once for both kernels) and 0.2 s for the plane layout, F 0.1 s.  No grid is
thinned.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import ROOT
import xof_cases as XC
import xof_ref as R
from oracle import _prims
from test_gpu_parity import mastic_amd  # noqa: F401

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "host", "_build", "libxof_ops.so")
LANES = XC.LANES
SENTINEL = 0xA5C3961E


@pytest.fixture(scope="module")
def xof_ops():
    if not os.path.exists(LIB):
        pytest.fail("libxof_ops.so missing: build() was not run")
    return _bind(LIB)


def _bind(path):
    lib = ctypes.CDLL(path)
    (i, sz, P) = (ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p)
    for (name, args) in [("xof_ops_perm", [i, sz, P, P]),
                         ("xof_ops_sponge", [i, P, P, P, sz, P, i, i, i, P, P, P]),
                         ("xof_ops_squeeze", [i, sz, i, i, i, P, P]),
                         ("xof_ops_node_proof", [i, P, P, P, sz, P, i, P, P, P]),
                         ("xof_ops_absorb", [i, i, i, i, sz, P, P, P, P, sz, P]),
                         ("xof_ops_aes", [i, i, i, i, i, P, P, P, P, P, P, P, P])]:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = args
    return lib


def _ptr(a):
    """(holds no reference: the array must outlive the call)"""
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


def _first_bad(got, want):
    """index of the first differing entry along the leading axes"""
    bad = np.argwhere(got != want)
    return None if bad.size == 0 else tuple(int(x) for x in bad[0])


def _census(name, census):
    """printed and asserted here as in tests/test_xof_ref.py: no edge class is empty"""
    print("%s census: %s" % (name, census))
    assert all(v > 0 for v in census.values()), (name, census)


# ---------------------------------------------------------------- A
@functools.lru_cache(maxsize=None)
def _perm_states():
    rng = np.random.default_rng(11)
    one_bit = np.zeros((1600, 25), np.uint64)
    for b in range(1600):
        one_bit[b, b // 64] = np.uint64(1) << np.uint64(b % 64)
    st = np.concatenate([np.zeros((1, 25), np.uint64), np.full((1, 25), 2 ** 64 - 1, np.uint64), one_bit,
                         rng.integers(0, 2 ** 64, size=(200, 25), dtype=np.uint64)])
    return (st, R.keccak_p12(st))


@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=["p12_fused", "p12_unfused", "pair_dpp", "pair_swz"])
def test_permutation_variants(xof_ops, variant):
    (st, want) = _perm_states()
    got = np.zeros_like(st)
    assert xof_ops.xof_ops_perm(variant, len(st), _ptr(st), _ptr(got)) == 0
    bad = _first_bad(got, want)
    assert bad is None, ("state (0 zero, 1 ones, 2.. one bit, 1602.. random), word", bad)


# ---------------------------------------------------------------- prefixes of B and D
def _prefixes(lens, seed):
    rng = np.random.default_rng(seed)
    raw = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens]
    offs = np.cumsum([0] + [len(b) for b in raw[:-1]]).astype(np.int32)
    blob = np.frombuffer(b"".join(raw) + b"\0", np.uint8).copy()
    return (raw, blob, offs, np.array(lens, np.int32))


# ---------------------------------------------------------------- B
@functools.lru_cache(maxsize=None)
def _sponge_inputs():
    cfgs = XC.sponge_cfgs()
    (raw, blob, offs, lens) = _prefixes(XC.SPONGE_PREFIX_LENS, 21)
    maxw = (max(nb for (_, nb) in cfgs) + 3) // 4
    body = np.random.default_rng(22).integers(0, 2 ** 32, size=(maxw, 128), dtype=np.uint32)
    return (cfgs, raw, blob, offs, lens, maxw, body)


@functools.lru_cache(maxsize=None)
def _sponge_expected():
    (cfgs, raw, _, _, _, maxw, body) = _sponge_inputs()
    lane_bytes = [np.ascontiguousarray(body[:, r]).astype("<u4").tobytes() for r in range(LANES)]
    want = np.zeros((len(cfgs), LANES, 48), np.uint8)
    ts = _prims.turboshake128
    for (c, (L, nb)) in enumerate(cfgs):
        for r in range(LANES):
            msg = raw[L] + lane_bytes[r][:nb]
            want[c, r] = np.frombuffer(ts(msg, 1, 32) + ts(msg, 2, 16), np.uint8)
    return want


def test_one_lane_sponge(xof_ops):
    (cfgs, raw, blob, offs, lens, maxw, body) = _sponge_inputs()
    want = _sponge_expected()
    _census("sponge", XC.sponge_census(cfgs))
    cfg = np.array(cfgs, np.int32)  # the prefix index is its length
    got = np.zeros((len(cfgs), LANES, 12), np.uint32)
    pfx_f = np.full(len(raw), -1, np.int32)
    rc = xof_ops.xof_ops_sponge(len(raw), _ptr(blob), _ptr(offs), _ptr(lens), len(cfgs), _ptr(cfg), LANES, 128, maxw,
                                _ptr(body), _ptr(got), _ptr(pfx_f))
    assert rc == 0
    assert pfx_f.tolist() == [n % 168 for n in XC.SPONGE_PREFIX_LENS]
    gb = got.view(np.uint8).reshape(len(cfgs), LANES, 48)
    for (name, sl) in (("domain 1, 32 bytes", slice(0, 32)), ("domain 2, 16 bytes", slice(32, 48))):
        bad = _first_bad(gb[:, :, sl], want[:, :, sl])
        assert bad is None, (name, "(prefix length, body bytes)", cfgs[bad[0]], "lane", bad[1], "byte", bad[2])


# ---------------------------------------------------------------- C
@functools.lru_cache(maxsize=None)
def _squeeze_expected(bits):
    (p, enc, _) = XC.FIELDS[bits]
    cases = XC.squeeze_cases(bits)
    st = XC.squeeze_states(bits, cases)
    return (cases, st, {count: R.next_vec_from_states(st, p, enc, count) for count in XC.squeeze_counts(bits)})


@pytest.mark.parametrize("bits", [64, 128])
def test_next_vec_from_chosen_states(xof_ops, bits):
    (cases, st, expected) = _squeeze_expected(bits)
    w32 = bits // 32
    S = 128
    assert len(cases) > 64
    _census("squeeze Field%d" % bits, XC.squeeze_census(bits, cases))
    for (count, res) in expected.items():
        rows = (count + 2) * w32  # two guard elements after the last
        want = np.full((rows, S), SENTINEL, np.uint32)
        for (r, (vals, _)) in enumerate(res):
            for (e, v) in enumerate(vals):
                for i in range(w32):
                    want[e * w32 + i, r] = (v >> (32 * i)) & 0xffffffff
        got = np.full((rows, S), SENTINEL, np.uint32)
        assert xof_ops.xof_ops_squeeze(bits, len(cases), S, count, rows, _ptr(st), _ptr(got)) == 0
        bad = _first_bad(got.T, want.T)
        assert bad is None, ("count", count, "lane", bad[0], cases[bad[0]].name if bad[0] < len(cases) else "no lane",
                             "plane row", bad[1], hex(int(got[bad[1], bad[0]])), hex(int(want[bad[1], bad[0]])))


# ---------------------------------------------------------------- D
@functools.lru_cache(maxsize=None)
def _node_proof_inputs():
    cfgs = XC.node_proof_cfgs()
    (raw, blob, offs, lens) = _prefixes(XC.NP_PREFIX_LENS, 31)
    rng = np.random.default_rng(32)
    rec = rng.integers(0, 2 ** 32, size=(LANES, 21), dtype=np.uint32)
    rec[:, 20] = rng.integers(0, 2, size=LANES)  # t, mixed inside each wave
    assert 0 < rec[:64, 20].sum() < 64 and 0 < rec[64:, 20].sum() < LANES - 64
    return (cfgs, raw, blob, offs, lens, rec)


@functools.lru_cache(maxsize=None)
def _node_proof_expected():
    (cfgs, raw, _, _, _, rec) = _node_proof_inputs()
    seed = [rec[r, 0:4].astype("<u4").tobytes() for r in range(LANES)]
    path = [rec[r, 12:20].astype("<u4").tobytes() for r in range(LANES)]
    want = np.zeros((len(cfgs), LANES, 8), np.uint32)
    for (c, (L, pb)) in enumerate(cfgs):
        (bits, level) = (8 * pb, 8 * pb - 1)
        mid = bits.to_bytes(2, "little") + level.to_bytes(2, "little")
        for r in range(LANES):
            want[c, r] = np.frombuffer(_prims.turboshake128(raw[L] + seed[r] + mid + path[r][:pb], 1, 32), "<u4")
    want ^= rec[None, :, 4:12] * rec[None, :, 20:21]  # the proof correction word where t
    return want


def test_node_proof_one(xof_ops):
    (cfgs, raw, blob, offs, lens, rec) = _node_proof_inputs()
    want = _node_proof_expected()
    _census("node proof", XC.node_proof_census(cfgs))
    cfg = np.array(cfgs, np.int32)
    got = np.zeros((len(cfgs), LANES, 16), np.uint32)
    pfx_f = np.full(len(raw), -1, np.int32)
    rc = xof_ops.xof_ops_node_proof(len(raw), _ptr(blob), _ptr(offs), _ptr(lens), len(cfgs), _ptr(cfg), LANES,
                                    _ptr(rec), _ptr(got), _ptr(pfx_f))
    assert rc == 0
    assert pfx_f.tolist() == XC.NP_PREFIX_LENS
    for (name, sl) in (("node_proof_one<true>", slice(0, 8)), ("node_proof_one<false>", slice(8, 16))):
        bad = _first_bad(got[:, :, sl], want)
        assert bad is None, (name, "(f, path_bytes)", cfgs[bad[0]], "lane", bad[1], "t", int(rec[bad[1], 20]),
                             "word", bad[2])


# ---------------------------------------------------------------- E
AB_POOL_WORDS = 2 * 64 * 200


@functools.lru_cache(maxsize=None)
def _absorb_data():
    rng = np.random.default_rng(41)
    S = XC.AB_STRIDE
    init = rng.integers(0, 2 ** 32, size=(2, 50, S), dtype=np.uint32)
    pools = [rng.integers(0, 2 ** 32, size=AB_POOL_WORDS, dtype=np.uint32) for _ in range(2)]
    states = [np.ascontiguousarray(init[w].T).view(np.uint64) for w in range(2)]  # (S, 25): planes 2i, 2i + 1 = lo, hi
    return (init, pools, states)


def _absorb_reference(entries, layout):
    """entries: (sponge, f, nbytes, tot, skip), the stream words [skip, skip +
    nbytes / 4) of a segment of tot words per report that ends with the pool.
    Returns (len(entries), stride, 25): every lane's state after the absorb."""
    (_, pools, states) = _absorb_data()
    S = XC.AB_STRIDE
    lane = np.arange(S)
    out = np.zeros((len(entries), S, 25), np.uint64)
    step = 64
    for i0 in range(0, len(entries), step):
        part = entries[i0:i0 + step]
        maxw = max(max(nb for (_, _, nb, _, _) in part) // 4, 1)
        m = np.arange(maxw)
        st = np.concatenate([states[w] for (w, _, _, _, _) in part])
        data = np.zeros((len(part), S, maxw), np.uint32)
        for (j, (w, f, nb, tot, skip)) in enumerate(part):
            if layout == 0:  # tiled: rstride 64, gstride tot * 64
                base = AB_POOL_WORDS - (S // 64) * tot * 64 + skip * 64
                idx = base + (lane // 64)[:, None] * tot * 64 + m[None, :] * 64 + (lane % 64)[:, None]
            else:  # planes: rstride stride, gstride 64
                base = AB_POOL_WORDS - tot * S + skip * S
                idx = base + (lane // 64)[:, None] * 64 + m[None, :] * S + (lane % 64)[:, None]
            data[j] = pools[w][np.minimum(idx, AB_POOL_WORDS - 1)]  # (words past nbytes are not absorbed)
        fs = np.repeat([f for (_, f, _, _, _) in part], S)
        nbs = np.repeat([nb for (_, _, nb, _, _) in part], S)
        (res, _) = R.absorb(st, fs, data.astype("<u4").view(np.uint8).reshape(len(part) * S, maxw * 4), nbs)
        out[i0:i0 + len(part)] = res.reshape(len(part), S, 25)
    return out


def _entries_of(launches):
    """the reference's view of every launch: what each sponge has absorbed
    since the initial planes when the launch ends (a chained launch: both pieces)"""
    out = []
    prev = None
    for l in launches:
        (f0, n0, f1, n1, _prio, reset, t0, t1, s0, s1) = l
        if reset:
            cur = [(0, f0, n0, t0, s0), (1, f1, n1, t1, s1)]
        else:
            cur = [(w, pf, pn + n, t, ps) for ((w, pf, pn, t, ps), n) in zip(prev, (n0, n1))]
        out += cur
        prev = cur
    return out


@functools.lru_cache(maxsize=None)
def _absorb_expected(which):
    if which == "grid":
        items = XC.absorb_items()
        launches = XC.absorb_launches(items)
        # one sponge with nbytes = 0 (either one): its planes come back untouched
        launches += [(5, 0, 9, 172, 3, 1, 0, 43, 0, 0), (166, 340, 3, 0, 0, 1, 85, 0, 0, 0)]
        launches += XC.absorb_chain_launches()
        layout = 0
    else:
        launches = XC.absorb_launches(XC.absorb_items(XC.AB_PLANE_FS))
        layout = 1
    want = _absorb_reference(_entries_of(launches), layout)
    return (launches, layout, want.reshape(len(launches), 2, XC.AB_STRIDE, 25))


@pytest.mark.parametrize("which", ["grid", "planes"])
@pytest.mark.parametrize("pair", [0, 1], ids=["k_absorb", "k_absorb_pair"])
def test_absorb_kernels(xof_ops, pair, which):
    (init, pools, states) = _absorb_data()
    (launches, layout, want) = _absorb_expected(which)
    S = XC.AB_STRIDE
    _census("absorb " + which, XC.absorb_census([(l[2 * w], l[2 * w + 1]) for l in launches for w in (0, 1)]
                                                if which == "grid" else XC.absorb_items(XC.AB_PLANE_FS)))
    cases = np.array(launches, np.int32)
    got = np.zeros((len(launches), 2, 50, S), np.uint32)
    rc = xof_ops.xof_ops_absorb(pair, layout, XC.AB_N, S, len(launches), _ptr(cases), _ptr(init), _ptr(pools[0]),
                                _ptr(pools[1]), AB_POOL_WORDS, _ptr(got))
    assert rc == 0
    gs = np.ascontiguousarray(got.transpose(0, 1, 3, 2)).view(np.uint64)  # (launch, sponge, lane, 25)
    bad = _first_bad(gs, want)
    assert bad is None, ("launch (f0, nb0, f1, nb1, prio, reset, tot0, tot1, skip0, skip1)", launches[bad[0]],
                         "sponge", bad[1], "lane", bad[2], "word", bad[3])
    if which == "grid":
        zero = [i for (i, l) in enumerate(launches) if l[1] == 0 or l[3] == 0]
        assert len(zero) == 2
        for i in zero:
            w = 0 if launches[i][1] == 0 else 1
            assert np.array_equal(got[i, w], init[w]), "planes of a sponge with nbytes = 0 changed"
        # chained launches: the second piece ends where the concatenation alone does
        chained = [i for (i, l) in enumerate(launches) if l[5] == 0]
        assert len(chained) == len(XC.AB_CHAINS) // 2
        for i in chained:
            assert np.array_equal(got[i], got[i + 1]), ("chained launches differ from one launch", launches[i])


# ---------------------------------------------------------------- F
@functools.lru_cache(maxsize=None)
def _aes_inputs():
    rng = np.random.default_rng(51)
    rec = rng.integers(0, 2 ** 32, size=(LANES, 12), dtype=np.uint32)  # key, seed a, seed b
    v = (np.arange(256, dtype=np.uint32) * np.uint32(0x01010101))
    blocks = np.ascontiguousarray(rec[:, None, 0:4] ^ v[None, :, None])  # k0 XOR (v in all 16 bytes)
    return (rec, blocks, np.array(XC.AES_CTRS, np.uint32), np.array(XC.AES_GROUP_OPS, np.uint32))


@functools.lru_cache(maxsize=None)
def _aes_expected():
    (rec, blocks, ctrs, ops) = _aes_inputs()
    rks = [_prims.aes128_expand(rec[r, 0:4].astype("<u4").tobytes()) for r in range(LANES)]
    rk = np.array([np.frombuffer(k, "<u4") for k in rks], np.uint32)
    ct = np.zeros_like(blocks)
    for r in range(LANES):
        for b in range(blocks.shape[1]):
            ct[r, b] = np.frombuffer(_prims.aes128_encrypt(rks[r], blocks[r, b].astype("<u4").tobytes()), "<u4")
    used = sorted(set(int(c) for c in ctrs) | {int(o[j]) ^ x for o in ops for j in (3, 4) for x in (0, 1)})
    fk = {}
    for r in range(LANES):
        for (s, sl) in (("a", slice(4, 8)), ("b", slice(8, 12))):
            seed = rec[r, sl].astype("<u4").tobytes()
            for c in used:
                fk[(r, s, c)] = np.frombuffer(_prims.fixed_key_aes_blocks(rks[r], seed, c, 1), "<u4")
    return (rk, ct, fk)


def _fk_rows(fk, ctrs, layout):
    """layout: per output block (seed, counter offset)"""
    n = len(ctrs)
    out = np.zeros((LANES, n, 4 * len(layout)), np.uint32)
    for r in range(LANES):
        for i in range(n):
            for (k, (s, d)) in enumerate(layout):
                out[r, i, 4 * k:4 * k + 4] = fk[(r, s, int(ctrs[(i + d) % n]))]
    return out


def test_fixed_key_aes_lds_path(xof_ops):
    (rec, blocks, ctrs, _) = _aes_inputs()
    (rk_want, ct_want, fk) = _aes_expected()
    rk = np.zeros((LANES, 44), np.uint32)
    ct = np.zeros_like(blocks)
    got = np.zeros((LANES, len(ctrs), 16), np.uint32)
    none = np.zeros(8, np.uint32)
    rc = xof_ops.xof_ops_aes(0, LANES, blocks.shape[1], len(ctrs), 0, _ptr(rec), _ptr(rk), _ptr(blocks), _ptr(ctrs),
                             _ptr(none), _ptr(ct), _ptr(got), _ptr(none))
    assert rc == 0
    assert _first_bad(rk, rk_want) is None, ("aes128_expand: lane, word", _first_bad(rk, rk_want))
    assert _first_bad(ct, ct_want) is None, ("aes128_encrypt: lane, table entry, word", _first_bad(ct, ct_want))
    want = _fk_rows(fk, ctrs, [("a", 0), ("a", 0), ("a", 0), ("b", 1)])
    bad = _first_bad(got, want)
    assert bad is None, ("lane", bad[0], "counter", hex(int(ctrs[bad[1]])),
                         "word (0 RkRegs, 4 RkLds, 8 fixed_key_block2)", bad[2])


def test_fixed_key_aes_perm_path(xof_ops):
    (rec, blocks, ctrs, ops) = _aes_inputs()
    (rk_want, ct_want, fk) = _aes_expected()
    rk = rk_want.copy()
    ct = np.zeros_like(blocks)
    got = np.zeros((LANES, len(ctrs), 36), np.uint32)
    grp = np.zeros((LANES, len(ops), 16), np.uint32)
    rc = xof_ops.xof_ops_aes(1, LANES, blocks.shape[1], len(ctrs), len(ops), _ptr(rec), _ptr(rk), _ptr(blocks),
                             _ptr(ctrs), _ptr(ops), _ptr(ct), _ptr(got), _ptr(grp))
    assert rc == 0, "(-2: the table was not at LDS address 0)"
    assert _first_bad(ct, ct_want) is None, ("aes128_encrypt: lane, table entry, word", _first_bad(ct, ct_want))
    want = _fk_rows(fk, ctrs, [("a", 0), ("a", 0), ("b", 1), ("a", 0), ("b", 1), ("a", 2), ("b", 3), ("a", 0),
                               ("b", 1)])
    bad = _first_bad(got, want)
    assert bad is None, ("lane", bad[0], "counter", hex(int(ctrs[bad[1]])),
                         "word (0 <1>, 4 <2>, 12 <4>, 28 fixed_key_block2)", bad[2])
    gw = np.zeros_like(grp)
    for r in range(LANES):
        for (k, (kind, _ha, _hb, ca, cb)) in enumerate(XC.AES_GROUP_OPS):
            gw[r, k, 0:4] = fk[(r, "a", ca)]
            if kind == 1:
                gw[r, k, 4:8] = fk[(r, "a", cb)]
            if kind in (2, 4):
                gw[r, k, 4:8] = fk[(r, "b", cb)]
            if kind == 4:  # ctr_blocks_n<4>
                gw[r, k, 8:12] = fk[(r, "a", ca ^ 1)]
                gw[r, k, 12:16] = fk[(r, "b", cb ^ 1)]
    bad = _first_bad(grp, gw)
    assert bad is None, ("counter groups: lane", bad[0], "op (kind, hi_a, hi_b, c_a, c_b)",
                         [hex(x) for x in XC.AES_GROUP_OPS[bad[1]]], "word", bad[2])


# ---------------------------------------------------------------- refusals
def test_harness_refuses_what_could_leave_its_buffers(xof_ops):
    """the -1 paths: every one returns before anything is allocated or launched"""
    z = np.zeros(4096, np.uint32)
    zi = np.zeros(64, np.int32)
    p = _ptr(z)
    assert xof_ops.xof_ops_perm(4, 70, p, p) == -1
    assert xof_ops.xof_ops_perm(0, 0, p, p) == -1
    # sponge: a prefix index past the list, a body longer than the planes, more lanes than a row, S < lanes
    one = np.array([0], np.int32)
    for (cfg, lanes, S, maxw) in (((1, 4), 70, 128, 4), ((0, 17), 70, 128, 4), ((0, 4), 129, 256, 4),
                                  ((0, 4), 70, 64, 4), ((0, -4), 70, 128, 4), ((0, 4), 0, 128, 4)):
        c = np.array(cfg, np.int32)
        assert xof_ops.xof_ops_sponge(1, p, _ptr(one), _ptr(one), 1, _ptr(c), lanes, S, maxw, p, p, _ptr(zi)) == -1
    assert xof_ops.xof_ops_sponge(1, p, _ptr(one), _ptr(one), 0, _ptr(one), 70, 128, 4, p, p, _ptr(zi)) == -1
    # squeeze: fewer rows than count elements, a stride below the lanes, an unknown field, count 0
    assert xof_ops.xof_ops_squeeze(64, 70, 128, 21, 41, p, p) == -1
    assert xof_ops.xof_ops_squeeze(128, 70, 128, 10, 39, p, p) == -1
    assert xof_ops.xof_ops_squeeze(64, 70, 64, 1, 2, p, p) == -1
    assert xof_ops.xof_ops_squeeze(32, 70, 128, 1, 2, p, p) == -1
    assert xof_ops.xof_ops_squeeze(64, 70, 128, 0, 2, p, p) == -1
    # node proofs: path_bytes outside 1..32
    for pb in (0, 33, -1):
        c = np.array((0, pb), np.int32)
        assert xof_ops.xof_ops_node_proof(1, p, _ptr(one), _ptr(one), 1, _ptr(c), 70, p, p, _ptr(zi)) == -1
    # absorb: f outside 0..167, nbytes no multiple of 4, a window past its segment, a segment past the pool,
    # a stride that is no multiple of 64, more reports than the stride, a first case that continues nothing
    good = (0, 8, 0, 8, 3, 1, 2, 2, 0, 0)
    for (i, v) in ((0, 168), (2, -1), (1, 6), (3, -4), (8, 1), (6, 1 << 20), (4, 4), (5, 0)):
        k = list(good)
        k[i] = v
        c = np.array(k, np.int32)
        assert xof_ops.xof_ops_absorb(0, 0, 70, 128, 1, _ptr(c), p, p, p, 4096, p) == -1, (i, v)
    c = np.array(good, np.int32)
    assert xof_ops.xof_ops_absorb(1, 0, 70, 100, 1, _ptr(c), p, p, p, 4096, p) == -1
    assert xof_ops.xof_ops_absorb(1, 0, 129, 128, 1, _ptr(c), p, p, p, 4096, p) == -1
    assert xof_ops.xof_ops_absorb(2, 0, 70, 128, 1, _ptr(c), p, p, p, 4096, p) == -1
    assert xof_ops.xof_ops_absorb(0, 0, 70, 128, 0, _ptr(c), p, p, p, 4096, p) == -1
    # AES: a counter outside its group, a block from a group that was never initialised, group ops on the AesLds path
    for op in ((0, 0, 0, 0x100, 0), (1, 0, 0, 0, 0x100), (2, 0, 0, 0, 0x100), (3, 0, 0, 0, 0), (4, 0, 0, 0, 0x100),
               (5, 0, 0, 0, 0)):
        o = np.array(op, np.uint32)
        assert xof_ops.xof_ops_aes(1, 70, 1, 1, 1, p, p, p, p, _ptr(o), p, p, p) == -1, op
    o = np.array((0, 0, 0, 0, 0), np.uint32)
    assert xof_ops.xof_ops_aes(0, 70, 1, 1, 1, p, p, p, p, _ptr(o), p, p, p) == -1
    assert xof_ops.xof_ops_aes(1, 129, 1, 1, 0, p, p, p, p, _ptr(o), p, p, p) == -1
    assert xof_ops.xof_ops_aes(1, 70, 0, 1, 0, p, p, p, p, _ptr(o), p, p, p) == -1
