"""csrc/flp.hpp's device code against oracle.flp.FlpBBCGGI19, bit for bit.
tests/host/flp_ops.hip (a test-only library built by build()) runs flp_prove,
flp_query (num_shares = 2) and flp_decide on chosen inputs, one lane per case,
with the product's constants.  Unlike the end-to-end tests, the randomness is
explicit, so the cases include what TurboSHAKE output reaches with probability
2^-62: a test point on every P-th root of unity (the query aborts), test
points 0, 2, p-2 and one with t^P = -1, joint randomness of 0 and p-1, prove
randomness of 0, a reducing query rand of 0 and shares of 0 and p-1; and
dishonest encodings (tests/flp_grid.py), whose decide must be false, as the
plain predicate of tests/test_oracle_flp_grid.py says.

Per shape: the expected values of every case first, then three launches
(prove, query of both shares, decide), each of more than 64 lanes.
"""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import ROOT
import flp_grid as G
from oracle.flp import FlpBBCGGI19
from test_gpu_parity import mastic_amd  # noqa: F401
from test_oracle_flp_grid import is_valid

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "host", "_build", "libflp_ops.so")
MIN_CASES = 70  # every launch covers a second wave and a partly filled stride


@pytest.fixture(scope="module")
def flp_ops():
    if not os.path.exists(LIB):
        pytest.fail("libflp_ops.so missing: build() was not run")
    return _bind(LIB)


def _bind(path):
    lib = ctypes.CDLL(path)
    (i, u64, sz, P) = (ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p)
    shape = [i, i, i, u64, i]
    for (name, extra) in [("flp_ops_sizes", [P]), ("flp_ops_prove", [sz, P, P, P, P]),
                          ("flp_ops_query", [sz, P, P, P, P, P, P]), ("flp_ops_decide", [sz, P, P])]:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = shape + extra
    return lib


def _shape_args(shape):
    (circuit, kw) = shape
    return (G.CIRCUIT_IDS[circuit], kw.get("length", 0), kw.get("sum_vec_bits", 0), kw.get("max_measurement", 0),
            kw.get("chunk_length", 0))


def _pack(rows, enc):
    """case-major little-endian elements"""
    data = b"".join(x.to_bytes(enc, "little") for row in rows for x in row)
    return np.frombuffer(data if data else bytes(enc), np.uint8).copy()


def _unpack(arr, n, elems, enc):
    raw = arr.tobytes()
    return [[int.from_bytes(raw[(c * elems + e) * enc:(c * elems + e + 1) * enc], "little") for e in range(elems)]
            for c in range(n)]


def _ptr(a):
    """(holds no reference: the array must outlive the call)"""
    return ctypes.c_void_p(a.ctypes.data)


class Case:
    """One lane: explicit inputs of prove and of both queries."""

    def __init__(self, name, meas, prand, jr, qr, m0, p0, honest=None):
        (self.name, self.meas, self.prand, self.jr, self.qr, self.m0, self.p0) = (name, meas, prand, jr, qr, m0, p0)
        self.honest = honest  # None: decide is only compared with the oracle's


def _build_cases(shape, flp, rng):
    f = flp.field
    p = f.MODULUS
    big_p = flp.valid.GADGET_CALLS[0] + 1
    P = 1
    while P < big_p:
        P *= 2
    alpha = pow(f.gen().val, f.GEN_ORDER // P, p)
    eol = flp.valid.EVAL_OUTPUT_LEN
    t_at = eol if eol > 1 else 0  # index of the test point in the query rand

    def vec(n):
        return [rng.randrange(p) for _ in range(n)]

    def case(name, enc, honest, **over):
        c = Case(name, list(enc), vec(flp.PROVE_RAND_LEN), vec(flp.JOINT_RAND_LEN), vec(flp.QUERY_RAND_LEN),
                 vec(flp.MEAS_LEN), vec(flp.PROOF_LEN), honest)
        for (k, v) in over.items():
            setattr(c, k, v)
        return c

    cases = []
    for m in G.boundary_measurements(shape):
        cases.append(case("honest %r" % (m,), G.encode(shape, m), True))
    for _ in range(5):
        cases.append(case("honest random", G.encode(shape, G.random_measurement(shape, rng)), True))
    for (name, enc) in G.dishonest_encodings(shape):
        cases.append(case("dishonest " + name, enc, False))

    # test-point edges share one honest measurement, proof and share split
    base = case("base", G.encode(shape, G.random_measurement(shape, rng)), True)

    def with_t(name, t, honest):
        qr = list(base.qr)
        qr[t_at] = t % p
        return Case(name, base.meas, base.prand, base.jr, qr, base.m0, base.p0, honest)
    for k in range(P):
        cases.append(with_t("t = alpha^%d" % k, pow(alpha, k, p), "abort"))
    assert pow(alpha, P // 2, p) == p - 1  # t = 1 and t = p-1 are among them
    for t in (0, 2, p - 2):
        cases.append(with_t("t = %d" % t, t, True))
    if P <= 64:
        beta = pow(f.gen().val, f.GEN_ORDER // (2 * P), p)  # primitive 2P-th root
        t = pow(beta, 3 if P > 1 else 1, p)
        assert pow(t, P, p) == p - 1
        cases.append(with_t("t^P = -1", t, True))

    # randomness edges, honest measurements
    def honest_enc():
        return G.encode(shape, G.random_measurement(shape, rng))
    if flp.JOINT_RAND_LEN > 0:
        for (i, x) in [(0, 0), (flp.JOINT_RAND_LEN - 1, p - 1), (0, p - 1), (flp.JOINT_RAND_LEN - 1, 0)]:
            c = case("joint rand[%d] = %d" % (i, x), honest_enc(), True)
            c.jr[i] = x
            cases.append(c)
    cases.append(case("prove rand 0", honest_enc(), True, prand=[0] * flp.PROVE_RAND_LEN))
    if eol > 1:
        for i in sorted({0, eol - 1}):
            c = case("query rand[%d] = 0" % i, honest_enc(), True)
            c.qr[i] = 0
            cases.append(c)
    cases.append(case("meas share 0", honest_enc(), True, m0=[0] * flp.MEAS_LEN))
    cases.append(case("meas share p-1", honest_enc(), True, m0=[p - 1] * flp.MEAS_LEN))
    cases.append(case("proof share 0", honest_enc(), True, p0=[0] * flp.PROOF_LEN))
    cases.append(case("proof share p-1", honest_enc(), True, p0=[p - 1] * flp.PROOF_LEN))
    while len(cases) - P < MIN_CASES:  # the decide launch gets the cases that do not abort
        cases.append(case("honest random", honest_enc(), True))
    return cases


def _expected(flp, cases):
    """Oracle proofs, verifier shares (None: the query raises) and decides."""
    f = flp.field
    p = f.MODULUS
    proofs = {}
    out = []
    for c in cases:
        key = (tuple(c.meas), tuple(c.prand), tuple(c.jr))
        if key not in proofs:
            proofs[key] = [x.val for x in flp.prove([f(x) for x in c.meas], [f(x) for x in c.prand],
                                                    [f(x) for x in c.jr])]
        proof = proofs[key]
        m1 = [(a - b) % p for (a, b) in zip(c.meas, c.m0)]
        p1 = [(a - b) % p for (a, b) in zip(proof, c.p0)]
        vers = []
        for (ms, ps) in [(c.m0, c.p0), (m1, p1)]:
            try:
                v = flp.query([f(x) for x in ms], [f(x) for x in ps], [f(x) for x in c.qr], [f(x) for x in c.jr], 2)
                vers.append([x.val for x in v])
            except ValueError as e:
                assert str(e) == "test point is a root of unity"
                vers.append(None)
        assert (vers[0] is None) == (vers[1] is None) == (c.honest == "abort"), c.name
        total = None if vers[0] is None else [(a + b) % p for (a, b) in zip(vers[0], vers[1])]
        decide = None if total is None else flp.decide([f(x) for x in total])
        out.append((proof, [c.m0, m1], [c.p0, p1], vers, total, decide))
    return out


@pytest.mark.parametrize("shape", [G.COUNT] + G.GRID, ids=G.shape_id)
def test_device_flp_matches_oracle(mastic_amd, flp_ops, shape):  # noqa: F811
    (circuit, kw) = shape
    rng = random.Random("gpu flp ops " + G.shape_id(shape))
    flp = FlpBBCGGI19(G.oracle_valid(shape))
    enc = flp.field.ENCODED_SIZE
    args = _shape_args(shape)
    sizes = (ctypes.c_int * 8)()
    assert flp_ops.flp_ops_sizes(*args, sizes) == 0
    assert list(sizes)[:7] == [8 * enc, flp.MEAS_LEN, flp.PROVE_RAND_LEN, flp.JOINT_RAND_LEN, flp.QUERY_RAND_LEN,
                               flp.PROOF_LEN, flp.VERIFIER_LEN]

    cases = _build_cases(shape, flp, rng)
    want = _expected(flp, cases)
    n = len(cases)
    assert n > 64

    # the oracle's verdicts first: honest accepted, dishonest rejected, as the plain predicate says
    for (c, w) in zip(cases, want):
        if c.honest is True or c.honest is False:
            assert is_valid(circuit, kw, c.meas) == c.honest, c.name
            assert w[5] == c.honest, "%s: oracle decide %s" % (c.name, w[5])

    # prove
    got = np.zeros(n * flp.PROOF_LEN * enc, np.uint8)
    bufs = [_pack([c.meas for c in cases], enc), _pack([c.prand for c in cases], enc),
            _pack([c.jr for c in cases], enc)]
    rc = flp_ops.flp_ops_prove(*args, n, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), _ptr(got))
    assert rc == 0, "hip error %d" % rc
    for (c, w, g) in zip(cases, want, _unpack(got, n, flp.PROOF_LEN, enc)):
        assert g == w[0], "%s: proof differs from the oracle's" % c.name

    # query: lanes [0, n) are share 0 of each case, lanes [n, 2n) share 1
    ver = np.zeros(2 * n * flp.VERIFIER_LEN * enc, np.uint8)
    ok = np.full(2 * n, 255, np.uint8)
    bufs = [_pack([w[1][s] for s in range(2) for w in want], enc),
            _pack([w[2][s] for s in range(2) for w in want], enc),
            _pack([c.qr for c in cases] * 2, enc), _pack([c.jr for c in cases] * 2, enc)]
    rc = flp_ops.flp_ops_query(*args, 2 * n, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), _ptr(bufs[3]), _ptr(ver),
                               _ptr(ok))
    assert rc == 0, "hip error %d" % rc
    gver = _unpack(ver, 2 * n, flp.VERIFIER_LEN, enc)
    for s in range(2):
        for (i, (c, w)) in enumerate(zip(cases, want)):
            if w[3][s] is None:
                assert ok[s * n + i] == 0, "%s share %d: no abort on a root of unity" % (c.name, s)
            else:
                assert ok[s * n + i] == 1, "%s share %d: aborted" % (c.name, s)
                assert gver[s * n + i] == w[3][s], "%s share %d: verifier differs from the oracle's" % (c.name, s)

    # decide on the summed verifiers
    live = [(c, w) for (c, w) in zip(cases, want) if w[4] is not None]
    assert len(live) > 64
    dec = np.full(len(live), 255, np.uint8)
    sums = _pack([w[4] for (_c, w) in live], enc)
    rc = flp_ops.flp_ops_decide(*args, len(live), _ptr(sums), _ptr(dec))
    assert rc == 0, "hip error %d" % rc
    for ((c, w), d) in zip(live, dec):
        assert d == int(w[5]), "%s: device decide %d, oracle %s" % (c.name, d, w[5])
        if c.honest is False:
            assert d == 0, "%s: a dishonest encoding was accepted" % c.name
