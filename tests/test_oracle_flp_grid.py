"""The oracle's FLP against the circuits' plain definitions of "valid", over
the shape grid of tests/flp_grid.py plus Count.  oracle/flp.py restates
vdaf_poc.flp_bbcggi19 and is otherwise pinned only by the nine golden vectors;
the GPU code was written from the same reading of the draft.  Here, for honest
and dishonest encodings, decide(query_0 + query_1) must be true exactly when a
predicate written straight from the circuit definitions holds.

Soundness is probabilistic: a dishonest encoding is accepted with probability
about 2P/p (at most 2^-56 here) over the seeded randomness.  If a seed ever
lands on an accept, change the seed and say so; the assertion stays.
"""
import random

import pytest

import flp_grid as G
from oracle.flp import FlpBBCGGI19


def is_valid(circuit, params, encoded):
    """The circuit's definition of a valid encoding, over the integers."""
    def bits(xs):
        return all(x in (0, 1) for x in xs)

    def decode(xs):
        return sum(x << i for (i, x) in enumerate(xs))
    if circuit == "Count":
        return encoded[0] in (0, 1)
    if circuit == "Sum":
        b = params["max_measurement"].bit_length()
        offset = 2 ** b - 1 - params["max_measurement"]
        return len(encoded) == 2 * b and bits(encoded) and decode(encoded[:b]) + offset == decode(encoded[b:])
    if circuit == "SumVec":
        return bits(encoded)
    if circuit == "Histogram":
        return bits(encoded) and sum(encoded) == 1
    n = params["length"]
    offset = 2 ** params["max_measurement"].bit_length() - 1 - params["max_measurement"]
    return bits(encoded) and sum(encoded[:n]) + offset == decode(encoded[n:])


def shape_encodings(shape, rng, n_random=3):
    """[(name, encoded, honest)] of a shape: boundary and random honest
    measurements, then the dishonest encodings."""
    out = [("honest %r" % (m,), G.encode(shape, m), True) for m in G.boundary_measurements(shape)]
    for _ in range(n_random):
        out.append(("honest random", G.encode(shape, G.random_measurement(shape, rng)), True))
    out += [(name, enc, False) for (name, enc) in G.dishonest_encodings(shape)]
    return out


def run_flp(flp, rng, encoded):
    """prove, share, query twice, decide on the sum; all randomness from rng."""
    f = flp.field
    p = f.MODULUS

    def vec(n):
        return [f(rng.randrange(p)) for _ in range(n)]
    meas = [f(x) for x in encoded]
    joint_rand = vec(flp.JOINT_RAND_LEN)
    proof = flp.prove(meas, vec(flp.PROVE_RAND_LEN), joint_rand)
    query_rand = vec(flp.QUERY_RAND_LEN)
    (m0, p0) = (vec(len(meas)), vec(len(proof)))
    m1 = [a - b for (a, b) in zip(meas, m0)]
    p1 = [a - b for (a, b) in zip(proof, p0)]
    v0 = flp.query(m0, p0, query_rand, joint_rand, 2)
    v1 = flp.query(m1, p1, query_rand, joint_rand, 2)
    return flp.decide([a + b for (a, b) in zip(v0, v1)])


@pytest.mark.parametrize("shape", [G.COUNT] + G.GRID, ids=G.shape_id)
def test_oracle_decides_exactly_the_valid_encodings(shape):
    (circuit, kw) = shape
    rng = random.Random("oracle flp grid " + G.shape_id(shape))
    flp = FlpBBCGGI19(G.oracle_valid(shape))
    cases = shape_encodings(shape, rng)
    assert any(not honest for (_n, _e, honest) in cases)
    for (name, enc, honest) in cases:
        assert len(enc) == flp.MEAS_LEN
        assert is_valid(circuit, kw, enc) == honest, "%s: the predicate disagrees with the case list" % name
        assert run_flp(flp, rng, enc) == honest, "%s: oracle decide is %s" % (name, not honest)
