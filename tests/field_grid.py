"""Edge values for csrc/field.hpp, shared by tests/test_field_host.py (host
build) and tests/test_gpu_field_ops.py (gfx950 code generation), with Python
restatements of the two reduction routines that say which branch a pair takes.
The expected results themselves are plain Python integer arithmetic mod p."""
import random

P64 = 2 ** 64 - 2 ** 32 + 1
P128 = 2 ** 128 - 28 * 2 ** 64 + 1
C128 = 28 * 2 ** 64 - 1          # 2^128 mod p (F128::fold)
EPS64 = 2 ** 32 - 1              # 2^64 mod p (F64::reduce128)
M64 = 2 ** 64 - 1


def f128_fold_count(a, b):
    """F128::mul's fold loop: (iterations taken, value before the final
    conditional subtract).  Each iteration replaces L + 2^128 H by L + c H."""
    r = a * b
    n = 0
    while r >> 128:
        assert n < 5, "the loop is unrolled five times"
        r = (r & (2 ** 128 - 1)) + C128 * (r >> 128)
        n += 1
    return (n, r)


def f64_reduce_branches(a, b):
    """F64::reduce128 on a * b: (borrow in lo - hh, carry in t0 + t1, final
    conditional subtract taken)."""
    x = a * b
    (lo, hi) = (x & M64, x >> 64)
    (hh, hl) = (hi >> 32, hi & EPS64)
    t0 = (lo - hh) & M64
    borrow = lo < hh
    if borrow:
        t0 = (t0 - EPS64) & M64
    t1 = hl * EPS64
    t2 = (t0 + t1) & M64
    carry = t2 < t0
    if carry:
        t2 = (t2 + EPS64) & M64
    return (borrow, carry, t2 >= P64)


def _constructed(p, want, rng, tries=20000):
    """Pairs (a, b) with a * b mod p = a small chosen value: the products whose
    reduction ends just above p (final subtract) or needs one more fold."""
    out = []
    for _ in range(tries):
        b = rng.randrange(p // 2, p)
        v = rng.randrange(1, 2 ** rng.randrange(1, 80))
        a = v * pow(b, p - 2, p) % p
        if want(a, b):
            out.append((a, b))
            if len(out) == 3:
                break
    return out


def values(bits):
    """The grid of one field: edge values, 40 fixed-seed random values, and
    the members of constructed pairs (tests take all ordered pairs)."""
    rng = random.Random(64128 + bits)
    if bits == 64:
        p = P64
        edge = [0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, p - 1, p - 2, p - 2 ** 32, (p - 1) // 2, (p + 1) // 2,
                2 ** 63]
        extra = _constructed(p, lambda a, b: f64_reduce_branches(a, b)[2], rng)
    else:
        p = P128
        c = C128
        edge = [0, 1, c - 1, c, c + 1, p - 1, p - c, 2 ** 64 - 1, 2 ** 64 + 1, 2 ** 127, (p - 1) // 2, (p + 1) // 2,
                (2 ** 64 - 28) << 64]
        extra = (_constructed(p, lambda a, b: f128_fold_count(a, b)[0] == 4, rng)
                 + _constructed(p, lambda a, b: f128_fold_count(a, b)[1] >= p, rng))
    vals = edge + [rng.randrange(p) for _ in range(40)]
    for (a, b) in extra:
        vals += [a, b]
    assert all(0 <= v < p for v in vals)
    return vals


def expected(p, a, b):
    """(add, sub, mul, neg a, inv a) as Python integers; inv(0) = 0^(p-2) = 0."""
    return ((a + b) % p, (a - b) % p, a * b % p, (-a) % p, pow(a, p - 2, p))
