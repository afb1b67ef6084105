"""The FLP shape grid and the honest and dishonest encodings shared by
tests/test_oracle_flp_grid.py (CPU), tests/test_gpu_flp_ops.py and
tests/test_gpu_flp_shapes.py.

A shape is (circuit, kwargs) with the keyword names of mastic_amd.Mastic:
max_measurement (Sum: the largest weight; MultihotCountVec: max_weight),
length, sum_vec_bits, chunk_length.  Encodings are lists of Python integers
in [0, p).  Each grid line names what it reaches that the other suites do not.
"""
from oracle import flp as oflp
from oracle.field import Field64, Field128

GRID = [
    ("Sum", dict(max_measurement=1)),                      # wbits 1, P 4
    ("Sum", dict(max_measurement=2)),                      # max = 2^k: largest offset; calls 4 -> P 8
    ("Sum", dict(max_measurement=4)),                      # calls 6 -> P 8
    ("Sum", dict(max_measurement=2047)),                   # 24 query rands: second sponge block
    ("Sum", dict(max_measurement=2 ** 32)),                # truncation group of 33 bits; P 128
    ("Sum", dict(max_measurement=2 ** 63 - 1)),            # wbits 63, offset 0; VALUE_LEN 127
    ("Sum", dict(max_measurement=2 ** 62 + 12345)),        # wbits 63, huge offset
    ("SumVec", dict(length=1, sum_vec_bits=1, chunk_length=1)),    # smallest; P 2 with ParallelSum
    ("SumVec", dict(length=1, sum_vec_bits=63, chunk_length=1)),   # 63-bit group; 63 joint rands
    ("SumVec", dict(length=2, sum_vec_bits=33, chunk_length=5)),   # group crossing chunks; padded last chunk
    ("SumVec", dict(length=3, sum_vec_bits=5, chunk_length=64)),   # chunk > meas_len: one call, arity 128
    ("SumVec", dict(length=11, sum_vec_bits=1, chunk_length=1)),   # 11 joint rands: element 10 straddles the rate
    ("SumVec", dict(length=16, sum_vec_bits=2, chunk_length=2)),   # calls exactly 2^k: P doubles
    ("Histogram", dict(length=1, chunk_length=1)),
    ("Histogram", dict(length=2, chunk_length=1)),
    ("Histogram", dict(length=15, chunk_length=1)),        # calls 2^k - 1
    ("Histogram", dict(length=16, chunk_length=1)),        # calls 2^k
    ("Histogram", dict(length=5, chunk_length=9)),         # chunk > length
    ("Histogram", dict(length=33, chunk_length=3)),        # calls 11
    ("MultihotCountVec", dict(length=1, max_measurement=1, chunk_length=1)),   # smallest
    ("MultihotCountVec", dict(length=5, max_measurement=5, chunk_length=3)),   # max_weight == length, offset 2
    ("MultihotCountVec", dict(length=9, max_measurement=4, chunk_length=2)),   # offset 3; count bits over chunks
    ("MultihotCountVec", dict(length=6, max_measurement=1, chunk_length=7)),   # chunk > meas_len
    ("MultihotCountVec", dict(length=12, max_measurement=8, chunk_length=4)),  # max = 2^k: offset 7
]
COUNT = ("Count", dict())

CIRCUIT_IDS = {"Count": 1, "Sum": 2, "SumVec": 3, "Histogram": 4, "MultihotCountVec": 5}


def shape_id(shape):
    (circuit, kw) = shape
    return circuit + "".join("-%d" % kw[k] for k in ("length", "sum_vec_bits", "max_measurement", "chunk_length")
                             if k in kw)


def oracle_valid(shape):
    """The oracle's validity circuit of a shape."""
    (circuit, kw) = shape
    if circuit == "Count":
        return oflp.Count(Field64)
    if circuit == "Sum":
        return oflp.Sum(Field64, kw["max_measurement"])
    if circuit == "SumVec":
        return oflp.SumVec(Field128, kw["length"], kw["sum_vec_bits"], kw["chunk_length"])
    if circuit == "Histogram":
        return oflp.Histogram(Field128, kw["length"], kw["chunk_length"])
    return oflp.MultihotCountVec(Field128, kw["length"], kw["max_measurement"], kw["chunk_length"])


def _bits(x, n):
    assert 0 <= x < 2 ** n
    return [(x >> i) & 1 for i in range(n)]


def boundary_measurements(shape):
    """The measurements at the edges of a shape's range: 0, the maximum, all
    ones, first and last bucket, weight 0 and max_weight."""
    (circuit, kw) = shape
    if circuit == "Count":
        return [0, 1]
    if circuit == "Sum":
        mx = kw["max_measurement"]
        out = [0, mx, 1, 2 ** (mx.bit_length() - 1) - 1, 2 ** (mx.bit_length() - 1)]
        return list(dict.fromkeys(out))
    if circuit == "SumVec":
        (n, top) = (kw["length"], 2 ** kw["sum_vec_bits"] - 1)
        out = [[0] * n, [top] * n, [top] + [0] * (n - 1), [0] * (n - 1) + [top]]
        return [list(x) for x in dict.fromkeys(tuple(x) for x in out)]
    if circuit == "Histogram":
        return list(dict.fromkeys([0, kw["length"] - 1]))
    (n, w) = (kw["length"], kw["max_measurement"])
    out = [[False] * n, [True] * w + [False] * (n - w), [False] * (n - w) + [True] * w]
    return [list(x) for x in dict.fromkeys(tuple(x) for x in out)]


def random_measurement(shape, rng):
    (circuit, kw) = shape
    if circuit == "Count":
        return rng.randrange(2)
    if circuit == "Sum":
        return rng.randrange(kw["max_measurement"] + 1)
    if circuit == "SumVec":
        return [rng.randrange(2 ** kw["sum_vec_bits"]) for _ in range(kw["length"])]
    if circuit == "Histogram":
        return rng.randrange(kw["length"])
    k = rng.randrange(min(kw["max_measurement"], kw["length"]) + 1)
    idx = set(rng.sample(range(kw["length"]), k))
    return [i in idx for i in range(kw["length"])]


def encode(shape, measurement):
    return [x.int() for x in oracle_valid(shape).encode(measurement)]


def dishonest_encodings(shape):
    """[(name, encoded)]: encodings no honest client produces, at the first and
    at the last position that the circuit treats differently."""
    (circuit, kw) = shape
    p = oracle_valid(shape).field.MODULUS
    out = []

    def put(name, enc):
        out.append((name, [x % p for x in enc]))

    def with_at(enc, i, x):
        enc = list(enc)
        enc[i] = x
        return enc

    if circuit == "Count":
        put("2", [2])
        put("p-1", [p - 1])
    elif circuit == "Sum":
        mx = kw["max_measurement"]
        b = mx.bit_length()
        off = 2 ** b - 1 - mx
        v = mx // 2
        good = _bits(v, b) + _bits(v + off, b)
        for i in sorted({0, b - 1}):
            put("lo[%d]=2" % i, with_at(good, i, 2))
            put("lo[%d]=p-1" % i, with_at(good, i, p - 1))
            put("hi[%d]=2" % i, with_at(good, b + i, 2))
            put("hi[%d]=p-1" % i, with_at(good, b + i, p - 1))
            # lo and hi are bit strings, but hi is not lo + offset
            put("hi[%d] flipped" % i, with_at(good, b + i, 1 - good[b + i]))
            put("lo[%d] flipped" % i, with_at(good, i, 1 - good[i]))
        if off > 0:
            # max + 1 fits the low half; max + 1 + offset = 2^b does not fit the high half
            put("max+1, hi wrapped", _bits(mx + 1, b) + _bits(0, b))
            put("max+1, hi of max", _bits(mx + 1, b) + _bits(2 ** b - 1, b))
    elif circuit == "SumVec":
        (n, sb) = (kw["length"], kw["sum_vec_bits"])
        good = [(i * 5 + 1) % 2 for i in range(n * sb)]
        for i in sorted({0, n * sb - 1}):
            put("[%d]=2" % i, with_at(good, i, 2))
            put("[%d]=p-1" % i, with_at(good, i, p - 1))
    elif circuit == "Histogram":
        n = kw["length"]
        put("zero-hot", [0] * n)
        if n >= 2:
            put("two-hot", with_at(with_at([0] * n, 0, 1), n - 1, 1))
            put("2 and p-1", with_at(with_at([0] * n, 0, 2), n - 1, p - 1))
            put("p-1 and 2", with_at(with_at([0] * n, 0, p - 1), n - 1, 2))
            put("all ones", [1] * n)
        else:
            put("2", [2])
            put("p-1", [p - 1])
    else:
        (n, mw) = (kw["length"], kw["max_measurement"])
        b = mw.bit_length()
        off = 2 ** b - 1 - mw

        def vec(w, first=True):
            return [1] * w + [0] * (n - w) if first else [0] * (n - w) + [1] * w
        if n > mw:
            # weight max_weight + 1: offset + weight = 2^b wraps to 0; or the count of max_weight
            put("weight max+1, count wrapped", vec(mw + 1) + _bits(0, b))
            put("weight max+1, count of max", vec(mw + 1, False) + _bits(2 ** b - 1, b))
        w = min(2, mw, n - 1)
        put("weight %d claimed %d" % (w + 1, w), vec(w + 1) + _bits(off + w, b))
        put("weight %d claimed %d, last" % (w + 1, w), vec(w + 1, False) + _bits(off + w, b))
        good = vec(min(1, mw)) + _bits(off + min(1, mw), b)
        for i in sorted({0, n - 1}):
            put("vec[%d]=2" % i, with_at(good, i, 2))
            put("vec[%d]=p-1" % i, with_at(good, i, p - 1))
        for i in sorted({0, b - 1}):
            put("count[%d]=2" % i, with_at(good, n + i, 2))
            put("count[%d]=p-1" % i, with_at(good, n + i, p - 1))
    return out
