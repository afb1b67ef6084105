"""A plain reference of the XOF layer, written from the specifications
(FIPS 202 for Keccak-p, RFC 9861 for TurboSHAKE128, draft-irtf-cfrg-vdaf-13
section 6.2 for next_vec), not from the device code: the round constants come
from the LFSR and the rotation offsets from the (x, y) walk of FIPS 202, the
sponge works on bytes.  tests/test_xof_ref.py pins it against
oracle._prims.turboshake128 and oracle.xof before a GPU test trusts it.

States are numpy ``uint64`` arrays of shape (lanes, 25), word x + 5 y at
column x + 5 y, vectorised over lanes so that the GPU tests' host side stays
short.  A word's bytes are little-endian, so the rate is the first 21 words.

AES needs no reference here: oracle._prims.aes128_expand, aes128_encrypt and
fixed_key_aes_blocks are it.  fixed_key_aes_blocks(rk, seed, first_ctr, n)
takes first_ctr as an unsigned 64-bit integer and XORs le64(first_ctr + b)
into seed bytes 0..7 (bytes 8..15 are never touched), so every 32-bit counter
the device code takes (it XORs ctr into seed word 0) is in its range.
"""
import numpy as np

RATE = 168
RATE_WORDS = 21
_CHUNK = 4096  # lanes per permutation call: the working set stays in cache


def _round_constants():
    def rc_bit(t):
        r = 1
        for _ in range(t % 255):
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        return r & 1

    out = []
    for ir in range(24):
        rc = 0
        for j in range(7):
            if rc_bit(j + 7 * ir):
                rc |= 1 << ((1 << j) - 1)
        out.append(rc)
    return out[12:]  # Keccak-p[1600, 12]: the last 12 rounds of Keccak-f


def _rho_offsets():
    r = [0] * 25
    (x, y) = (1, 0)
    for t in range(24):
        r[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        (x, y) = (y, (2 * x + 3 * y) % 5)
    return r


RC12 = _round_constants()
RHO = _rho_offsets()
_RHO_L = np.array(RHO, np.uint64)[:, None]
_RHO_R = np.array([63 - r for r in RHO], np.uint64)[:, None]
# pi: B[y + 5 ((2x + 3y) % 5)] = A[x + 5y]
_PI_DST = np.array([y + 5 * ((2 * x + 3 * y) % 5) for y in range(5) for x in range(5)])
_ONE = np.uint64(1)
_63 = np.uint64(63)


def _perm_cols(a):
    """a: (25, n), one state per column"""
    n = a.shape[1]
    for rc in RC12:
        a5 = a.reshape(5, 5, n)  # [y][x]
        c = a5[0] ^ a5[1] ^ a5[2] ^ a5[3] ^ a5[4]
        c1 = np.roll(c, -1, axis=0)  # C[x + 1]
        d = np.roll(c, 1, axis=0) ^ ((c1 << _ONE) | (c1 >> _63))
        a = (a5 ^ d[None]).reshape(25, n)
        rot = (a << _RHO_L) | ((a >> _RHO_R) >> _ONE)  # a right shift by 64 - r, also for r = 0
        b = np.empty_like(rot)
        b[_PI_DST] = rot
        b5 = b.reshape(5, 5, n)
        a = (b5 ^ (~np.roll(b5, -1, axis=1) & np.roll(b5, -2, axis=1))).reshape(25, n)
        a[0] ^= np.uint64(rc)
    return a


def keccak_p12(states):
    """Keccak-p[1600, 12] of every row of states (lanes, 25); returns a new array."""
    states = np.ascontiguousarray(states, np.uint64)
    out = np.empty_like(states)
    for i in range(0, len(states), _CHUNK):
        out[i:i + _CHUNK] = _perm_cols(np.ascontiguousarray(states[i:i + _CHUNK].T)).T
    return out


def absorb(states, f, data, nbytes=None):
    """Absorb bytes at fill position f, permuting at each full block.

    states (lanes, 25); data (lanes, maxlen) uint8; f and nbytes are ints or
    per-lane arrays (lane i absorbs data[i, :nbytes[i]] at position f[i]).
    Returns (new states, new fill positions), the latter per lane.
    """
    states = np.array(states, np.uint64)
    n = len(states)
    data = np.asarray(data, np.uint8).reshape(n, -1)
    f = np.broadcast_to(np.asarray(f, np.int64), (n,))
    nbytes = np.broadcast_to(np.asarray(data.shape[1] if nbytes is None else nbytes, np.int64), (n,))
    assert ((0 <= f) & (f < RATE)).all() and (nbytes <= data.shape[1]).all()
    end = f + nbytes
    nblk = int((end.max() + RATE - 1) // RATE) if n else 0
    buf = np.zeros((n, max(nblk, 1) * RATE), np.uint8)
    (rows, cols) = np.nonzero(np.arange(data.shape[1])[None, :] < nbytes[:, None])
    buf[rows, cols + f[rows]] = data[rows, cols]
    for k in range(nblk):
        touched = np.nonzero(end > k * RATE)[0]
        blk = np.ascontiguousarray(buf[touched, k * RATE:(k + 1) * RATE]).view("<u8")
        states[touched, :RATE_WORDS] ^= blk
        full = np.nonzero(end >= (k + 1) * RATE)[0]
        states[full] = keccak_p12(states[full])
    return (states, end % RATE)


def pad(states, f, domain):
    """TurboSHAKE pad: the domain byte at f, 0x80 into byte 167, permute."""
    states = np.array(states, np.uint64)
    n = len(states)
    f = np.broadcast_to(np.asarray(f, np.int64), (n,))
    states[np.arange(n), f // 8] ^= np.uint64(domain) << (8 * (f % 8)).astype(np.uint64)
    states[:, RATE_WORDS - 1] ^= np.uint64(0x80 << 56)
    return keccak_p12(states)


def squeeze(states, nbytes):
    """nbytes of output per lane from padded states (which stay as they are): (lanes, nbytes) uint8."""
    states = np.array(states, np.uint64)
    out = []
    got = 0
    while True:
        out.append(np.ascontiguousarray(states[:, :RATE_WORDS]).view(np.uint8))
        got += RATE
        if got >= nbytes:
            break
        states = keccak_p12(states)
    return np.concatenate(out, axis=1)[:, :nbytes]


def turboshake128(msg: bytes, domain: int, out_len: int) -> bytes:
    st = np.zeros((1, 25), np.uint64)
    (st, f) = absorb(st, 0, np.frombuffer(msg, np.uint8).reshape(1, -1))
    return squeeze(pad(st, f, domain), out_len)[0].tobytes()


def next_vec(stream: bytes, modulus: int, enc: int, count: int):
    """Xof.next_vec over a byte stream: enc little-endian bytes per candidate,
    candidates >= modulus skipped.  Returns (values, indices of the rejected
    candidates among those read); IndexError if the stream runs out."""
    vals = []
    rejected = []
    i = 0
    while len(vals) < count:
        if (i + 1) * enc > len(stream):
            raise IndexError("stream too short")
        x = int.from_bytes(stream[i * enc:(i + 1) * enc], "little")
        if x < modulus:
            vals.append(x)
        else:
            rejected.append(i)
        i += 1
    return (vals, rejected)


def next_vec_from_states(states, modulus: int, enc: int, count: int):
    """next_vec of every lane's squeezed stream; states are padded states
    (their rate words are the stream's first block).  Per lane (values, rejected)."""
    nblk = (count * enc + RATE - 1) // RATE + 1
    while True:
        streams = squeeze(states, nblk * RATE)
        try:
            return [next_vec(streams[i].tobytes(), modulus, enc, count) for i in range(len(streams))]
        except IndexError:
            nblk += 2
