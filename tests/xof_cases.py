"""The case lists of tests/test_gpu_xof_ops.py, kept apart from it so that
tests/test_xof_ref.py can hold them to their intended classes on the CPU:
every edge class is counted (the census) and must be non-empty, and the
reference must reject exactly the candidates a squeeze case plans."""
import random

import numpy as np

RATE = 168
F64_P = 2 ** 64 - 2 ** 32 + 1
F128_P = 2 ** 128 - 7 * 2 ** 66 + 1
FIELDS = {64: (F64_P, 8, 21), 128: (F128_P, 16, 10)}  # modulus, ENCODED_SIZE, whole candidates in block 0
LANES = 70  # one full wave and a partly filled one

# ---------------------------------------------------------------- B: one-lane sponge
SPONGE_PREFIX_LENS = list(range(0, 171))
SPONGE_FIXED = [1, 2, 3, 4, 5, 8, 16, 18, 32, 64, 72, 336]
SPONGE_ENDS = [167, 168, 169, 335, 336, 337]


def sponge_cfgs():
    """[(prefix length, body bytes)]"""
    out = []
    for L in SPONGE_PREFIX_LENS:
        f = L % RATE
        lens = list(SPONGE_FIXED)
        for end in SPONGE_ENDS:
            if end - f > 0 and end - f not in lens:
                lens.append(end - f)
        out += [(L, nb) for nb in lens]
    return out


def sponge_census(cfgs):
    c = {"fill positions": len({L % RATE for (L, _) in cfgs}),
         "prefix crosses a block": sum(1 for (L, _) in cfgs if L > RATE),
         "prefix fills a block exactly": sum(1 for (L, _) in cfgs if L == RATE)}
    for end in SPONGE_ENDS:
        c["f + nbytes == %d" % end] = sum(1 for (L, nb) in cfgs if L % RATE + nb == end)
    for nb in SPONGE_FIXED:
        c["nbytes == %d" % nb] = sum(1 for (_, n) in cfgs if n == nb)
    return c


# ---------------------------------------------------------------- C: next_vec from chosen states
class SqueezeCase:
    def __init__(self, name, cands, plan):
        (self.name, self.cands, self.plan) = (name, cands, frozenset(plan))

    def planned_rejections(self, count, k):
        """rejections the plan causes while `count` elements are taken (block 0's k candidates only)"""
        (acc, rej) = (0, 0)
        for i in range(k):
            if acc == count:
                break
            if i in self.plan:
                rej += 1
            else:
                acc += 1
        return rej


def squeeze_counts(bits):
    return [1, 20, 21, 22, 42, 43] if bits == 64 else [1, 10, 11, 12, 21, 22]


def squeeze_cases(bits, seed=1):
    """Block 0's candidates of every lane, chosen.  Returns the cases in lane
    order, shuffled so that every wave mixes lanes with 0, 1 and many rejections."""
    (p, enc, k) = FIELDS[bits]
    top = 1 << (8 * enc)
    rng = random.Random(1000 * bits + seed)
    if bits == 64:
        kept = [("p-1", p - 1), ("0xffffffff00000000", 0xffffffff00000000)]
        bad = [("p", p), ("p+1", p + 1), ("2^64-1", top - 1)]
    else:
        kept = [("p-1", p - 1), ("hi=..e3 lo=2^64-1", (0xffffffffffffffe3 << 64) | (2 ** 64 - 1))]
        bad = [("p", p), ("hi=..e5 lo=0", 0xffffffffffffffe5 << 64), ("2^128-1", top - 1)]
    assert all(v < p for (_, v) in kept) and all(p <= v < top for (_, v) in bad)
    pool = [v for (_, v) in bad]

    def ok():
        return rng.getrandbits(8 * enc - 1)  # top bit clear: below p

    def no():
        return rng.choice(pool + [rng.randrange(p, top)])

    def run(name, plan):
        return SqueezeCase(name, [no() if i in plan else ok() for i in range(k)], plan)

    cases = [run("no rejection", ())]
    cases += [run("candidate %d rejected" % i, (i,)) for i in range(k)]
    cases += [run("first %d rejected" % j, range(j)) for j in range(1, k + 1)]
    cases += [run("even candidates rejected", range(0, k, 2)), run("odd candidates rejected", range(1, k, 2))]
    for at in (0, k - 1):
        for (name, v) in kept + bad:
            c = run("%s at candidate %d" % (name, at), ())
            c.cands[at] = v
            if v >= p:
                c.plan = frozenset((at,))
            cases.append(c)
    while len(cases) < LANES:
        cases.append(run("no rejection (filler %d)" % len(cases), ()))
    rng.shuffle(cases)
    # the partly filled second wave gets one lane of each kind too
    for (slot, kind) in ((64, 0), (65, 1), (66, 2)):
        j = next(i for i in range(64) if min(len(cases[i].plan), 2) == kind)
        (cases[slot], cases[j]) = (cases[j], cases[slot])
    return cases


def squeeze_states(bits, cases, seed=1):
    """(lanes, 25) uint64: the rate words hold the cases' candidates, the rest is random."""
    (_, enc, k) = FIELDS[bits]
    rng = np.random.default_rng(77 * bits + seed)
    st = rng.integers(0, 2 ** 64, size=(len(cases), 25), dtype=np.uint64)
    for (i, c) in enumerate(cases):
        raw = b"".join(v.to_bytes(enc, "little") for v in c.cands)
        st[i, :len(raw) // 8] = np.frombuffer(raw, "<u8")
    return st


def squeeze_census(bits, cases):
    (p, _, k) = FIELDS[bits]
    c = {"lanes": len(cases),
         "no rejection": sum(1 for x in cases if not x.plan),
         "one rejection": sum(1 for x in cases if len(x.plan) == 1),
         "many rejections": sum(1 for x in cases if len(x.plan) > 1),
         "whole block rejected": sum(1 for x in cases if len(x.plan) == k),
         "p-1 kept": sum(1 for x in cases if p - 1 in x.cands),
         "p rejected": sum(1 for x in cases if p in x.cands)}
    for i in range(k):
        c["candidate %d alone" % i] = sum(1 for x in cases if x.plan == frozenset((i,)))
        c["first %d" % (i + 1)] = sum(1 for x in cases if x.plan == frozenset(range(i + 1)))
    for w in range((len(cases) + 63) // 64):
        lanes = cases[64 * w:64 * w + 64]
        c["wave %d mixes 0 / 1 / many" % w] = min(sum(1 for x in lanes if not x.plan),
                                                  sum(1 for x in lanes if len(x.plan) == 1),
                                                  sum(1 for x in lanes if len(x.plan) > 1))
    return c


# ---------------------------------------------------------------- D: node proofs
NP_PREFIX_LENS = list(range(0, 168))
NP_PATH_BYTES = [1, 2, 3, 4, 5, 8, 16, 31, 32]


def node_proof_cfgs():
    """[(prefix length = f, path_bytes)]"""
    return [(L, pb) for L in NP_PREFIX_LENS for pb in NP_PATH_BYTES]


def node_proof_census(cfgs):
    c = {"q values": len({f >> 2 for (f, _) in cfgs}), "shifts": len({f & 3 for (f, _) in cfgs})}
    for pb in (1, 32):
        ends = [f + 20 + pb for (f, b) in cfgs if b == pb]
        c["path %d: f + nbytes == 167" % pb] = sum(1 for e in ends if e == 167)
        c["path %d: f + nbytes == 168" % pb] = sum(1 for e in ends if e == 168)
        c["path %d: f + nbytes > 168" % pb] = sum(1 for e in ends if e > 168)
        c["path %d: f + nbytes < 167" % pb] = sum(1 for e in ends if e < 167)
    return c


# ---------------------------------------------------------------- E: k_absorb, k_absorb_pair
AB_N = 70
AB_STRIDE = 128
AB_FIXED = [4, 32, 164, 168, 172, 336, 340, 508, 676]


def absorb_flip_lengths(f):
    """nbytes at which the second block's in-range test flips: k_absorb takes
    the plain loads when base + 42 < nw, k_absorb_pair when base + 43 < nw."""
    base = 42 - (f >> 2) - (1 if f & 3 else 0)
    return [4 * (base + d) for d in (42, 43, 44)]


def absorb_items(fs=range(RATE)):
    """[(f, nbytes)], nbytes multiples of 4"""
    out = []
    for f in fs:
        lens = AB_FIXED + [nb for nb in absorb_flip_lengths(f) if nb not in AB_FIXED]
        out += [(f, nb) for nb in lens]
    return out


AB_PLANE_FS = [4 * q + sh for q in (0, 20, 41) for sh in range(4)]
AB_CHAINS = [(0, 4, 4), (1, 164, 168), (3, 168, 4), (5, 340, 336), (42, 128, 212), (83, 84, 84), (120, 48, 676),
             (121, 508, 172), (166, 4, 336), (167, 4, 164), (167, 172, 172), (2, 336, 340)]


def absorb_launches(items):
    """One launch covers both sponges with different (f, nbytes): consecutive
    items.  Case records of xof_ops_absorb (f0, nb0, f1, nb1, prio, reset,
    tot0, tot1, skip0, skip1); the priority alternates between 3 and 0."""
    if len(items) % 2:
        items = items + [items[0]]
    out = []
    for j in range(0, len(items), 2):
        ((f0, n0), (f1, n1)) = (items[j], items[j + 1])
        out.append((f0, n0, f1, n1, 3 if (j // 2) % 2 == 0 else 0, 1, n0 // 4, n1 // 4, 0, 0))
    return out


def absorb_chain_launches():
    """Per pair of chains three launches: the first piece, the second piece
    continuing it at f2 = (f + nbytes1) % 168, and the concatenation alone."""
    out = []
    for j in range(0, len(AB_CHAINS), 2):
        ((fa, a1, a2), (fb, b1, b2)) = (AB_CHAINS[j], AB_CHAINS[j + 1])
        (ta, tb) = ((a1 + a2) // 4, (b1 + b2) // 4)
        out.append((fa, a1, fb, b1, 3, 1, ta, tb, 0, 0))
        out.append(((fa + a1) % RATE, a2, (fb + b1) % RATE, b2, 3, 0, ta, tb, a1 // 4, b1 // 4))
        out.append((fa, a1 + a2, fb, b1 + b2, 3, 1, ta, tb, 0, 0))
    return out


def absorb_census(items):
    c = {"fill positions": len({f for (f, _) in items})}
    for nb in AB_FIXED:
        c["nbytes == %d" % nb] = sum(1 for (_, n) in items if n == nb)
    for d in (42, 43, 44):
        c["second block: nw - base == %d" % d] = sum(
            1 for (f, n) in items if n // 4 - (42 - (f >> 2) - (1 if f & 3 else 0)) == d)
    c["ends on a block boundary"] = sum(1 for (f, n) in items if (f + n) % RATE == 0)
    c["three or more blocks"] = sum(1 for (f, n) in items if f + n >= 3 * RATE)
    return c


# ---------------------------------------------------------------- F: fixed-key AES
AES_CTRS = [0, 1, 2, 0xfe, 0xff, 0x100, 0x101, 0x1ff, 0x200, 0xffff, 0x10000, 0xffffff00, 0xffffffff]
# (kind, hi_a, hi_b, c_a, c_b) of xof_ops_aes
AES_GROUP_OPS = (
    [(0, c & ~0xff, 0, c, 0) for c in AES_CTRS] +
    [(0, 0x1a5, 0, 0x100, 0), (0, 0x1a5, 0, 0x1ff, 0), (0, 0xabcdefff, 0, 0xabcdef00, 0),
     (0, 0xabcdefff, 0, 0xabcdef7f, 0),                       # ctr_hi with low bits set: masked
     (1, 0, 0, 0, 1), (1, 0x1a5, 0, 0x1fe, 0x101),            # two blocks of one group
     (1, 0, 0, 0x00, 0xff),                                   # counters 0x00 and 0xff of one group
     (2, 0, 0, 0, 0), (2, 0, 0, 1, 2), (2, 0x100, 0x100, 0x100, 0x101), (2, 0, 0x200, 0xff, 0x200),
     (0, 0, 0, 5, 0), (3, 0, 0, 0xfe, 0), (0, 0x100, 0, 0x107, 0), (3, 0, 0, 0x1ff, 0),  # re-initialised at 0x100
     (4, 0, 0x100, 0xfe, 0x101), (4, 0xffffff00, 0, 0xffffffff, 0)])                # ctr_blocks_n<4>: c, c ^ 1
