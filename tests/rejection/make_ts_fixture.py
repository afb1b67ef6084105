"""TEST INFRASTRUCTURE — generates tests/golden/ts_rejection_f64.json
(committed; re-run only to regenerate):

    python tests/rejection/make_ts_fixture.py [--prove-rand]

rejection_f64.json covers the fixed-key-AES convert stream only.  The
TurboSHAKE next_vec sampler (query rand, helper proof share, joint rand,
prove rand) rejects a Field64 candidate once per 2^32 elements, which no
reference vector and no random test reaches.  This script brute-forces
(find_ts_rejection.c, the oracle's own Keccak) for MasticSum(4, 1023)
(QUERY_RAND_LEN 22 = one gadget + 2*10 + 1 circuit outputs, PROOF_LEN 64):
  * query_rand: a nonce whose query-rand stream (verify key, level fixed) has
    a candidate >= p among its first 22;
  * query_rand_full_block: the same for MasticSum(4, 2^20 - 1), whose
    QUERY_RAND_LEN 42 is exactly two 168-byte squeeze blocks (a Sum circuit's
    2*bits + 2 is a multiple of 21 first at 20 bits), so the 42nd element
    comes from a third squeeze block that no other report needs;
  * proof_share: a 32-byte helper seed whose proof-share stream has a
    candidate >= p among its first 64;
  * prove_rand (--prove-rand; ~2^32 trials, 3.3e9 and six minutes on eight
    cores for the committed one): a prove-rand seed whose stream's first
    PROVE_RAND_LEN = 1 candidate is >= p.
The fixture holds only what the search found; the tests recompute every
expected output with the oracle.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import mastic as om  # noqa: E402
from oracle.common import to_le_bytes  # noqa: E402
from oracle.dst import USAGE_PROOF_SHARE, USAGE_PROVE_RAND, USAGE_QUERY_RAND, dst_alg  # noqa: E402

CTX = b"mastic ts rejection"
VERIFY_KEY = bytes(range(0x20, 0x40))
LEVEL = 1
BITS, MAX_MEASUREMENT, MAX_MEASUREMENT_FULL = 4, 1023, 2 ** 20 - 1
SALT = bytes.fromhex("91a7c3e5f1d2b4068899aabbccddeeff0123456789abcdef")  # the bytes after the counter


def search(exe, msg, off, count):
    t0 = time.time()
    out = subprocess.check_output([exe, msg.hex(), str(off), str(count), str(os.cpu_count() or 1)]).decode().split()
    (ctr, cand, scanned) = map(int, out)
    print("  counter %d candidate %d, %d counters scanned, %.1f s" % (ctr, cand, scanned, time.time() - t0), flush=True)
    return ctr.to_bytes(8, "little"), cand, ctr + 1  # trials: the counters up to the hit (the same on every run)


def candidates(o, seed, dst, binder, count):
    xof = o.xof(seed, dst, binder)
    return [int.from_bytes(xof.next(8), "little") for _ in range(count)]


def main():
    o = om.MasticSum(BITS, MAX_MEASUREMENT)
    assert o.flp.QUERY_RAND_LEN == 22 and o.flp.PROOF_LEN == 64
    o2 = om.MasticSum(BITS, MAX_MEASUREMENT_FULL)
    assert o2.flp.QUERY_RAND_LEN == 42  # 42 * 8 bytes = two squeeze blocks exactly
    exe = os.path.join(tempfile.mkdtemp(), "find_ts_rejection")
    subprocess.check_call(["gcc", "-O3", "-march=native", "-pthread", "-o", exe,
                           os.path.join(HERE, "find_ts_rejection.c")])
    p = o.field.MODULUS
    findings = {}

    print("query_rand", flush=True)
    d = dst_alg(CTX, USAGE_QUERY_RAND, o.ID)
    head = to_le_bytes(len(d), 2) + d + to_le_bytes(len(VERIFY_KEY), 1) + VERIFY_KEY
    nonce_tail = SALT[:8]
    (ctr, cand, trials) = search(exe, head + bytes(8) + nonce_tail + to_le_bytes(LEVEL, 2), len(head),
                                 o.flp.QUERY_RAND_LEN)
    nonce = ctr + nonce_tail
    assert candidates(o, VERIFY_KEY, d, nonce + to_le_bytes(LEVEL, 2), cand + 1)[cand] >= p
    findings["query_rand"] = dict(stream="query_rand", max_measurement=MAX_MEASUREMENT, nonce=nonce.hex(),
                                  candidate=cand, trials=trials)

    print("query_rand_full_block", flush=True)
    nonce_tail = SALT[8:16]  # the algorithm id is the same, so only the nonce tail separates the two searches
    (ctr, cand, trials) = search(exe, head + bytes(8) + nonce_tail + to_le_bytes(LEVEL, 2), len(head),
                                 o2.flp.QUERY_RAND_LEN)
    nonce = ctr + nonce_tail
    assert candidates(o2, VERIFY_KEY, d, nonce + to_le_bytes(LEVEL, 2), cand + 1)[cand] >= p
    findings["query_rand_full_block"] = dict(stream="query_rand", max_measurement=MAX_MEASUREMENT_FULL,
                                             nonce=nonce.hex(), candidate=cand, trials=trials)

    print("proof_share", flush=True)
    d = dst_alg(CTX, USAGE_PROOF_SHARE, o.ID)
    head = to_le_bytes(len(d), 2) + d + to_le_bytes(32, 1)
    (ctr, cand, trials) = search(exe, head + bytes(8) + SALT, len(head), o.flp.PROOF_LEN)
    seed = ctr + SALT
    assert candidates(o, seed, d, b"", cand + 1)[cand] >= p
    findings["proof_share"] = dict(stream="proof_share", max_measurement=MAX_MEASUREMENT,
                                   helper_seed=seed.hex(), candidate=cand, trials=trials)

    if "--prove-rand" in sys.argv[1:]:
        print("prove_rand", flush=True)
        d = dst_alg(CTX, USAGE_PROVE_RAND, o.ID)
        head = to_le_bytes(len(d), 2) + d + to_le_bytes(32, 1)
        (ctr, cand, trials) = search(exe, head + bytes(8) + SALT, len(head), o.flp.PROVE_RAND_LEN)
        seed = ctr + SALT
        assert candidates(o, seed, d, b"", cand + 1)[cand] >= p
        findings["prove_rand"] = dict(stream="prove_rand", max_measurement=MAX_MEASUREMENT,
                                  prove_rand_seed=seed.hex(), candidate=cand, trials=trials)

    fx = dict(comment="generated by tests/rejection/make_ts_fixture.py (search results only; see its docstring)",
              circuit="MasticSum", bits=BITS, ctx=CTX.hex(),
              verify_key=VERIFY_KEY.hex(), level=LEVEL, findings=findings)
    with open(os.path.join(ROOT, "tests", "golden", "ts_rejection_f64.json"), "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
