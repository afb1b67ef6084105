"""bench.py's plain / --full split and --dump-outputs.

On CPU: a plain run switches every leg besides the timed steps off and
--full leaves each leg's own switch as given; field elements are written as
32-bit limbs (exact in float64); an output over its share of the 64 MB budget
is cut to the same seeded sample of rows in every run.

On the GPU: one small plain run with --dump-outputs prints a line without the
legs that moved behind --full, runs exactly --steps timed steps, and writes
the agg share and prep shares that the library computes for the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
MOVED_KEYS = ("full_job", "cpu_baseline", "cpu_parity", "north_star")


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_plain_run_switches_the_other_legs_off():
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, "")
    assert (a.standalone, a.cpu_baseline, a.north_star, a.full_job) == (0, 0, 0, 0)
    # a leg's own switch does not bring it back without --full
    a = bench.parse(["--cpu-baseline", "1", "--north-star", "1", "--full-job", "1", "--standalone", "1"])
    assert (a.standalone, a.cpu_baseline, a.north_star, a.full_job) == (0, 0, 0, 0)
    a = bench.parse(["--full"])
    assert (a.standalone, a.cpu_baseline, a.north_star, a.full_job) == (1, 1, 1, -1)
    a = bench.parse(["--full", "--cpu-baseline", "0", "--standalone", "0", "--dump-outputs", "d"])
    assert (a.standalone, a.cpu_baseline, a.north_star, a.dump_outputs) == (0, 0, 1, "d")


def test_limbs_are_exact():
    bench = _bench()
    vals = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 53 + 1, 2 ** 64 - 2 ** 32]  # the last: Field64's p - 1
    raw = b"".join(v.to_bytes(8, "little") for v in vals)
    a = bench.limbs(raw, 8)
    assert a.dtype == np.float64 and a.shape == (len(vals), 2)
    assert [int(lo) + (int(hi) << 32) for (lo, hi) in a] == vals
    v128 = 2 ** 128 - 7 * 2 ** 66
    b = bench.limbs(v128.to_bytes(16, "little"), 16)
    assert b.shape == (1, 4) and sum(int(x) << (32 * i) for (i, x) in enumerate(b[0])) == v128


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)  # 2000 bytes per array below
    big = np.arange(300 * 4, dtype=np.float32).reshape(300, 4)  # 4800 bytes: cut to 125 rows
    small = np.arange(10, dtype=np.float64).reshape(5, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    got = np.load(tmp_path / "a" / "big.npy")
    assert got.dtype == np.float32 and got.shape == (125, 4)
    assert (np.diff(got[:, 0]) > 0).all() and (got == big[(got[:, 0] // 4).astype(int)]).all()  # rows of big, in order
    assert (got == np.load(tmp_path / "b" / "big.npy")).all()
    assert (np.load(tmp_path / "a" / "small.npy") == small).all()
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4000 + 2 * 128  # the budget plus the two .npy headers


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    (n, n_pre, steps) = (192, 24, 3)
    out = str(tmp_path / "dump")
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--reports", str(n),
           "--total-reports", str(2 * n), "--prefixes", str(n_pre), "--dump-outputs", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == steps and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "report*prefix/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert abs(d["value"] - n * n_pre / (d["ms_per_step"] / 1e3)) <= 1e-6 * d["value"]
    assert not [k for k in MOVED_KEYS if k in d] and d["roofline_absorb"]["standalone"] is None

    # the same inputs through the library: step 3 of 3 walks slice (3 - 1) % 2 = 0 of the resident reports
    bench = _bench()
    from mastic_amd import Mastic
    cfg = bench.CONFIGS["c2"]
    m = Mastic(32, "Sum", max_measurement=255)
    (attrs, alpha_b, betas, nonces, rands) = bench.synth(m, cfg, 0, 2 * n, n_pre, 0x4D41 + 2)
    vk = np.random.default_rng(0x4D41).integers(0, 256, size=32, dtype=np.uint8).tobytes()
    ctx = b"mastic-mi355x-bench"
    enc_ap = bench.agg_param_bytes(31, attrs)
    reps = m.reports_shard(ctx, alpha_b, betas, nonces, rands).view(0, n)
    m.prep_init_device(reps, vk, ctx, 0, enc_ap)
    agg = m.aggregate_device(0, enc_ap, raw=True)
    (ps, js, _o, st) = m.prep_result(reps, 0, enc_ap)

    got = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["agg_share", "joint_rand_seeds", "prep_shares", "prep_status"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["agg_share"].shape == (len(attrs) * (1 + m.OUTPUT_LEN), 2)
    assert (got["agg_share"] == bench.limbs(agg, 8)).all() and got["agg_share"].any()
    assert got["prep_shares"].shape == (n, m.prep_share_size(True))
    assert got["prep_shares"].astype(np.uint8).tobytes() == ps
    assert got["joint_rand_seeds"].astype(np.uint8).tobytes() == js
    assert (got["prep_status"][:, 0] == st).all() and not st.any()
