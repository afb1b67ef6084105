"""The sweep driver's calls, pinned (``compute_heavy_hitters``), on the CPU.

A recording stand-in takes the driver through the paths a real ``Mastic``
takes (the device form: GPU decide, packed candidates, device merge), which
the plaintext stand-ins of tests/test_sweep.py never reach: it is a subclass
of ``mastic_amd.vdaf.Mastic`` made without ``__init__`` whose library-backed
methods are plaintext (aggregator 0's share is the per-prefix report count and
weight sum, aggregator 1's is zero, as real ``Field64`` elements).  Every call
on it, on the merge object, the nonce set and the batch goes into one ordered
log.  ``tests/golden/sweep_calls.json`` holds, per scenario, that log and the
driver's outputs as the driver had them before it was split into frontier,
verify and fold; the test replays each scenario and compares for equality.

The fixture is recorded by this module from a checkout of that earlier driver:

    python tests/test_sweep_calls.py --record --package <checkout>/draft-mouris-cfrg-mastic_amd

(``--package`` puts that checkout's ``mastic_amd`` first on the path; without
it the tree's own package is recorded).  The recorder also asserts that the
scenarios reach what they are there for: the lazy prune, the four folds, both
compaction points, the zero-candidate levels.
"""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG_ROOT  # noqa: F401  (puts the package on sys.path)

if __name__ == "__main__" and "--package" in sys.argv:
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--package") + 1]))

from mastic_amd.field import Field64  # noqa: E402
from mastic_amd.heavy_hitters import compute_heavy_hitters, get_threshold  # noqa: E402
from mastic_amd.vdaf import Mastic, VidpfInfo  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "sweep_calls.json")
BITS = 5
CTX = b"ctx"
KEY = b"\x01\x02\x03\x04"


def index(value, length):
    return tuple((value >> (length - 1 - i)) & 1 != 0 for i in range(length))


def _show(x):
    """A call argument in a printable, JSON-able form."""
    if isinstance(x, (bytes, bytearray)):
        return bytes(x).hex()
    if isinstance(x, np.ndarray):
        return [int(v) for v in x]
    if isinstance(x, _Reports):
        return "R"
    if isinstance(x, Field64):
        return x.v
    if isinstance(x, (list, tuple)):
        if len(x) and all(isinstance(b, (bool, np.bool_)) for b in x):
            return "".join("1" if b else "0" for b in x)  # a prefix
        return [_show(v) for v in x]
    if isinstance(x, np.integer):
        return int(x)
    return x


def _decode(enc):
    """(level, prefixes) of an encoded aggregation parameter."""
    level = int.from_bytes(enc[:2], "big")
    count = int.from_bytes(enc[2:6], "big")
    plen = (level + 8) // 8
    assert len(enc) == 6 + plen * count + 1
    prefixes = []
    for i in range(count):
        b = enc[6 + plen * i: 6 + plen * (i + 1)]
        prefixes.append(tuple(bool((b[j // 8] >> (7 - j % 8)) & 1) for j in range(level + 1)))
    return (level, prefixes)


class _Reports:
    """The batch: one dict per report (nonce, alpha, weight, and how it is to
    fail).  ``n`` is read through the log, ``compact`` filters the rows."""

    def __init__(self, rows, log):
        self.rows = list(rows)
        self.log = log

    @property
    def n(self):
        self.log.append(["reports.n"])
        return len(self.rows)

    def compact(self, keep, staging_bytes=0):
        keep = np.asarray(keep)
        assert keep.shape == (len(self.rows),)
        self.log.append(["reports.compact", _show(keep.astype(np.uint8)), staging_bytes])
        self.rows = [r for (r, k) in zip(self.rows, keep) if k]
        return len(self.rows)


def _logged(name):
    """``Mastic.<name>`` itself, its outermost calls logged."""
    real = getattr(Mastic, name)

    def call(self, *args):
        if not self._depth:
            self.log.append([name] + [_show(a) for a in args])
        self._depth += 1
        try:
            return real(self, *args)
        finally:
            self._depth -= 1
    return call


class _Plain:
    """The plaintext aggregator behind both stand-ins."""
    circuit = "Count"
    field = Field64
    OUTPUT_LEN = 1
    JOINT_RAND_LEN = 0

    def setup(self, log, bits=BITS):
        self.log = log
        self.BITS = bits
        self.vidpf = VidpfInfo(Field64, bits, 2)
        self._depth = 0
        self._nodes = "seeds"
        self._dev = self._enc = None
        return self

    is_valid = _logged("is_valid")
    unshard = _logged("unshard")
    agg_init = _logged("agg_init")
    encode_agg_param = _logged("encode_agg_param")

    def _level(self):
        return int.from_bytes(self._enc[:2], "big")

    def _fails(self, row, level):
        return row["fails_from"] is not None and level >= row["fails_from"]

    def share(self, agg_id, mask=None):
        """agg_id's agg share of the last prep_init: per prefix the report
        count and the weight sum (aggregator 0), zeros (aggregator 1)."""
        rows = self._dev.rows
        keep = [True] * len(rows) if mask is None else [bool(k) for k in mask]
        assert len(keep) == len(rows)
        out = []
        for p in _decode(self._enc)[1]:
            hit = [r["weight"] for (r, k) in zip(rows, keep) if k and r["alpha"][:len(p)] == p]
            out += [Field64(len(hit) if agg_id == 0 else 0), Field64(sum(hit) if agg_id == 0 else 0)]
        return out

    def reports_upload(self, nonces, public_shares, input_shares_0=None, input_shares_1=None):
        self.log.append(["reports_upload", nonces.hex(), public_shares.hex(), input_shares_0.hex(),
                         input_shares_1.hex()])
        rows = [_row(nonces[16 * i:16 * i + 16], input_shares_0[2 * i], input_shares_0[2 * i + 1])
                for i in range(len(nonces) // 16)]
        return _Reports(rows, self.log)

    def set_frontier_cache(self, on):
        self.log.append(["set_frontier_cache", on])

    def set_frontier_cache_nodes(self, mode=None):
        self.log.append(["set_frontier_cache_nodes", mode])
        found = self._nodes
        if mode is not None:
            self._nodes = mode
        return found

    def prep_init_device(self, reports, verify_key, ctx, agg_id, agg_param):
        assert isinstance(agg_param, bytes)
        self.log.append(["prep_init_device", _show(reports), verify_key.hex(), ctx.hex(), agg_id, agg_param.hex()])
        (self._dev, self._enc) = (reports, agg_param)

    def last_prep_was_cached(self):
        self.log.append(["last_prep_was_cached"])
        return self._level() > 0

    def select_timing(self, agg_id):
        self.log.append(["select_timing", agg_id])

    def last_timing3(self):
        self.log.append(["last_timing3"])
        return (0.0, 0, 0.0, 0, 0.0, 0, 0.0)

    def aggregate_device(self, agg_id, agg_param, valid=None, raw=False):
        assert agg_param == self._enc
        self.log.append(["aggregate_device", agg_id, agg_param.hex(), _show(valid), raw])
        share = self.share(agg_id, valid)
        return Field64.encode_vec(share) if raw else share


class _DeviceMastic(_Plain, Mastic):
    """A ``Mastic`` (so the driver takes the device form) with no context."""

    def decide_results(self, ctx, n):
        self.log.append(["decide_results", ctx.hex(), n])
        rows = self._dev.rows
        assert n == len(rows)
        level = self._level()
        accept = np.array([0 if self._fails(r, level) else 1 for r in rows], np.uint8)
        return (accept, np.zeros(n, np.uint8))

    def prep_result(self, *args, **kw):
        raise AssertionError("the device form fetches no wire results")

    decide_batch = prep_result


class _WireMastic(_Plain):
    """Not a ``Mastic`` (so the driver takes the wire form), with the weight
    check's joint randomness on: ``prep_result`` returns the seeds
    ``joint_rand_confirmed`` compares and the status plane."""
    JOINT_RAND_LEN = 1
    merge = Mastic.merge
    agg_update = Mastic.agg_update
    decode_result = Mastic.decode_result
    encode_public_share = Mastic.encode_public_share
    test_vec_encode_input_share = Mastic.test_vec_encode_input_share

    def prep_result(self, reports, agg_id, agg_param):
        self.log.append(["prep_result", _show(reports), agg_id, agg_param.hex()])
        rows = self._dev.rows
        level = self._level()  # jr_bad: the helper's seed differs from the prep message at that level only
        seeds = b"".join(bytes([i ^ (0x80 if (agg_id == 1 and r["jr_bad"] == level) else 0)]) * 32
                         for (i, r) in enumerate(rows))
        status = np.array([-2 if (agg_id == 1 and r["status_bad"]) else 0 for r in rows], np.int32)
        return (b"prep%d" % agg_id, seeds, None, status)

    def decide_batch(self, ctx, agg_param, prep_shares_0, prep_shares_1):
        self.log.append(["decide_batch", ctx.hex(), agg_param.hex(), prep_shares_0.hex(), prep_shares_1.hex()])
        rows = self._dev.rows
        level = self._level()
        msgs = b"".join(bytes([i]) * 32 for i in range(len(rows)))
        return (msgs, np.array([0 if self._fails(r, level) else 1 for r in rows], np.uint8))


class _TotalMerge:
    """A one-rank device merge: ``total`` is both aggregators' shares summed."""

    def __init__(self, mastic):
        self.m = mastic

    def total(self, *args, **kwargs):
        self.m.log.append(["merge.total", _show(args), {k: _show(v) for (k, v) in sorted(kwargs.items())}])
        return self._total(*args, **kwargs)

    def _total(self, n_elems, valid=None, have_results=True):
        if n_elems == 0:
            return b""
        if not have_results:
            return bytes(8 * n_elems)
        both = [a + b for (a, b) in zip(self.m.share(0, valid), self.m.share(1, valid))]
        assert len(both) == n_elems
        return Field64.encode_vec(both)


class _LevelMerge(_TotalMerge):
    """A device merge that is told every level's candidates."""

    def begin_level(self, level, prefixes):
        self.m.log.append(["merge.begin_level", level, _show(prefixes)])


class _CallMerge:
    """A plain callable merge of one aggregator's field-object share."""

    def __init__(self, mastic):
        self.m = mastic

    def __call__(self, agg_share):
        self.m.log.append(["merge", _show(agg_share)])
        return list(agg_share)


class _NonceSet:
    def __init__(self, log):
        self.log = log
        self.seen = set()

    def admit(self, reports):
        self.log.append(["nonce_set.admit", _show(reports)])
        fresh = np.zeros(len(reports.rows), np.uint8)
        for (i, r) in enumerate(reports.rows):
            if r["nonce"] not in self.seen:
                self.seen.add(r["nonce"])
                fresh[i] = 1
        return fresh


def _row(nonce, value, weight, fails_from=None, status_bad=False, jr_bad=None):
    return {"nonce": bytes(nonce), "alpha": index(value, BITS), "weight": weight, "fails_from": fails_from,
            "status_bad": status_bad, "jr_bad": jr_bad}


def _rows():
    """24 reports: three heavy values (7, 5 and 6 copies; the first copy of
    each weighs 2) and six singletons, shuffled by a fixed permutation."""
    values = [0b10110] * 7 + [0b11011] * 5 + [0b00101] * 6 + [0b00010, 0b01100, 0b01111, 0b10001, 0b11100, 0b00111]
    rows = [_row(i.to_bytes(16, "big"), v, 2 if i in (0, 7, 12) else 1) for (i, v) in enumerate(values)]
    return [rows[(7 * i) % 24] for i in range(24)]


def _replayed_rows():
    """The 24 reports with replays of four of them mixed in; one report fails
    from level 0 and one from level 2."""
    rows = _rows()
    rows[5]["fails_from"] = 0
    rows[9]["fails_from"] = 2
    for (at, src) in ((3, 0), (11, 1), (12, 2), (27, 20)):
        rows.insert(at, dict(rows[src]))
    return rows


def _as_tuples(rows):
    """The reference's ``(nonce, public_share, input_shares)`` list; the
    leader's input share carries the measurement for ``reports_upload``."""
    return [(r["nonce"], b"", (bytes([int("".join("1" if b else "0" for b in r["alpha"]), 2), r["weight"]]), b""))
            for r in rows]


def _run(mastic_cls=_DeviceMastic, rows=None, thresholds=None, merge=None, trace=False, nonce_set=False,
         as_list=False, hook=None, catch=None, bits=BITS, **kw):
    """One sweep; returns ``{"log": ..., "out": ...}`` in JSON-able form."""
    log = []
    m = mastic_cls.__new__(mastic_cls).setup(log, bits)
    rows = _rows() if rows is None else rows
    reports = _as_tuples(rows) if (as_list or not rows) else _Reports(rows, log)
    thresholds = {"default": 4} if thresholds is None else thresholds
    tr = [] if trace else None
    for name in ("timing", "cached_levels"):
        if kw.get(name):
            kw[name] = []
    if kw.get("phase_times"):
        kw["phase_times"] = {}
    if hook is not None:
        def level_hook(level, enc, dev):
            log.append(["level_hook", level, _show(enc), _show(dev)])
            if hook == level:
                raise RuntimeError("hook")
        kw["level_hook"] = level_hook
    if "verify_key" not in kw:
        kw["verify_key"] = KEY
    hh = None
    try:
        hh = compute_heavy_hitters(m, CTX, thresholds, reports, trace=tr, merge=None if merge is None else merge(m),
                                   nonce_set=_NonceSet(log) if nonce_set else None, **kw)
    except catch or () as e:
        log.append(["raised", type(e).__name__])
    out = {
        "heavy_hitters": _show(hh),
        "trace": None if tr is None else [[t.level, _show(t.prefixes), _show(t.agg_result), t.n_valid] for t in tr],
        "cached_levels": kw.get("cached_levels"),
        "timing": None if kw.get("timing") is None else len(kw["timing"]),
        "phase_times": None if kw.get("phase_times") is None else sorted(kw["phase_times"]),
        "n": len(reports.rows) if isinstance(reports, _Reports) else None,
        "cache_nodes": m._nodes,
    }
    return json.loads(json.dumps({"log": log, "out": out}))


def _default_key_run():
    """Scenario c without a verify key: ``os.urandom(16)`` supplies it.  At a
    threshold of 6 one heavy hitter's aggregate is exactly the threshold."""
    real = os.urandom
    os.urandom = lambda n: bytes(range(0xA0, 0xA0 + n))
    try:
        return _run(verify_key=None, thresholds={"default": 6})
    finally:
        os.urandom = real


PER_PREFIX = {"default": 4, index(0b1, 1): 6, index(0b00, 2): 2}
SCENARIOS = {
    "a_wire": lambda: _run(_WireMastic, rows=[dict(r, status_bad=(i == 2), jr_bad={6: 0, 8: 1}.get(i),
                                                   fails_from=3 if i == 10 else None)
                                              for (i, r) in enumerate(_rows())],
                           thresholds=PER_PREFIX, trace=True, timing=True, phase_times=True),
    "b_trace": lambda: _run(trace=True, as_list=True),
    "c_lazy": _default_key_run,
    "d_total": lambda: _run(merge=_TotalMerge),
    "d_total_empty": lambda: _run(merge=_TotalMerge, rows=[]),
    "e_begin_level": lambda: _run(merge=_LevelMerge),
    "e_begin_level_empty": lambda: _run(merge=_LevelMerge, rows=[]),
    "f_callable": lambda: _run(merge=_CallMerge),
    "f_callable_empty": lambda: _run(merge=_CallMerge, rows=[]),
    "g_dies_lazy": lambda: _run(thresholds={"default": 12}),
    "g_dies_traced": lambda: _run(thresholds={"default": 12}, trace=True),
    "g_dies_total": lambda: _run(thresholds={"default": 12}, merge=_TotalMerge),
    "h_compact_0": lambda: _run(rows=_replayed_rows(), nonce_set=True, compact=0.0),
    "h_compact_1": lambda: _run(rows=_replayed_rows(), nonce_set=True, compact=1.0),
    "h_compact_none": lambda: _run(rows=_replayed_rows(), nonce_set=True, trace=True),
    "h_compact_all_dead": lambda: _run(rows=[dict(r, fails_from=0) for r in _rows()], compact=1.0, trace=True),
    "h_compact_refused": lambda: _run(compact=1.5, catch=ValueError),
    "i_cache": lambda: _run(frontier_cache=True, cached_levels=True, timing=True, phase_times=True, hook=-1,
                            cache_nodes="payloads"),
    "i_cache_hook_raises": lambda: _run(frontier_cache=True, cached_levels=True, hook=1, cache_nodes="payloads",
                                        catch=RuntimeError),
    "i_cache_off": lambda: _run(frontier_cache=False, cached_levels=True, thresholds={"default": 12}),
    "j_empty_lazy": lambda: _run(rows=[]),
    "j_empty_traced": lambda: _run(rows=[], trace=True),
    "j_empty_zero_threshold": lambda: _run(rows=[], thresholds={"default": 0}, bits=3),
}


def _calls(run, name):
    return [e for e in run["log"] if e[0] == name]


def _check_coverage(runs):
    """The scenarios reach what they are there for (asserted when recording)."""
    names = {name: {e[0] for e in run["log"]} for (name, run) in runs.items()}
    # wire form: wire results, the status planes and the joint-rand confirmation drop reports
    assert {"prep_result", "decide_batch", "encode_agg_param", "last_timing3"} <= names["a_wire"]
    assert [t[3] for t in runs["a_wire"]["out"]["trace"]] == [22, 22, 22, 21, 21]
    assert "reports_upload" in names["b_trace"]
    # device form: GPU decide, packed agg params (no encode_agg_param), raw folds
    for name in runs:
        if not name.startswith("a_"):
            assert not names[name] & {"prep_result", "decide_batch", "encode_agg_param"}, name
    assert all(e[4] is True for e in _calls(runs["b_trace"], "aggregate_device"))
    # lazy: no call carries prefix tuples, and the candidates still shrink and grow
    for name in ("c_lazy", "j_empty_zero_threshold", "d_total", "g_dies_lazy", "h_compact_0", "i_cache", "j_empty_lazy"):
        assert all(e[1][1] == [] for e in _calls(runs[name], "is_valid")), name
        assert not names[name] & {"agg_init", "unshard", "merge.begin_level", "merge"}, name
    counts = [int(e[5][4:12], 16) for e in _calls(runs["c_lazy"], "prep_init_device") if e[4] == 0]
    assert counts[0] == 2 and len(set(counts)) > 2 and len(counts) == BITS
    assert runs["c_lazy"]["out"]["heavy_hitters"] == runs["b_trace"]["out"]["heavy_hitters"] == \
        ["00101", "10110", "11011"]
    # an aggregate exactly at the threshold is kept: 11011 sums to 6, c's threshold
    assert [6] == [a for (p, a) in zip(*runs["b_trace"]["out"]["trace"][4][1:3]) if p == "11011"]
    # the wire form confirms the joint randomness with the weight check only: report 8's seed differs at
    # level 1 and it stays, report 6's differs at level 0 and it goes
    assert [e[2] for e in runs["a_wire"]["log"] if e[0] == "prep_result"][:1] == [0]
    assert _calls(runs["c_lazy"], "prep_init_device")[0][2] == bytes(range(0xA0, 0xB0)).hex()
    # the four folds: device merge (with and without results), raw, field objects, no-reports zeros
    # (the arguments exactly as passed: the mask positionally, have_results only to say there are none)
    assert all(len(e[1]) == 2 and len(e[1][1]) == 24 and e[2] == {} for e in _calls(runs["d_total"], "merge.total"))
    assert len(_calls(runs["d_total"], "merge.total")) == BITS
    assert [e[1:] for e in _calls(runs["d_total_empty"], "merge.total")] == [
        [[2 * n], {"have_results": False}] for n in (2, 0, 0, 0, 0)]
    assert "aggregate_device" not in names["d_total"]
    assert [e[2] for e in _calls(runs["g_dies_total"], "merge.total")] == [{}, {}] + [{"have_results": False}] * 3
    assert [e[1][0] for e in _calls(runs["g_dies_total"], "merge.total")] == [4, 4, 0, 0, 0]
    # a merge with begin_level is not lazy: it is handed the tuples, and is_valid sees them
    assert len(_calls(runs["e_begin_level"], "merge.begin_level")) == BITS
    assert all(e[2] for e in _calls(runs["e_begin_level"], "merge.begin_level"))
    assert all(e[1][1] for e in _calls(runs["e_begin_level"], "is_valid"))
    assert len(_calls(runs["f_callable"], "merge")) == 2 * BITS and "unshard" in names["f_callable"]
    assert all(e[4] is False for e in _calls(runs["f_callable"], "aggregate_device"))
    assert len(_calls(runs["j_empty_traced"], "agg_init")) == 2 * BITS
    assert names["j_empty_lazy"] == {"is_valid"}
    assert runs["j_empty_traced"]["out"]["heavy_hitters"] == []
    assert len(runs["j_empty_zero_threshold"]["out"]["heavy_hitters"]) == 2 ** 3  # zeros reach a threshold of 0
    assert {e[0] for e in runs["j_empty_zero_threshold"]["log"]} == {"is_valid"}
    # the candidates die out at level 1: two levels prepared, five levels run
    for name in ("g_dies_lazy", "g_dies_traced"):
        assert len(_calls(runs[name], "prep_init_device")) == 4 and len(_calls(runs[name], "is_valid")) == BITS
        assert runs[name]["out"]["heavy_hitters"] == []
    assert [len(t[1]) for t in runs["g_dies_traced"]["out"]["trace"]] == [2, 2, 0, 0, 0]
    # both compaction points, and no third
    log = [e[0] for e in runs["h_compact_0"]["log"]]
    at = [i for (i, x) in enumerate(log) if x == "reports.compact"]
    assert len(at) == 2 and at[0] < log.index("prep_init_device")
    first_fold = log.index("aggregate_device")
    assert first_fold < at[1] < [i for (i, x) in enumerate(log) if x == "prep_init_device"][2]
    assert runs["h_compact_0"]["out"]["n"] == 23
    for name in ("h_compact_1", "h_compact_none"):
        assert "reports.compact" not in names[name] and runs[name]["out"]["n"] == 28
    assert [t[3] for t in runs["h_compact_none"]["out"]["trace"]] == [23, 23, 22, 22, 22]
    assert runs["h_compact_all_dead"]["out"]["n"] == 0
    assert runs["h_compact_refused"]["log"] == [["raised", "ValueError"]]
    assert runs["h_compact_0"]["out"]["heavy_hitters"] == runs["h_compact_none"]["out"]["heavy_hitters"] != []
    # frontier cache: asked after aggregator 0's enqueue only; the node format is put back
    for name in ("i_cache", "i_cache_hook_raises"):
        log = runs[name]["log"]
        assert [e for e in log if e[0] == "set_frontier_cache_nodes"] == \
            [["set_frontier_cache_nodes", "payloads"], ["set_frontier_cache_nodes", "seeds"]]
        calls = [e[0] for e in log if e[0] != "raised"]
        assert calls[0] == "set_frontier_cache_nodes" and calls[-1] == "set_frontier_cache_nodes"
        assert runs[name]["out"]["cache_nodes"] == "seeds"
        for (i, e) in enumerate(log):
            if e[0] == "last_prep_was_cached":
                assert log[i - 1][0] == "prep_init_device" and log[i - 1][4] == 0
    assert runs["i_cache"]["out"]["cached_levels"] == [1, 2, 3, 4]
    assert runs["i_cache"]["out"]["timing"] == 2 * BITS
    assert runs["i_cache"]["out"]["phase_times"] == ["aggregate_merge", "decide_wait", "prep_init_enqueue",
                                                     "unshard_prune"]
    assert ["raised", "RuntimeError"] in runs["i_cache_hook_raises"]["log"]
    assert "last_prep_was_cached" not in names["i_cache_off"] and "set_frontier_cache" in names["i_cache_off"]
    for name in runs:
        if not name.startswith("i_"):
            assert "set_frontier_cache" not in names[name], name


def record():
    runs = {name: SCENARIOS[name]() for name in sorted(SCENARIOS)}
    _check_coverage(runs)
    with open(FIXTURE, "w") as f:
        f.write("{\n")
        for (k, name) in enumerate(sorted(runs)):
            f.write(" %s: {\n  \"log\": [\n" % json.dumps(name))
            f.write(",\n".join(" " + json.dumps(e, separators=(",", ":")) for e in runs[name]["log"]))
            out = json.dumps(runs[name]["out"], separators=(",", ":"), sort_keys=True)
            f.write("\n  ],\n  \"out\": %s\n }%s\n" % (out, "," if k + 1 < len(runs) else ""))
        f.write("}\n")
    print("recorded %d scenarios, %d bytes" % (len(runs), os.path.getsize(FIXTURE)))


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_scenario(recorded):
    assert sorted(recorded) == sorted(SCENARIOS)
    _check_coverage(recorded)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_sweep_makes_the_recorded_calls(recorded, name):
    got = SCENARIOS[name]()
    assert got["out"] == recorded[name]["out"]
    assert got["log"] == recorded[name]["log"]


# ---------------------------------------------------------------- the frontier
BITS9 = 9  # the packing grows a second byte at level 8
HEAVY9 = (0b101100111, 0b101100110, 0b010011000, 0b111111111)


def _sums9():
    """``sums(prefixes)``: a fixed 200-measurement workload's aggregate."""
    import random
    rng = random.Random(9)
    meas = [index(rng.choice(HEAVY9) if rng.random() < 0.7 else rng.randrange(2 ** BITS9), BITS9) for _ in range(200)]
    return lambda prefixes: [sum(a[:len(p)] == p for a in meas) for p in prefixes]


def _frontiers(thresholds, lazy=True):
    """(frontier, mastic) in each form: packings only, packings beside the
    tuples (a trace asks for them), and tuples only (the wire form)."""
    from mastic_amd.heavy_hitters import Frontier
    device = _DeviceMastic.__new__(_DeviceMastic).setup([], BITS9)
    wire = _WireMastic.__new__(_WireMastic).setup([], BITS9)
    out = {"both": (Frontier(BITS9, thresholds, True, trace=[]), device),
           "tuples": (Frontier(BITS9, thresholds, False), wire)}
    if lazy:
        out["packed"] = (Frontier(BITS9, thresholds, True), device)
    return out


def _walk(frontier, mastic, sums):
    """Take a frontier down the tree, pruning against ``sums``.  Returns every
    level's encoded aggregation parameter and the heavy hitters."""
    encs = []
    for level in range(BITS9):
        agg_param = frontier.agg_param(level)
        assert agg_param[0] == level and agg_param[2] == (level == 0)
        encs.append(frontier.encode(mastic, agg_param))
        (enc_level, prefixes) = _decode(encs[-1])
        assert enc_level == level and len(prefixes) == frontier.n_cand and encs[-1][-1] == int(level == 0)
        assert agg_param[1] == (() if frontier.lazy else tuple(prefixes))
        frontier.prune(level, sums(prefixes))
    return (encs, frontier.heavy_hitters)


def _plain_walk(thresholds, sums):
    """poc/examples.py:37-91 on plaintext sums: (every level's candidates, the heavy hitters)."""
    (levels, prefixes) = ([], [(False,), (True,)])
    for level in range(BITS9):
        levels.append(prefixes)
        kept = [p for (p, s) in zip(prefixes, sums(prefixes)) if s >= get_threshold(thresholds, p)]
        prefixes = [p + (bit,) for p in kept for bit in (False, True)]
    return (levels, kept)


def test_frontier_forms_are_decided_by_the_lazy_rule():
    from mastic_amd.heavy_hitters import Frontier
    log = []
    m = _DeviceMastic.__new__(_DeviceMastic).setup(log)
    one = {"default": 3}
    assert Frontier(BITS, one, True).lazy and Frontier(BITS, one, True, merge=_TotalMerge(m)).lazy
    for kw in ({"trace": []}, {"merge": _LevelMerge(m)}, {"merge": _CallMerge(m)}):
        f = Frontier(BITS, one, True, **kw)
        assert not f.lazy and f.prefixes == [(False,), (True,)] and f.packed == [b"\x00", b"\x80"]
    assert not Frontier(BITS, PER_PREFIX, True).lazy           # per-prefix thresholds need the tuples
    wire = Frontier(BITS, one, False)
    assert not wire.lazy and wire.packed is None and wire.n_cand == 2
    lazy = Frontier(BITS, one, True)
    assert lazy.prefixes is None and lazy.n_cand == 2 and lazy.agg_param(0) == (0, (), True)


def test_frontier_forms_give_the_same_agg_params_and_heavy_hitters():
    """The packings alone, the packings beside the tuples and the tuples
    through ``encode_agg_param`` give the same encoded aggregation parameter at
    every level and the same heavy hitters, which are the plaintext walk's."""
    sums = _sums9()
    th = {"default": 12}
    walks = {k: _walk(f, m, sums) for (k, (f, m)) in _frontiers(th).items()}
    assert walks["packed"] == walks["both"] == walks["tuples"]
    (encs, hh) = walks["packed"]
    (levels, want) = _plain_walk(th, sums)
    assert [_decode(e)[1] for e in encs] == levels
    assert hh == want and set(hh) == {index(v, BITS9) for v in HEAVY9}
    assert all(type(p) is tuple and all(type(b) is bool for b in p) for p in hh)
    assert len(encs[7]) == 7 + len(levels[7]) and len(encs[8]) == 7 + 2 * len(levels[8])  # the byte boundary
    assert any(len(a) > len(b) for (a, b) in zip(levels, levels[1:]))  # pruning drops candidates too


def test_frontier_per_prefix_thresholds_are_get_thresholds():
    """With per-prefix thresholds a candidate is kept iff its aggregate reaches
    ``get_threshold`` of it, in both tuple-holding forms."""
    sums = _sums9()
    th = {"default": 12, index(0b1011001, 7): 40, index(0b01, 2): 3, index(0b1, 1): 30}
    (levels, want) = _plain_walk(th, sums)
    assert want and want != _plain_walk({"default": 12}, sums)[1]
    for (k, (f, m)) in _frontiers(th, lazy=False).items():
        (encs, hh) = _walk(f, m, sums)
        assert [_decode(e)[1] for e in encs] == levels and hh == want, k


def test_frontier_threshold_is_of_the_longest_proper_prefix():
    """The prefix's own entry never decides, the longest listed proper prefix does."""
    from mastic_amd.heavy_hitters import Frontier
    th = {"default": 5, index(0b0, 1): 2, index(0b01, 2): 9, index(0b1, 1): 7}
    f = Frontier(BITS9, th, True)
    f.prune(0, [5, 4])              # the default decides: (0,)'s own 2 and (1,)'s own 7 do not
    assert f.prefixes == [index(0b00, 2), index(0b01, 2)]
    f.prune(1, [2, 8])              # (0,)'s 2 for both; (0, 1)'s own 9 not yet
    assert f.prefixes == [index(v, 3) for v in (0b000, 0b001, 0b010, 0b011)]
    f.prune(2, [1, 2, 8, 9])        # 000 and 001 under (0,): 2; 010 and 011 under (0, 1): 9
    assert f.prefixes == [index(v, 4) for v in (0b0010, 0b0011, 0b0110, 0b0111)]
    assert f.packed == [bytes([v << 4]) for v in (0b0010, 0b0011, 0b0110, 0b0111)]


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_sweep_calls.py --record [--package DIR]")
    record()
