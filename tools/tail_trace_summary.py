"""Summarise a rocprofv3 --kernel-trace CSV of bench.py (C2 / C4 / C5 steps):
  python3 tools/tail_trace_summary.py <run_kernel_trace.csv> [--timeline N]
per-kernel launch counts and summed time, then per prep_init call (one
k_finalize each) the step's serial tail: the end of the last binder-sponge
launch minus the end of the last level-kernel launch, and the summed
level-kernel time of the call.  --timeline N also lists the last call's last N
launches before k_finalize, times in ms relative to the last level kernel's end.
"""
import collections
import csv
import sys


def short(name):
    return name.split("(")[0].replace("void ", "")


def main():
    path = sys.argv[1]
    nline = int(sys.argv[sys.argv.index("--timeline") + 1]) if "--timeline" in sys.argv else 0
    rows = [(short(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
            for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: r[1])
    by = collections.defaultdict(lambda: [0, 0])
    for (n, s, e) in rows:
        by[n][0] += 1
        by[n][1] += e - s
    print("trace %s" % path)
    for (n, (cnt, ns)) in sorted(by.items(), key=lambda kv: -kv[1][1])[:10]:
        print("  %-70s n=%5d total_ms=%10.3f" % (n, cnt, ns / 1e6))
    tails, level_ms, proof_ms = [], [], []
    prev = 0
    last = None
    for (i, (n, s, e)) in enumerate(rows):
        if not n.startswith("k_finalize"):
            continue
        call = [r for r in rows[prev:i]]
        prev = i + 1
        lv = [r for r in call if r[0].startswith("k_eval_aes")]
        sp = [r for r in call if r[0].startswith("k_absorb")]
        if not lv or not sp:
            continue
        lv_end = max(r[2] for r in lv)
        tails.append((max(r[2] for r in sp) - lv_end) / 1e6)
        level_ms.append(sum(r[2] - r[1] for r in lv) / 1e6)
        proof_ms.append(sum(r[2] - r[1] for r in call if r[0].startswith("k_node_proof")) / 1e6)
        last = (call, lv_end)
    print("  last sponge end - last level kernel end per call (ms): %s" % ["%.2f" % t for t in tails])
    print("  level kernels per call (ms): %s" % ["%.1f" % t for t in level_ms])
    print("  k_node_proof per call (ms): %s" % ["%.1f" % t for t in proof_ms])
    if nline and last:
        (call, t0) = last
        print("  last call, last %d launches (start, end in ms after the last level kernel's end):" % nline)
        for (n, s, e) in call[-nline:]:
            print("    %-44s %9.2f %9.2f" % (n[:44], (s - t0) / 1e6, (e - t0) / 1e6))


if __name__ == "__main__":
    main()
