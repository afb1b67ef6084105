"""Table of the level kernels' register, scratch and occupancy figures from
the remarks of a build with -Rpass-analysis=kernel-resource-usage:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Iinclude \
        -Rpass-analysis=kernel-resource-usage -o /tmp/lib.so \
        draft-mouris-cfrg-mastic_amd/csrc/mastic_hip.hip 2> remarks.txt
    python3 tools/kernel_resources.py before=old_remarks.txt after=remarks.txt

One row per k_eval_aes / k_eval_aes_wide instantiation and labelled file; with
two files the script also says which rows differ."""
import re
import sys

KEYS = ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill")


def demangle(name):
    """_Z10k_eval_aesI3F64Lb1ELb1ELb0EE... -> k_eval_aes<F64, GEN=1, FC=1, SPLIT=0, PAY=0>
    (a build from before the PAY parameter: PAY=0, so the rows pair up)"""
    m = re.match(r"_Z\d+(k_eval_aes(?:_wide)?)I(\d+)(F\d+)((?:Lb[01]E)+)E", name)
    if not m:
        return name
    names = ("GEN", "SPLIT") if m.group(1).endswith("wide") else ("GEN", "FC", "SPLIT", "PAY")
    flags = (re.findall(r"Lb([01])E", m.group(4)) + ["0"] * len(names))[:len(names)]
    return "%s<%s, %s>" % (m.group(1), m.group(3), ", ".join("%s=%s" % nf for nf in zip(names, flags)))


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1) if "k_eval_aes" in m.group(1) else None
            if cur:
                cur = demangle(cur)
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur and m.group(1) in KEYS:
            out[cur][m.group(1)] = m.group(2)
    return out


def main():
    tables = [(a.split("=", 1)[0], parse(a.split("=", 1)[1])) for a in sys.argv[1:]]
    names = sorted({n for (_l, t) in tables for n in t})
    print("%-54s %-7s %s" % ("kernel", "build", "  ".join(KEYS)))
    for n in names:
        rows = [(label, t.get(n, {})) for (label, t) in tables]
        for (label, r) in rows:
            print("%-54s %-7s %s" % (n, label, "  ".join("%*s" % (len(k), r.get(k, "-")) for k in KEYS)))
        if len(rows) == 2:
            diff = [k for k in KEYS if rows[0][1].get(k) != rows[1][1].get(k)]
            verdict = "identical" if not diff else "differs: " + ", ".join(diff)
            if not rows[0][1] or not rows[1][1]:
                verdict = "only in " + (rows[1][0] if rows[1][1] else rows[0][0])
            print("%-54s %-7s %s" % ("", "", verdict))
    print("%d instantiations" % len(names))


if __name__ == "__main__":
    main()
