#!/usr/bin/env python3
"""Compare the device code of two builds function by function.

    tools/codeobj_diff.py A B

A and B are gfx950 code objects, or host libraries that embed one (their
.hip_fatbin section is unbundled first, the recipe of
profiles/r11_v1_knob_retirement.txt part A).  Whole-section hashes are printed
for information only: the order in which the host code first names a kernel
reorders .text without changing any function.  What counts, and what the exit
status reports (0 = equal), is
  * the same set of function symbols (llvm-objdump -d, split at "<symbol>:");
  * identical disassembly of every function (addresses and raw encodings are
    not part of the text compared);
  * for every kernel the same resources in the code object's metadata note:
    VGPR / SGPR / AGPR counts, spill counts, private and group segment sizes,
    kernarg size, workgroup size limit.
Needs ROCm's LLVM tools (llvm-objdump, llvm-objcopy, llvm-readelf,
clang-offload-bundler) in PATH or under $ROCM_PATH/llvm/bin (/opt/rocm).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RESOURCES = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count",
             "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size",
             "max_flat_workgroup_size", "wavefront_size")


def tool(name):
    d = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    return d if os.path.exists(d) else name


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(path, tmp, tag):
    """path itself, or the gfx950 code object unbundled from its .hip_fatbin."""
    if ".hip_fatbin" not in run(tool("llvm-readelf"), "--section-headers", path):
        return path
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    run(tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path, os.devnull)
    run(tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET,
        "--output=" + co)
    return co


def functions(co):
    """{symbol: sha256 of its disassembly text}"""
    out, name, body = {}, None, []
    text = run(tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
    for line in text.splitlines() + ["<end>:"]:
        m = re.match(r"^<(.+)>:$", line)
        if m:
            if name is not None:
                out[name] = hashlib.sha256("\n".join(body).encode()).hexdigest()
            name, body = m.group(1), []
        elif name is not None and line.strip():
            body.append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def kernels(co):
    """{kernel name: {resource: value}} from the amdhsa.kernels metadata note."""
    out, cur = {}, None
    for line in run(tool("llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)  # a kernel-level key (arguments sit deeper)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == "name":
            out[m.group(3)] = cur
        elif m.group(2) in RESOURCES:
            cur[m.group(2)] = m.group(3)
    return out


def sections(co, tmp, tag):
    res = {}
    for s in (".text", ".rodata", ".note"):
        f = os.path.join(tmp, tag + s)
        run(tool("llvm-objcopy"), "--dump-section", s + "=" + f, co, os.devnull)
        data = open(f, "rb").read()
        res[s] = (len(data), hashlib.sha256(data).hexdigest())
    return res


def main(a, b):
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        ca, cb = code_object(a, tmp, "a"), code_object(b, tmp, "b")
        fa, fb = functions(ca), functions(cb)
        ka, kb = kernels(ca), kernels(cb)
        for s, (la, ha) in sections(ca, tmp, "a").items():
            lb, hb = sections(cb, tmp, "b")[s]
            print("section %-8s A %#x bytes %s  B %#x bytes %s  %s (information only)"
                  % (s, la, ha, lb, hb, "equal" if (la, ha) == (lb, hb) else "DIFFERENT"))
        nsym = [len(re.findall(r"\bFUNC\b", run(tool("llvm-readelf"), "--symbols", c))) for c in (ca, cb)]
        print("FUNC symbols: A %d, B %d" % tuple(nsym))
    for name in sorted(set(fa) ^ set(fb)):
        print("only in %s: %s" % ("A" if name in fa else "B", name))
        bad += 1
    for name in sorted(set(fa) & set(fb)):
        if fa[name] != fb[name]:
            print("body differs: %s" % name)
            bad += 1
    for name in sorted(set(ka) ^ set(kb)):
        print("kernel metadata only in %s: %s" % ("A" if name in ka else "B", name))
        bad += 1
    for name in sorted(set(ka) & set(kb)):
        for r in RESOURCES:
            if ka[name].get(r) != kb[name].get(r):
                print("metadata differs: %s %s: A %s, B %s" % (name, r, ka[name].get(r), kb[name].get(r)))
                bad += 1
    print("functions: A %d, B %d; kernels with metadata: A %d, B %d; differences: %d"
          % (len(fa), len(fb), len(ka), len(kb), bad))
    return 1 if bad or nsym[0] != nsym[1] else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
