"""The device headers of csrc/ stand alone: a translation unit that consists of
one `#include "H"` compiles for gfx950 (syntax only, no GPU), so a test
library or a tool can include the one subsystem it needs.  kernels.hpp stays an
index (comments and includes only), and no source file but the level kernel's
grows past 1,300 lines."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "draft-mouris-cfrg-mastic_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
LEVEL_KERNEL = "level_kernel.hpp"
MAX_LINES = 1300
HEADERS = [
    "planes.hpp", "unpack_kernels.hpp", "conv_stream.hpp", "node_proof.hpp", LEVEL_KERNEL, "absorb_kernels.hpp",
    "finish_kernels.hpp", "fold_kernels.hpp", "decide_kernels.hpp",
    "kernels.hpp", "shard.hpp", "rows_kernels.hpp", "nonce_set_kernels.hpp", "aes.hpp", "keccak.hpp", "flp.hpp",
    "field.hpp",
]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc in PATH")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    tu = tmp_path / "tu.hip"
    tu.write_text('#include "%s"\n' % header)
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, "-I", INCLUDE,
                        str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_kernels_hpp_is_an_index():
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for word in ("__global__", "MH_D", "struct"):
        assert not re.search(r"\b%s\b" % word, code), word
    for line in code.splitlines():
        assert not line.strip() or line.startswith("#pragma once") or line.startswith("#include "), line


def test_source_files_stay_navigable():
    for name in sorted(os.listdir(CSRC)):
        if name == LEVEL_KERNEL:
            continue
        with open(os.path.join(CSRC, name)) as f:
            lines = sum(1 for _ in f)
        assert lines <= MAX_LINES, (name, lines)
