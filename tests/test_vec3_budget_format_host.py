"""The host arithmetic of vqvdb_amd/csrc/vq_vec3_budget_format.h as a program of its own: tests/host/vec3_budget_check.cpp
runs the pick and the .vqv3 file size over the cases of tests/test_vec3_budget_host.py, over 2^32 - 1 leaves with 6144 payload bytes
each, and over sums that would pass 2^63 - 1, which must be refused.  The program includes that header alone, is built with
AddressSanitizer and UndefinedBehaviorSanitizer by the host compiler, and is run as a program of its own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "vec3_budget_check.cpp")
HEADER = os.path.join(ROOT, "vqvdb_amd", "csrc", "vq_vec3_budget_format.h")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(exe):
    """g++ first, with the sanitizer runtimes linked statically so that the program stands alone; a compiler without them fails at
    the link, then ROCm's clang++ (which links them statically anyway) has a try."""
    errors = []
    for cxx, extra in (("g++", ["-static-libasan", "-static-libubsan"]), ("g++", []), ("/opt/rocm/llvm/bin/clang++", []),
                       ("/opt/rocm/lib/llvm/bin/clang++", [])):
        path = shutil.which(cxx)
        if not path:
            continue
        r = subprocess.run([path, *FLAGS, *extra, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            assert "warning" not in r.stderr, r.stderr
            return
        errors.append(f"{cxx}:\n{r.stderr[-2000:]}")
    pytest.fail("no host compiler built tests/host/vec3_budget_check.cpp with -fsanitize=address,undefined\n" + "\n".join(errors))


def test_budget_header_includes_nothing_of_hip():
    text = open(HEADER).read()
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, flags=re.M)
    assert "vq_vec3_file_format.h" in includes                       # the layout it computes the size from, itself free of HIP
    assert not [i for i in includes if "hip" in i.lower() or (i.startswith("vq") and i != "vq_vec3_file_format.h")], includes
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__device__|__host__|__HIPCC__", code)
    check = open(SRC).read()
    assert re.findall(r'#include\s+"([^"]+)"', check) == ["../../vqvdb_amd/csrc/vq_vec3_budget_format.h"]


def test_pick_and_file_size_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "vec3_budget_check")
    _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("vec3 budget ok:") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(re.search(r"ok: (\d+) checks", r.stdout).group(1)) > 150
