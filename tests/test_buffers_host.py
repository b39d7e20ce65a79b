"""The owning buffer of vqvdb_amd/csrc/vq_buffers.h on the host: tests/host/buffers_check.cpp instantiates the core template with a
malloc / free policy that counts live blocks and can fail the k-th allocation, is built with AddressSanitizer and
UndefinedBehaviorSanitizer by the host compiler, and is run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "buffers_check.cpp")
HEADER = os.path.join(ROOT, "vqvdb_amd", "csrc", "vq_buffers.h")
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
            return
        errors.append(f"{cxx}:\n{r.stderr[-2000:]}")
    pytest.fail("no host compiler built tests/host/buffers_check.cpp with -fsanitize=address,undefined\n" + "\n".join(errors))


def test_core_template_includes_nothing_of_hip():
    core = open(HEADER).read().split("#ifdef __HIPCC__")[0]
    assert "class Buffer" in core and "hip" not in core.split("#pragma once")[1].lower()


def test_buffer_contract_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "buffers_check")
    _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("buffers ok:") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
