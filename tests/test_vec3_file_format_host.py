"""The .vqv3 reader / writer core of vqvdb_amd/csrc/vq_vec3_file_format.h on the host: tests/host/vec3_file_check.cpp
writes a two-grid file of each kind and reads it back, then feeds the parser every refusal case (damaged fields, wrong lengths, a
truncation at every section boundary, counts of 2^32 - 1 leaves in a file of 100 bytes).  The program includes that header alone, is
built with AddressSanitizer and UndefinedBehaviorSanitizer by the host compiler, and is run as a program of its own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "vec3_file_check.cpp")
HEADER = os.path.join(ROOT, "vqvdb_amd", "csrc", "vq_vec3_file_format.h")
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
    pytest.fail("no host compiler built tests/host/vec3_file_check.cpp with -fsanitize=address,undefined\n" + "\n".join(errors))


def test_format_header_includes_nothing_of_hip():
    text = open(HEADER).read()
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, flags=re.M)
    assert includes and not [i for i in includes if "hip" in i.lower() or i.startswith("vq")], includes
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__device__|__host__|__HIPCC__", code)
    check = open(SRC).read()
    assert re.findall(r'#include\s+"([^"]+)"', check) == ["../../vqvdb_amd/csrc/vq_vec3_file_format.h"]


def test_reader_and_writer_core_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "vec3_file_check")
    _build(exe)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("vec3 file ok:") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the files the program wrote are the numpy restatement's too
    from vqvdb_amd import vqvdbfile
    for name, kind in (("two_grids_active.vqv3", 1), ("two_grids_indices.vqv3", 0)):
        data = (work / name).read_bytes()
        header, grids = vqvdbfile.read_vec3(data)
        assert header["kind"] == kind and [g["name"] for g in grids] == ["velocity", "", "n" * 300]
        assert [len(g["origins"]) for g in grids] == [37, 0, 11]
        assert vqvdbfile.dumps_vec3(header, grids) == data
