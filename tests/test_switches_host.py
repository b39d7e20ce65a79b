"""The kernel-switch table and parser of vqvdb_amd/csrc/vq_switches.h on the host: tests/host/switches_check.cpp parses a fake
environment (defaults, every legal value, typos, malformed and out-of-range integers), is built with AddressSanitizer and
UndefinedBehaviorSanitizer by the host compiler and run as a program of its own; the table it prints is the one in INTEGRATION.md,
its "covered by" entries name tests that exist, and the library reads no VQHIP_* variable that the table does not hold."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "switches_check.cpp")
CSRC = os.path.join(ROOT, "vqvdb_amd", "csrc")
HEADER = os.path.join(CSRC, "vq_switches.h")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
BEGIN, END = "<!-- switches:begin (printed by tests/host/switches_check.cpp table) -->\n", "<!-- switches:end -->\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++ first, with the sanitizer runtimes linked statically so that the program stands alone; a compiler without them fails at
    the link, then ROCm's clang++ (which links them statically anyway) has a try."""
    out = str(tmp_path_factory.mktemp("switches") / "switches_check")
    errors = []
    for cxx, extra in (("g++", ["-static-libasan", "-static-libubsan"]), ("g++", []), ("/opt/rocm/llvm/bin/clang++", []),
                       ("/opt/rocm/lib/llvm/bin/clang++", [])):
        path = shutil.which(cxx)
        if not path:
            continue
        r = subprocess.run([path, *FLAGS, *extra, SRC, "-o", out], capture_output=True, text=True)
        if r.returncode == 0:
            return out
        errors.append(f"{cxx}:\n{r.stderr[-2000:]}")
    pytest.fail("no host compiler built tests/host/switches_check.cpp with -fsanitize=address,undefined\n" + "\n".join(errors))


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return r.stdout


def _rows(table):
    """[(name, values, selects, covered by)] of the Markdown table"""
    rows = [[c.strip() for c in re.split(r"(?<!\\)\|", line)[1:-1]] for line in table.splitlines()[2:]]
    assert rows and all(len(r) == 4 for r in rows), rows
    return [(r[0].strip("`"), r[1], r[2], r[3].strip("`")) for r in rows]


def test_header_includes_nothing_of_hip():
    text = open(HEADER).read()
    assert "struct Switches" in text and "parse_switches" in text
    assert not [line for line in text.splitlines() if line.startswith("#include") and "hip/" in line]
    assert "__HIPCC__" not in text and "hipStream" not in text


def test_parser_against_a_fake_environment_under_asan_and_ubsan(exe):
    assert _run(exe).startswith("switches ok:")


def test_integration_table_is_the_one_the_array_prints(exe):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert doc.count(BEGIN) == 1 and doc.count(END) == 1
    assert doc.split(BEGIN)[1].split(END)[0] == _run(exe, "table")


def test_covered_by_names_tests_that_exist(exe):
    rows = _rows(_run(exe, "table"))
    assert sum(1 for r in rows if r[3]) >= 15   # the table is not allowed to go blank
    for name, _, _, covered in rows:
        if not covered:
            continue
        path, func = covered.split("::")
        assert path.startswith("tests/") and os.path.isfile(os.path.join(ROOT, path)), (name, covered)
        assert re.search(rf"^def {re.escape(func)}\(", open(os.path.join(ROOT, path)).read(), re.M), (name, covered)


def test_the_library_reads_no_switch_outside_the_table(exe):
    """Every "VQHIP_..." string literal in the library's sources is a name handed to getenv or to the table's lookup; their set is
    the table's.  And getenv itself stands in two places: the lookup given to parse_switches and copy_threads_cap()."""
    table = {r[0] for r in _rows(_run(exe, "table"))}
    literals, getenvs = set(), []
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        literals |= set(re.findall(r'"(VQHIP_[A-Z0-9_]+)"', text))
        code = "\n".join(line.split("//")[0] for line in text.splitlines())
        getenvs += [f] * len(re.findall(r"\bgetenv\s*\(", code))
    assert literals == table, (sorted(literals - table), sorted(table - literals))
    assert getenvs == ["vq_runtime.hip", "vq_runtime.hip"], getenvs
