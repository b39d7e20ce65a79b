"""Size sweep of the Vec3 handle without a GPU: the C ABI of include/vqvdb_hip_vec3_rate.h (declarations, exports,
bindings, NULL handle), the payload helper and the choice of a rung within a budget against the numpy restatement
tests/torch_ref_vec3_rate.py, a fixture that fills every column of a histogram row, and the wrapper's argument checks."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3_rate as t3t  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import codec  # noqa: E402

HEADER = os.path.join(ROOT, "include", "vqvdb_hip_vec3_rate.h")
NAMES = ["vqhip_vec3_rate_payload_bytes", "vqhip_vec3_rate_sweep_device", "vqhip_vec3_rate_sweep", "vqhip_vec3_rate_compress", "vqhip_vec3_rate_pick"]
ARITY = dict(zip(NAMES, (1, 9, 6, 13, 4)))
F = np.float32


def test_header_library_and_bindings_hold_exactly_the_vec3_rate_names():
    assert codec.VEC3_RATE_SYMBOLS == NAMES
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(NAMES)
    assert all(n.startswith("vqhip_vec3_rate_") for n in NAMES)
    assert re.search(r"#define\s+VQHIP_VEC3_RATE_MAX_TOLS\s+64\b", text) and re.search(r"#define\s+VQHIP_VEC3_RATE_CLASSES\s+51\b", text)
    assert (codec.VEC3_RATE_MAX_TOLS, codec.VEC3_RATE_CLASSES) == (64, 51) and (t3t.CLASSES, t3t.RAW_COL, t3t.KEPT_COL) == (51, 49, 50)
    assert re.search(r'#include\s+"vqvdb_hip_vec3_residual.h"', text)
    for name in NAMES:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert params.count(",") + 1 == ARITY[name], name
    others = [v for k, v in vars(codec).items() if k.endswith("_SYMBOLS") and k != "VEC3_RATE_SYMBOLS"]
    assert len(others) >= 9 and codec.RATE_SYMBOLS in others and codec.VEC3_RESIDUAL_SYMBOLS in others
    for other in others:
        assert not set(NAMES) & set(other)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h == "vqvdb_hip_vec3_rate.h":
            continue
        assert "vqhip_vec3_rate_" not in open(os.path.join(ROOT, "include", h)).read(), h
    lib = codec.load_library()
    for name in NAMES:
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == ARITY[name], name
        assert f.restype == (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int), name
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_\w+)\b", out))
    assert {n for n in exported if n.startswith("vqhip_vec3_rate_")} == set(NAMES)


def test_a_null_handle_is_refused_and_the_payload_helper_needs_no_device():
    lib = codec.load_library()
    tols, hist = np.array([0.5], F), np.zeros((1, 51), np.int64)
    used, nbytes = ctypes.c_float(0), ctypes.c_int64(0)
    assert lib.vqhip_vec3_rate_sweep_device(None, None, None, None, 1, tols.ctypes.data, 1, None, None) == -1
    assert lib.vqhip_vec3_rate_sweep(None, None, 1, tols.ctypes.data, 1, hist.ctypes.data) == -1
    assert lib.vqhip_vec3_rate_compress(None, None, 1, tols.ctypes.data, 1, 0, ctypes.byref(used), None, None, None, None, None, ctypes.byref(nbytes)) == -1
    row = np.zeros(51, np.int64)
    assert codec.vec3_rate_payload_bytes(row) == 0 == t3t.payload_bytes(row)
    row[:] = np.arange(1, 52)
    want = sum(64 * s * (s + 1) for s in range(49)) + 6144 * 50
    assert codec.vec3_rate_payload_bytes(row) == want == t3t.payload_bytes(row)
    row[50] = 10 ** 12                                               # kept leaves cost nothing
    assert codec.vec3_rate_payload_bytes(row) == want == t3t.payload_bytes(row)
    big = np.zeros(51, np.int64)
    big[49] = 1 << 32                                                # 2^32 raw leaves: the sums are 64-bit
    assert codec.vec3_rate_payload_bytes(big) == 6144 << 32 == t3t.payload_bytes(big)
    big[49], big[48] = 0, 1 << 32
    assert codec.vec3_rate_payload_bytes(big) == 3072 << 32 == t3t.payload_bytes(big)
    assert lib.vqhip_vec3_rate_payload_bytes(None) == -1
    for bad in (np.zeros(50, np.int64), np.zeros(19, np.int64), np.zeros(51, np.float64), np.zeros((2, 51), np.int64)):
        with pytest.raises(ValueError, match="51 integers"):
            codec.vec3_rate_payload_bytes(bad)


def test_every_column_of_a_row_and_the_helper_against_the_classes():
    tol = 0.5
    x, recon, err = t3t.every_column_leaves(tol)
    n = len(x)
    assert n == 52
    code, off = t3r.classify(x, recon, err, tol)
    for s in range(49):                                              # the widths the fixture promises, leaf by leaf
        assert t3r.widths(code[s]).tolist() == [min(s, 16), min(max(s - 16, 0), 16), max(s - 32, 0)], s
    assert code[49] == t3r.RAW and code[50] == t3r.RAW and code[51] == t3r.KEPT
    assert np.array_equal(t3t.columns(code), codec.HipVec3Codec.rate_columns(code))
    assert codec.HipVec3Codec.rate_columns(np.array([0, 16 | 16 << 5 | 16 << 10, 3 | 5 << 10, 0xFFFF, 0xFFFE], np.uint16)).tolist() == [0, 48, 8, 49, 50]
    tols = [tol, 0.0, float("nan"), float("inf"), 0.25, 1.0, 1e-3, -1.0]
    hist = t3t.sweep(x, recon, err, tols)
    assert hist.shape == (len(tols), 51) and hist.dtype == np.int64 and (hist.sum(axis=1) == n).all()
    assert (hist[0] >= 1).all() and hist[0, :49].tolist() == [1] * 49 and hist[0, 49] == 2 and hist[0, 50] == 1, hist[0]
    assert hist[1, 49] == n and hist[2, 49] == n and hist[7, 49] == n    # tol 0, NaN and a negative tol: every leaf raw
    assert hist[3, 50] == n - int(np.isnan(err[:, 0]).sum()) == n - 1 and hist[3, 49] == 1   # +inf keeps every leaf with a finite error
    for t, v in enumerate(tols):
        c, o = t3r.classify(x, recon, err, v)
        assert codec.vec3_rate_payload_bytes(hist[t]) == t3t.payload_bytes(hist[t]) == o[-1] == len(t3r.pack(x, recon, v, c)), v
        assert np.array_equal(hist[t], np.bincount(codec.HipVec3Codec.rate_columns(c), minlength=51)), v
    assert t3t.payload_bytes(hist[0]) == 64 * sum(range(49)) + 2 * 6144


def test_pick_takes_the_smallest_fitting_value_not_the_first_fitting_index():
    def row(raw, s8):
        r = np.zeros(51, np.int64)
        r[49], r[8], r[50] = raw, s8, 100 - raw - s8
        return r

    lib = codec.load_library()
    # sizes 6144 * raw + 512 * s8: not monotone in the tolerance (the rung 0.2 escapes to raw leaves)
    tols = np.array([0.4, np.nan, 0.1, 0.2, 0.3, 0.3], F)
    hist = np.ascontiguousarray(np.stack([row(0, 2), row(0, 0), row(0, 40), row(30, 10), row(0, 8), row(0, 8)]))
    assert [t3t.payload_bytes(r) for r in hist] == [1024, 0, 20480, 184320 + 5120, 4096, 4096]

    def c_pick(budget, h=hist, v=tols):
        return lib.vqhip_vec3_rate_pick(h.ctypes.data, v.ctypes.data, len(v), budget)

    for budget, want in ((5000, 4), (21000, 2), (1024, 0), (10 ** 12, 2), (4096, 4), (4095, 0)):
        assert t3t.pick(hist, tols, budget) == want == c_pick(budget) == codec.vec3_rate_pick(hist, tols, budget), budget
    assert tols[t3t.pick(hist, tols, 21000)] == F(0.1)               # 0.1 fits although the larger 0.2 does not
    for budget in (1023, 0):                                         # only the NaN rung's 0 bytes would fit: never chosen
        with pytest.raises(ValueError, match=f"no rung fits {budget} bytes"):
            t3t.pick(hist, tols, budget)
        with pytest.raises(ValueError, match=f"no rung fits {budget} bytes"):
            codec.vec3_rate_pick(hist, tols, budget)
        assert c_pick(budget) == -1
    with pytest.raises(ValueError):
        t3t.pick(hist[1:2], tols[1:2], 10 ** 9)
    assert c_pick(10 ** 9, np.ascontiguousarray(hist[1:2]), tols[1:2].copy()) == -1
    rung = np.array([np.inf, 0.0], F)                                # +inf and 0 are rungs like any other
    two = np.ascontiguousarray(np.stack([row(0, 0), row(100, 0)]))
    assert c_pick(614400, two, rung) == 1 == t3t.pick(two, rung, 614400) and c_pick(614399, two, rung) == 0 == t3t.pick(two, rung, 614399)
    # invalid arguments of the C function: -1, nothing is read
    assert lib.vqhip_vec3_rate_pick(None, tols.ctypes.data, 6, 5000) == -1 and lib.vqhip_vec3_rate_pick(hist.ctypes.data, None, 6, 5000) == -1
    assert lib.vqhip_vec3_rate_pick(hist.ctypes.data, tols.ctypes.data, 0, 5000) == -1
    assert lib.vqhip_vec3_rate_pick(hist.ctypes.data, tols.ctypes.data, 65, 5000) == -1
    assert lib.vqhip_vec3_rate_pick(hist.ctypes.data, tols.ctypes.data, 6, -1) == -1
    with pytest.raises(ValueError, match="51 integers"):
        codec.vec3_rate_pick(hist[:, :50], tols, 5000)
    with pytest.raises(ValueError, match="shape"):
        codec.vec3_rate_pick(hist[:5], tols, 5000)
    with pytest.raises(ValueError, match="payload_budget must be >= 0"):
        codec.vec3_rate_pick(hist, tols, -1)
    with pytest.raises(TypeError, match="payload_budget"):
        codec.vec3_rate_pick(hist, tols, 5e3)


def test_wrapper_checks_its_arguments_before_any_device():
    H = codec.HipVec3Codec
    fake = object.__new__(H)                                         # no handle: every check below runs before the library is called
    x = np.zeros((2, 512, 3), F)
    for bad in ([], [0.5] * 65):
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_sweep(x, bad)
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_sweep_device(1, 1, 1, 2, bad, 1)
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_compress(x, bad, 100)
    for bad in ([0.5, -1.0], [float("-inf")]):
        with pytest.raises(ValueError, match="tol must be >= 0"):
            fake.rate_sweep(x, bad)
        with pytest.raises(ValueError, match="tol must be >= 0"):
            fake.rate_sweep_device(1, 1, 1, 2, bad, 1)
        with pytest.raises(ValueError, match="tol must be >= 0"):
            fake.rate_compress(x, bad, 100)
    for bad in ([0.5, "1"], "1", 0.5, [True]):
        with pytest.raises(TypeError, match="real number"):
            fake.rate_sweep(x, bad)
        with pytest.raises(TypeError, match="real number"):
            fake.rate_compress(x, bad, 100)
    with pytest.raises(TypeError, match="float32"):
        fake.rate_sweep(x.astype(np.float64), [0.5])
    with pytest.raises(ValueError, match="shape"):
        fake.rate_sweep(np.zeros((2, 512), F), [0.5])
    with pytest.raises(ValueError, match="shape"):
        fake.rate_compress(np.zeros((2, 512), F), [0.5], 100)
    with pytest.raises(ValueError, match="payload_budget must be >= 0"):
        fake.rate_compress(x, [0.5], -1)
    for bad in (1e6, True, "100", None):
        with pytest.raises(TypeError, match="payload_budget"):
            fake.rate_compress(x, [0.5], bad)
    with pytest.raises(ValueError, match="NULL device pointer"):
        fake.rate_sweep_device(1, 0, 1, 2, [0.5], 1)
    got = H.check_tols([0.0, 0.1, float("nan"), float("inf"), 1])
    assert got.dtype == F and got[0] == 0 and np.isnan(got[2]) and np.isinf(got[3]) and got[4] == 1
    assert got[1] == np.nextafter(F(0.1), F(0)) and float(got[1]) <= 0.1   # rounded down to float32, never up
    assert len(H.check_tols(np.geomspace(1e-3, 1.0, 64))) == 64
