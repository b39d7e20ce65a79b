"""Size sweep of the scalar handle without a GPU: the C ABI of include/vqvdb_hip_rate.h (declarations, exports,
bindings, NULL handle), the two size helpers against the numpy restatement tests/torch_ref_rate.py and against the real .vqres v2
framing of vqvdbfile, the choice of a rung within a budget, and the wrapper's argument checks."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_rate as trt  # noqa: E402
import torch_ref_residual as trr  # noqa: E402
from vqvdb_amd import codec, vqvdbfile  # noqa: E402

HEADER = os.path.join(ROOT, "include", "vqvdb_hip_rate.h")
NAMES = ["vqhip_rate_payload_bytes", "vqhip_rate_sidecar_bytes", "vqhip_rate_sweep_device", "vqhip_rate_sweep", "vqhip_rate_sweep_file",
         "vqhip_rate_compress_file"]
ARITY = {"vqhip_rate_payload_bytes": 1, "vqhip_rate_sidecar_bytes": 2, "vqhip_rate_sweep_device": 9, "vqhip_rate_sweep": 6, "vqhip_rate_sweep_file": 8,
         "vqhip_rate_compress_file": 14}
F = np.float32


def test_header_library_and_bindings_hold_exactly_the_rate_names():
    assert codec.RATE_SYMBOLS == NAMES
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(NAMES)
    assert all(n.startswith("vqhip_rate_") for n in NAMES)
    assert re.search(r"#define\s+VQHIP_RATE_MAX_TOLS\s+64\b", text) and re.search(r"#define\s+VQHIP_RATE_CLASSES\s+19\b", text)
    assert (codec.RATE_MAX_TOLS, codec.RATE_CLASSES) == (64, 19) and (trt.CLASSES, trt.RAW_COL, trt.KEPT_COL) == (19, 17, 18)
    assert re.search(r'#include\s+"vqvdb_hip_residual.h"', text)
    for name in NAMES:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert params.count(",") + 1 == ARITY[name], name
    for other in (codec.ABI_SYMBOLS, codec.VEC3_TRAIN_SYMBOLS, codec.VEC3_FULLTRAIN_SYMBOLS, codec.VEC3_PRECISION_SYMBOLS, codec.VEC3_BOUNDED_SYMBOLS,
                  codec.VEC3_RESIDUAL_SYMBOLS, codec.BOUNDED_SYMBOLS, codec.RESIDUAL_SYMBOLS):
        assert not set(NAMES) & set(other)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h == "vqvdb_hip_rate.h":
            continue
        assert "vqhip_rate_" not in open(os.path.join(ROOT, "include", h)).read(), h
    lib = codec.load_library()
    for name in NAMES:
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == ARITY[name], name
        assert f.restype == (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int), name
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_\w+)\b", out))
    assert set(NAMES) <= exported and {n for n in exported if n.startswith("vqhip_rate_")} == set(NAMES)


def test_a_null_handle_is_refused_and_the_helpers_need_no_device():
    lib = codec.load_library()
    tols, hist = np.array([0.5], F), np.zeros((1, 19), np.int64)
    used = ctypes.c_float(0)
    assert lib.vqhip_rate_sweep_device(None, None, None, None, 1, tols.ctypes.data, 1, None, None) == -1
    assert lib.vqhip_rate_sweep(None, None, 1, tols.ctypes.data, 1, hist.ctypes.data) == -1
    assert lib.vqhip_rate_sweep_file(None, None, 1, 0, tols.ctypes.data, 1, hist.ctypes.data, None) == -1
    assert lib.vqhip_rate_compress_file(None, b"a", b"b", None, 1, 0, tols.ctypes.data, 1, 0, ctypes.byref(used), None, None, None, None) == -1
    row = np.zeros(19, np.int64)
    assert codec.rate_payload_bytes(row) == 0 and codec.rate_sidecar_bytes(row, 1) == 15 and codec.rate_sidecar_bytes(row, 255) == 11 + 4 * 255
    row[:] = np.arange(1, 20)
    want = sum(64 * b * (b + 1) for b in range(17)) + 2048 * 18
    assert codec.rate_payload_bytes(row) == want == trt.payload_bytes(row)
    assert codec.rate_sidecar_bytes(row, 3) == 11 + 12 + 5 * sum(range(1, 19)) + want == trt.sidecar_bytes(row, 3)
    row[18] = 10 ** 12                                               # kept leaves cost nothing
    assert codec.rate_sidecar_bytes(row, 3) == trt.sidecar_bytes(row, 3) == 11 + 12 + 5 * sum(range(1, 19)) + want
    big = np.zeros(19, np.int64)
    big[17] = 1 << 32                                                # 2^32 raw leaves: the sums are 64-bit
    assert codec.rate_payload_bytes(big) == 2048 << 32 and codec.rate_sidecar_bytes(big, 1) == 15 + (2053 << 32)
    assert lib.vqhip_rate_payload_bytes(None) == -1 and lib.vqhip_rate_sidecar_bytes(None, 1) == -1
    for bad in (np.zeros(18, np.int64), np.zeros(19, np.float64), np.zeros((2, 19), np.int64)):
        with pytest.raises(ValueError, match="19 integers"):
            codec.rate_payload_bytes(bad)


def class_leaves(tol):
    """torch_ref_residual's one leaf per class 0 .. 16 and a 17-bit leaf (raw) at ``tol``, then a NaN leaf and a kept leaf."""
    qmax = [0, -1] + [1 << (b - 2) for b in range(2, 17)] + [32768]
    pairs = [trr.leaf_with_max_q(abs(q), tol, np.random.default_rng(b), negative=q < 0) for b, q in enumerate(qmax)]
    x, recon = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    nan_leaf = x[5].copy()
    nan_leaf[300] = np.nan
    x, recon = np.concatenate([x, nan_leaf[None], x[3:4]]), np.concatenate([recon, recon[5:6], recon[3:4]])
    with np.errstate(invalid="ignore"):
        err = np.abs(x - recon).max(axis=1)
    err[0], err[-1] = 1.0, tol                                       # the all-zero residual is selected by its error alone; equality keeps
    return x, recon, np.stack([err, err], axis=1).astype(F)


def random_leaves(tol, n=45, seed=3):
    rng = np.random.default_rng(seed)
    recon = rng.standard_normal((n, 512)).astype(F)
    x = (recon + rng.uniform(-40.0, 40.0, (n, 512)).astype(F) * F(tol) * rng.uniform(0.0, 1.0, (n, 1)).astype(F)).astype(F)
    err = np.abs(x - recon).max(axis=1)
    return x, recon, np.stack([err, err], axis=1)


def framed(x, recon, err, tol, cuts):
    """the .vqres v2 bytes of the leaves cut into grids, from the restatement's classes and records"""
    grids = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if lo == hi:                                                 # a grid without leaves: a count of zero
            grids.append((np.zeros(0, np.int64), np.zeros(0, np.uint8), []))
            continue
        cls, _ = trr.classify(x[lo:hi], recon[lo:hi], err[lo:hi], tol)
        recs = trr.records(cls, trr.pack(x[lo:hi], recon[lo:hi], tol, cls))
        ids = np.flatnonzero(cls != trr.KEPT)
        grids.append((ids, cls[ids], [recs[i] for i in ids]))
    return vqvdbfile.dumps_residual_v2(tol, grids)


def test_the_size_helpers_equal_the_framed_sidecar_to_the_byte():
    tol_s = float(F(0.66))
    for (x, recon, err), every in ((class_leaves(tol_s), True), (random_leaves(1e-3), False)):
        n = len(x)
        med = float(np.nanmedian(err[:, 0]))
        tols = [tol_s, 0.0, med, float("inf"), float("nan"), float(np.nanmin(err[:, 0])), med / 4]
        hist = trt.sweep(x, recon, err, tols)
        assert hist.shape == (len(tols), 19) and (hist.sum(axis=1) == n).all()
        if every:
            assert (hist[0] > 0).all(), hist[0]                      # every column at TOL_S: classes 0 .. 16, raw, kept
        assert hist[1, 17] == n and hist[4, 17] == n                 # tol 0 and NaN: every leaf raw
        assert hist[3, 18] == n - int(np.isnan(err[:, 0]).sum())     # +inf keeps every leaf with a finite error
        for g, cuts in ((1, (0, n)), (2, (0, n // 3, n)), (3, (0, 7, 7, n))):   # the third split has an empty grid
            for t, tol in enumerate(tols):
                buf = framed(x, recon, err, tol, cuts)
                assert codec.rate_sidecar_bytes(hist[t], g) == len(buf) == trt.sidecar_bytes(hist[t], g), (g, tol)
                cls, off = trr.classify(x, recon, err, tol)
                assert codec.rate_payload_bytes(hist[t]) == off[-1] == trt.payload_bytes(hist[t]), tol


def test_pick_takes_the_smallest_fitting_value_not_the_first_fitting_index():
    def row(raw, b4):
        r = np.zeros(19, np.int64)
        r[17], r[4], r[18] = raw, b4, 100 - raw - b4
        return r

    # sizes 15 + 5 * selected + 2048 * raw + 256 * b4: not monotone in the tolerance (the rung 0.2 escapes to raw leaves)
    tols = np.array([0.4, np.nan, 0.1, 0.2, 0.3, 0.3], F)
    hist = np.stack([row(0, 2), row(0, 0), row(0, 40), row(30, 10), row(0, 8), row(0, 8)])
    sizes = [trt.sidecar_bytes(r, 1) for r in hist]
    assert sizes == [15 + 10 + 512, 15, 15 + 200 + 10240, 15 + 200 + 61440 + 2560, 15 + 40 + 2048, 15 + 40 + 2048]
    assert trt.pick(hist, tols, 1, 5000) == 4                        # 0.3 (its duplicate would do as well), not index 0 = 0.4
    assert tols[trt.pick(hist, tols, 1, 11000)] == F(0.1)            # 0.1 fits although the larger 0.2 does not
    assert trt.pick(hist, tols, 1, 600) == 0
    assert trt.pick(hist, tols, 1, 10 ** 9) == 2
    with pytest.raises(ValueError, match="no rung fits 100 bytes"):
        trt.pick(hist, tols, 1, 100)                                 # only the NaN rung's 15 bytes would fit: never chosen
    with pytest.raises(ValueError):
        trt.pick(hist[1:2], tols[1:2], 1, 10 ** 9)


def test_wrapper_checks_its_arguments_before_any_device():
    H = codec.HipCodec
    fake = object.__new__(H)                                         # no handle: every check below runs before the library is called
    x = np.zeros((2, 512), F)
    for bad in ([], [0.5] * 65):
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_sweep(x, bad)
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_sweep_device(1, 1, 1, 2, bad, 1)
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_sweep_file([], bad)
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_compress_file("a", "b", [], bad, 100)
    for bad in ([0.5, -1.0], [float("-inf")]):
        with pytest.raises(ValueError, match="tol must be >= 0"):
            fake.rate_sweep(x, bad)
        with pytest.raises(ValueError, match="tol must be >= 0"):
            fake.rate_sweep_device(1, 1, 1, 2, bad, 1)
        with pytest.raises(ValueError, match="tol must be >= 0"):
            fake.rate_sweep_file([], bad)
        with pytest.raises(ValueError, match="tol must be >= 0"):
            fake.rate_compress_file("a", "b", [], bad, 100)
    for bad in ([0.5, "1"], "1", 0.5):
        with pytest.raises(TypeError, match="real number"):
            fake.rate_sweep(x, bad)
    with pytest.raises(TypeError, match="float32"):
        fake.rate_sweep(x.astype(np.float64), [0.5])
    with pytest.raises(ValueError, match="shape"):
        fake.rate_sweep(np.zeros((2, 511), F), [0.5])
    with pytest.raises(ValueError, match="sidecar_budget must be >= 0"):
        fake.rate_compress_file("a", "b", [], [0.5], -1)
    with pytest.raises(TypeError, match="sidecar_budget"):
        fake.rate_compress_file("a", "b", [], [0.5], 1e6)
    with pytest.raises(ValueError, match="rounds"):
        fake.rate_compress_file("a", "b", [], [0.5], 100, rounds=0)
    with pytest.raises(ValueError, match="NULL device pointer"):
        fake.rate_sweep_device(1, 0, 1, 2, [0.5], 1)
    got = H.check_tols([0.0, 0.1, float("nan"), float("inf"), 1])
    assert got.dtype == F and got[0] == 0 and np.isnan(got[2]) and np.isinf(got[3]) and got[4] == 1
    assert got[1] == np.nextafter(F(0.1), F(0)) and float(got[1]) <= 0.1   # rounded down to float32, never up
