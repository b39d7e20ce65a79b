"""Active-voxel masks without a GPU: the C ABI of include/vqvdb_hip_vec3_mask.h (declarations, exports, bindings,
prefix rules, NULL handle; the scalar handle has no masked calls), the mask's bit order on literal examples, and the numpy
restatement tests/torch_ref_masked.py, for one channel and for three, held against the contract: direct definition == substitution
principle, all-ones mask == the unmasked restatements, monotonicity per leaf, and the designed input that the GPU tests reuse."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_bounded as tbd  # noqa: E402
import torch_ref_masked as trm  # noqa: E402
import torch_ref_rate as trt  # noqa: E402
import torch_ref_residual as trr  # noqa: E402
import torch_ref_vec3_bounded as t3b  # noqa: E402
import torch_ref_vec3_rate as t3t  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import codec  # noqa: E402

F = np.float32
V3_NAMES = ["vqhip_vec3_mask_leaf_err_device", "vqhip_vec3_mask_residual_encode_device", "vqhip_vec3_mask_sweep_device",
            "vqhip_vec3_mask_compress_residual", "vqhip_vec3_mask_sweep"]
V3_ARITY = {"vqhip_vec3_mask_leaf_err_device": 7, "vqhip_vec3_mask_residual_encode_device": 12, "vqhip_vec3_mask_sweep_device": 10,
            "vqhip_vec3_mask_compress_residual": 10, "vqhip_vec3_mask_sweep": 7}
FORBIDDEN_PREFIXES = ("vqhip_rate_", "vqhip_vec3_rate_", "vqhip_vec3_fulltrain_", "vqhip_vec3_train_", "vqhip_vec3_roundtrip", "vqhip_vec3_select",
                      "vqhip_vec3_compress")


def unmasked(C):
    """(leaf_err_fixed, classify, pack, sweep, KEPT, RAW) of the existing restatements"""
    if C == 1:
        return tbd.leaf_err_fixed, trr.classify, trr.pack, trt.sweep, trr.KEPT, trr.RAW
    return t3b.leaf_err_fixed, t3r.classify, t3r.pack, t3t.sweep, t3r.KEPT, t3r.RAW


def test_headers_library_and_bindings_hold_exactly_the_mask_names():
    assert codec.VEC3_MASK_SYMBOLS == V3_NAMES and codec.MASK_WORDS == 8 and not hasattr(codec, "MASK_SYMBOLS")
    lib = codec.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_\w+)\b", out))
    for header, names, arity, prefix, parent in (("vqvdb_hip_vec3_mask.h", V3_NAMES, V3_ARITY, "vqhip_vec3_mask_", "vqvdb_hip_vec3_rate.h"),):
        raw = open(os.path.join(ROOT, "include", header)).read()
        assert "vqhip_rate_" not in raw and "vqhip_vec3_rate_" not in raw, header     # comments included: older tests search every header
        text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
        assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(names), header
        assert all(n.startswith(prefix) for n in names)
        assert re.search(r'#include\s+"' + re.escape(parent) + '"', text), header
        assert re.search(r"#define\s+VQHIP_VEC3_MASK_WORDS\s+8\b", text), header
        for name in names:
            params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
            assert params.count(",") + 1 == arity[name], name
            f = getattr(lib, name)
            assert f.argtypes is not None and len(f.argtypes) == arity[name] and f.restype == ctypes.c_int, name
            assert not any(name.startswith(p) for p in FORBIDDEN_PREFIXES) and "precision" not in name, name
        assert {n for n in exported if n.startswith(prefix)} == set(names), header
    for other in (codec.ABI_SYMBOLS, codec.VEC3_TRAIN_SYMBOLS, codec.VEC3_FULLTRAIN_SYMBOLS, codec.VEC3_PRECISION_SYMBOLS, codec.VEC3_BOUNDED_SYMBOLS,
                  codec.VEC3_RESIDUAL_SYMBOLS, codec.VEC3_RATE_SYMBOLS, codec.BOUNDED_SYMBOLS, codec.RESIDUAL_SYMBOLS, codec.RATE_SYMBOLS):
        assert not set(V3_NAMES) & set(other)
    assert {n for n in exported if "precision" in n} == set(codec.VEC3_PRECISION_SYMBOLS)
    assert not {n for n in exported if n.startswith("vqhip_mask_")}                         # the scalar handle has no masked calls
    assert "mask" not in open(os.path.join(ROOT, "include", "vqvdb_hip.h")).read().lower()   # nothing new in the base header
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "vqvdb_hip_vec3_mask.h":
            assert "vqhip_mask_" not in open(os.path.join(ROOT, "include", h)).read() and "vqhip_vec3_mask_" not in open(os.path.join(ROOT, "include", h)).read(), h


def test_a_null_handle_is_refused():
    lib = codec.load_library()
    tols, hist, nbytes = np.array([0.5], F), np.zeros((1, 51), np.int64), ctypes.c_int64(0)
    assert lib.vqhip_vec3_mask_leaf_err_device(None, None, None, None, 1, None, None) == -1
    assert lib.vqhip_vec3_mask_residual_encode_device(None, None, None, None, None, 1, 0.5, None, None, None, 0, None) == -1
    assert lib.vqhip_vec3_mask_sweep_device(None, None, None, None, None, 1, tols.ctypes.data, 1, None, None) == -1
    assert lib.vqhip_vec3_mask_compress_residual(None, None, None, 1, 0.5, None, None, None, None, ctypes.byref(nbytes)) == -1
    assert lib.vqhip_vec3_mask_sweep(None, None, None, 1, tols.ctypes.data, 1, hist.ctypes.data) == -1


def test_mask_bit_order_on_literal_examples():
    want = {0: (0, 1), 63: (0, 1 << 63), 64: (1, 1), 511: (7, 1 << 63), 65: (1, 2), 448: (7, 1)}
    for voxel, (word, value) in want.items():
        a = np.zeros((2, 512), bool)
        a[1, voxel] = True
        for got in (codec.pack_masks(a), trm.pack_masks(a), codec.pack_masks(a.reshape(2, 8, 8, 8))):
            assert got.dtype == np.uint64 and got.shape == (2, 8) and not got[0].any()
            assert int(got[1, word]) == value and int((got[1] != 0).sum()) == 1, voxel
        assert np.array_equal(trm.unpack_masks(trm.pack_masks(a)), a)
    # the voxel offset is d*64 + h*8 + w: word d, bit h*8 + w
    a = np.zeros((1, 8, 8, 8), bool)
    a[0, 3, 2, 5] = True
    assert int(codec.pack_masks(a)[0, 3]) == 1 << 21
    rnd = np.random.default_rng(1).random((5, 512)) < 0.5
    assert np.array_equal(codec.pack_masks(rnd), trm.pack_masks(rnd)) and np.array_equal(trm.unpack_masks(codec.pack_masks(rnd)), rnd)
    assert (codec.pack_masks(np.ones((3, 512), bool)) == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    with pytest.raises(TypeError, match="bool"):
        codec.pack_masks(np.ones((3, 512), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        codec.pack_masks(np.ones((3, 511), bool))
    good = codec.pack_masks(rnd)
    assert codec.check_masks(good, 5) is good
    with pytest.raises(TypeError, match="uint64"):
        codec.check_masks(good.astype(np.int64), 5)
    with pytest.raises(ValueError, match="shape"):
        codec.check_masks(good.reshape(-1), 5)
    with pytest.raises(ValueError, match="5 masks"):
        codec.check_masks(good, 4)
    with pytest.raises(ValueError, match="contiguous"):
        codec.check_masks(np.zeros((5, 16), np.uint64)[:, ::2], 5)


def finite_batch(C, n=24, seed=5):
    """finite x^ and x = x^ + noise whose scale differs from leaf to leaf, with some exact zeros, -0 in x^ and a huge value in x"""
    rng = np.random.default_rng(seed + C)
    shape = (n, 512) if C == 1 else (n, 512, 3)
    recon = rng.standard_normal(shape).astype(F)
    recon[0].flat[:7] = F(-0.0)
    scale = (10.0 ** rng.uniform(-4, 0, n)).astype(F).reshape((n,) + (1,) * (len(shape) - 1))
    x = (recon + rng.standard_normal(shape).astype(F) * scale).astype(F)
    x[1].flat[11] = F(3e38)                                             # a difference that overflows when squared
    x[2] = recon[2]                                                     # a leaf without error
    return x, recon


def mask_set(n, x=None, seed=9):
    rng = np.random.default_rng(seed)
    word = np.zeros((n, 512), bool)
    for i in range(n):
        word[i, 64 * (i % 8):64 * (i % 8) + 64] = True
    return {"ones": np.ones((n, 512), bool), "zeros": np.zeros((n, 512), bool), "half": rng.random((n, 512)) < 0.5,
            "sparse": rng.random((n, 512)) < 0.05, "one_word": word}


def tolerances(err):
    e = err[:, 0]
    e = e[np.isfinite(e)]
    return [float(e.min()), float(np.quantile(e, 0.25, method="lower")), float(np.median(e)), float(e.max()), float("inf"), 0.0, float("nan")]


def from_substitution(C, x, recon, active, tol):
    """what the contract's substitution principle predicts: the unmasked restatement on x' = where(active, x, x^), with the two
    exceptions the contract names (raw records hold x; a selected leaf without active voxels has code 0 and no record)"""
    err_u, classify_u, pack_u, _, KEPT, RAW = unmasked(C)
    xs = trm.substitute(x, recon, active, C)
    err = err_u(xs, recon)
    code, _ = classify_u(xs, recon, err, tol)
    code = code.copy()
    empty = ~active.any(axis=1)
    code[empty & (code == RAW)] = 0
    recs = []
    for i, c in enumerate(code):
        src = x if int(c) == RAW else xs
        recs.append(pack_u(src[i:i + 1], recon[i:i + 1], tol, [c]))
    return err, code, recs


@pytest.mark.parametrize("C", (1, 3))
def test_direct_definition_equals_the_substitution_principle(C):
    x, recon = finite_batch(C)
    for name, active in mask_set(len(x)).items():
        err = trm.leaf_err_fixed(x, recon, active, C)
        if name == "zeros":
            assert err.tobytes() == np.zeros_like(err).tobytes()                                  # {+0, +0}, not -0
        for tol in tolerances(trm.leaf_err_fixed(x, recon, np.ones_like(active), C)):
            serr, scode, srecs = from_substitution(C, x, recon, active, tol)
            assert err.tobytes() == serr.tobytes(), (name, tol)
            code, off = trm.classify(x, recon, err, tol, active, C)
            assert np.array_equal(code, scode), (name, tol, np.flatnonzero(code != scode)[:5])
            payload = trm.pack(x, recon, tol, code, active, C)
            assert len(payload) == off[-1] and payload == b"".join(srecs), (name, tol)


@pytest.mark.parametrize("C", (1, 3))
def test_an_all_ones_mask_equals_the_unmasked_restatement(C):
    err_u, classify_u, pack_u, sweep_u, _, _ = unmasked(C)
    x, recon = finite_batch(C)
    x[3].flat[100] = np.nan                                                                       # non-finite values as before
    x[4].flat[9] = np.inf
    ones = np.ones((len(x), 512), bool)
    err = trm.leaf_err_fixed(x, recon, ones, C)
    assert err.tobytes() == err_u(x, recon).tobytes() and np.isnan(err[3, 0]) and np.isnan(err[4, 0])
    tols = tolerances(err)
    for tol in tols:
        code, off = trm.classify(x, recon, err, tol, ones, C)
        ucode, uoff = classify_u(x, recon, err, tol)
        assert np.array_equal(code, ucode) and np.array_equal(off, uoff), tol
        assert trm.pack(x, recon, tol, code, ones, C) == pack_u(x, recon, tol, ucode), tol
    assert np.array_equal(trm.sweep(x, recon, err, tols, ones, C), sweep_u(x, recon, err, tols))


@pytest.mark.parametrize("C", (1, 3))
def test_a_mask_never_grows_a_record_and_a_kept_leaf_stays_kept(C):
    err_u, classify_u, _, _, KEPT, _ = unmasked(C)
    x, recon = finite_batch(C)
    x[5].flat[40] = np.nan
    dx, dr, dact, _ = trm.designed(C)
    x, recon = np.concatenate([x, dx]), np.concatenate([recon, dr])
    uerr = err_u(x, recon)
    masks = mask_set(len(x))
    masks["designed"] = np.concatenate([np.ones((len(x) - len(dx), 512), bool), dact])
    for name, active in masks.items():
        err = trm.leaf_err_fixed(x, recon, active, C)
        for tol in tolerances(uerr) + [trm.TOL_D]:
            code, _ = trm.classify(x, recon, err, tol, active, C)
            ucode, _ = classify_u(x, recon, uerr, tol)
            assert (trm.record_size(code, C) <= trm.record_size(ucode, C)).all(), (name, tol)
            assert (code[ucode == KEPT] == KEPT).all(), (name, tol)


@pytest.mark.parametrize("C", (1, 3))
def test_the_designed_input_holds_one_leaf_of_every_kind(C):
    err_u, classify_u, _, _, KEPT, RAW = unmasked(C)
    x, recon, active, kinds = trm.designed(C)
    tol = trm.TOL_D
    k = {name: i for i, name in enumerate(kinds)}
    assert np.isfinite(recon).all() and len(x) == len(kinds) == 9
    uerr, err = err_u(x, recon), trm.leaf_err_fixed(x, recon, active, C)
    ucode, uoff = classify_u(x, recon, uerr, tol)
    code, off = trm.classify(x, recon, err, tol, active, C)
    usize, size = trm.record_size(ucode, C), trm.record_size(code, C)
    quant = lambda c: c not in (KEPT, RAW)                                                        # noqa: E731
    i = k["kept_by_mask"]
    assert quant(ucode[i]) and usize[i] > 0 and code[i] == KEPT and err[i, 0] == 0 and uerr[i, 0] > tol
    i = k["narrower_by_mask"]
    assert quant(ucode[i]) and quant(code[i]) and 0 < size[i] < usize[i]
    i = k["raw_to_quantised"]
    assert ucode[i] == RAW and np.isnan(uerr[i, 0]) and quant(code[i]) and np.isfinite(err[i]).all() and 0 < size[i] < usize[i]
    i = k["raw_either_way"]
    assert ucode[i] == RAW and code[i] == RAW and np.isnan(err[i, 0])
    i = k["all_inactive"]
    assert not active[i].any() and err[i].tobytes() == np.zeros(2, F).tobytes() and code[i] == KEPT and quant(ucode[i])
    assert trm.classify(x, recon, err, float("nan"), active, C)[0][i] == 0                        # selected without active voxels: code 0
    for name, v in (("single_0", 0), ("single_63", 63), ("single_64", 64), ("single_511", 511)):
        i = k[name]
        assert active[i].sum() == 1 and active[i, v] and quant(code[i]) and quant(ucode[i]) and 0 < size[i] < usize[i], name
        rec = trm.records(code, trm.pack(x, recon, tol, code, active, C), C)[i]
        words = np.frombuffer(rec, "<u8").reshape(-1, 8)
        assert (words[:, [w for w in range(8) if w != v // 64]] == 0).all() and not (words[:, v // 64] & ~np.uint64(1 << (v % 64))).any(), name
    assert off[-1] < uoff[-1]
    # after the existing decoder: raw leaves are x, the bound holds at every active value, inactive values are x^ + 0 * step
    payload = trm.pack(x, recon, tol, code, active, C)
    out = trm.apply(recon, tol, code, payload, C)
    act = trm._active(active, C)
    for i, c in enumerate(code):
        if c == KEPT:
            assert out[i].tobytes() == recon[i].tobytes()
        elif c == RAW:
            assert out[i].tobytes() == x[i].tobytes()
        else:
            assert (np.abs(x[i] - out[i])[act[i]] <= F(tol)).all(), kinds[i]
            assert (out[i] + F(0)).tobytes() == out[i].tobytes() and np.array_equal(out[i][~act[i]], (recon[i] + F(0) * trr.step_of(tol))[~act[i]])
    assert (np.abs(x - recon)[act & (code == KEPT).reshape((-1,) + (1,) * (act.ndim - 1))] <= F(tol)).all()


def test_wrapper_checks_its_arguments_before_any_device():
    m = np.zeros((2, 8), np.uint64)
    for H, leaves in ((codec.HipVec3Codec, np.zeros((2, 512, 3), F)),):
        fake = object.__new__(H)                                        # no handle: every check below runs before the library is called
        with pytest.raises(TypeError, match="uint64"):
            fake.compress_residual_masked(leaves, m.astype(np.int64), 0.5)
        with pytest.raises(ValueError, match="2 leaves but 3 masks"):
            fake.compress_residual_masked(leaves, np.zeros((3, 8), np.uint64), 0.5)
        with pytest.raises(ValueError, match="shape"):
            fake.rate_sweep_masked(leaves, np.zeros((2, 7), np.uint64), [0.5])
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.rate_sweep_masked(leaves, m, [])
        with pytest.raises(ValueError, match="NULL device pointer"):
            fake.mask_leaf_err_device(1, 1, 0, 2, 1)
        with pytest.raises(ValueError, match="NULL device pointer"):
            fake.mask_residual_encode_device(1, 1, 0, 1, 2, 0.5, 1, 1, 1, 10)
        with pytest.raises(ValueError, match="payload_capacity"):
            fake.mask_residual_encode_device(1, 1, 1, 1, 2, 0.5, 1, 1, 1, -1)
        with pytest.raises(ValueError, match="NULL device pointer"):
            fake.mask_sweep_device(1, 1, 0, 1, 2, [0.5], 1)
        with pytest.raises(ValueError, match="1..64 tolerances"):
            fake.mask_sweep_device(1, 1, 1, 1, 2, [0.5] * 65, 1)
