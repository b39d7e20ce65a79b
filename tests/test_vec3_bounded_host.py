"""Error-bounded round trip of the Vec3 handle without a GPU: the C ABI of
include/vqvdb_hip_vec3_bounded.h (declarations, exports, bindings), the numpy restatement tests/torch_ref_vec3_bounded.py
against float64 on the fixture leaves, the selection rule on hand-made errors, and the compress_bounded /
decompress_bounded bookkeeping of the wrapper on a codec without a device."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
import torch_ref_vec3_bounded as tbd  # noqa: E402
from vqvdb_amd import codec, synth_vec3  # noqa: E402

HEADER = os.path.join(ROOT, "include", "vqvdb_hip_vec3_bounded.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_v1.npz")
# include/vqvdb_hip.h as it was before this header existed, plus vqhip_compute_units on the scalar handle and the sentence on refused
# kernel-switch values in three of its comments: its Vec3 name list is fixed
VQVDB_HIP_H_SHA256 = "2454f49845215e149f40bebc8b33e62811d2966f515d1e6fb88bb1d967cdaede"
NAMES = ["vqhip_vec3_roundtrip_device", "vqhip_vec3_select_outliers_device", "vqhip_vec3_compress_bounded"]


@pytest.fixture(scope="module")
def leaves():
    return np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])


@pytest.fixture(scope="module")
def recon(leaves):
    """The fixture leaves' own reconstructions: the float32 torch restatement of the decoder on the fixture's indices."""
    w32 = tr.weights_to_torch(synth_vec3.make_weights(0), torch.float32)
    with torch.no_grad():
        return tr.decode(np.load(GOLDEN)["idx"], w32).numpy()


def test_header_library_and_bindings_hold_exactly_the_three_names():
    assert codec.VEC3_BOUNDED_SYMBOLS == NAMES
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(vqhip_vec3_\w+)\s*\(", text))) == sorted(NAMES)
    assert re.search(r"#define\s+VQHIP_VEC3_ERR_FLOATS\s+2\b", text) and codec.VEC3_ERR_FLOATS == 2
    for other in (codec.ABI_SYMBOLS, codec.VEC3_TRAIN_SYMBOLS, codec.VEC3_FULLTRAIN_SYMBOLS, codec.VEC3_PRECISION_SYMBOLS):
        assert not set(NAMES) & set(other)
    with open(os.path.join(ROOT, "include", "vqvdb_hip.h"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == VQVDB_HIP_H_SHA256
    lib = codec.load_library()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype == ctypes.c_int, name
    assert len(lib.vqhip_vec3_roundtrip_device.argtypes) == 7
    assert lib.vqhip_vec3_select_outliers_device.argtypes[3] == ctypes.c_float and len(lib.vqhip_vec3_select_outliers_device.argtypes) == 7
    assert lib.vqhip_vec3_compress_bounded.argtypes[3] == ctypes.c_float and len(lib.vqhip_vec3_compress_bounded.argtypes) == 8
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(vqhip_vec3_(?:roundtrip|select|compress)\w*)\b", out)) == set(NAMES)
    # a NULL handle is refused without a device
    assert lib.vqhip_vec3_roundtrip_device(None, None, 1, None, None, None, None) == -1
    assert lib.vqhip_vec3_select_outliers_device(None, None, 1, 0.0, None, None, None) == -1
    assert lib.vqhip_vec3_compress_bounded(None, None, 1, 0.0, None, None, None, None) == -1


def test_fixed_order_sum_is_within_1e5_of_float64_on_the_fixture_reconstructions(leaves, recon):
    """<= 15 chained float32 additions per leaf (2 in the lane, 6 wave levels, 7 across waves) of non-negative terms, each
    term two roundings (difference, square): about 18 * 2^-24 = 1.1e-6 relative, inside the 42 * 2^-24 = 2.5e-6 of the
    contract and the project's 1e-5 bar."""
    got, ref = tbd.leaf_err_fixed(leaves, recon), tbd.leaf_err_f64(leaves, recon)
    assert got.dtype == np.float32 and got.shape == (520, 2)
    assert (ref[:, 1] > 0).all()
    rel = np.abs(got[:, 1].astype(np.float64) - ref[:, 1]) / ref[:, 1]
    print(f"fixed-order float32 sum against float64: largest relative difference {rel.max():.2e}")
    assert rel.max() <= 1e-5
    # the maximum of float32 differences: no reduction error, only the rounding of each difference
    assert np.array_equal(got[:, 0], np.abs(leaves - recon).reshape(520, -1).max(axis=1))
    assert (np.abs(got[:, 0].astype(np.float64) - ref[:, 0]) <= 2.0 ** -24 * np.maximum(ref[:, 0], 1.0)).all()


def test_fixed_order_depends_on_the_leaf_only_and_keeps_non_finite_values(leaves, recon):
    a = tbd.leaf_err_fixed(leaves, recon)
    p = np.random.default_rng(0).permutation(520)
    assert np.array_equal(tbd.leaf_err_fixed(leaves[p], recon[p]).view(np.uint32), a[p].view(np.uint32))
    assert np.array_equal(tbd.leaf_err_fixed(leaves[7:8], recon[7:8]).view(np.uint32), a[7:8].view(np.uint32))
    x = leaves[:4].copy()
    x[1, 100, 2] = np.nan
    x[2, 511, 0] = np.inf
    x[3, 0, 1] = -np.inf
    e = tbd.leaf_err_fixed(x, recon[:4])
    assert np.array_equal(e[0].view(np.uint32), a[0].view(np.uint32))
    assert np.isnan(e[1:, 0]).all() and np.isnan(e[1, 1]) and np.isposinf(e[2:, 1]).all()
    # exact reconstruction: zero error, not selected at tol 0
    z = tbd.leaf_err_fixed(leaves[:2], leaves[:2])
    assert not z.any() and tbd.select_outliers(z, 0.0).size == 0


def test_selection_rule_on_hand_made_errors():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    e = np.array([[0.5, 9], [0.25, 9], [nan, nan], [0.0, 0], [inf, inf], [0.25, 1], [1.0, 2]], dtype=np.float32)
    sel = lambda tol: tbd.select_outliers(e, tol).tolist()   # noqa: E731
    assert sel(0.25) == [0, 2, 4, 6]          # equality is not an outlier
    assert sel(np.nextafter(np.float32(0.25), np.float32(0))) == [0, 1, 2, 4, 5, 6]
    assert sel(0.0) == [0, 1, 2, 4, 5, 6]
    assert sel(inf) == [2]                    # only the NaN error
    assert sel(nan) == [0, 1, 2, 3, 4, 5, 6]  # a NaN tolerance selects everything
    assert sel(-1.0) == [0, 1, 2, 3, 4, 5, 6]
    assert sel(1.0) == [2, 4]
    assert tbd.select_outliers(np.zeros((0, 2), np.float32), 0.5).dtype == np.int64
    assert tbd.select_outliers(e, 0.25).dtype == np.int64


class _FakeCodec(codec.HipVec3Codec):
    """The wrapper's bookkeeping around a codec without a device: 'decode' returns a stored lossy copy of the leaves."""

    def __init__(self, leaves, noise):
        self._x = leaves
        self._rec = (leaves + noise).astype(np.float32)

    def _compress_bounded_host(self, leaves, tol):
        assert leaves is self._x or np.array_equal(leaves, self._x)
        err = tbd.leaf_err_fixed(leaves, self._rec)
        idx = np.arange(len(leaves) * 64, dtype=np.int64).reshape(-1, 64).astype(np.uint16)
        return idx, err, tbd.select_outliers(err, tol)

    def decode(self, indices):
        assert indices.dtype == np.uint16 and indices.shape == (len(self._x), 64)
        return self._rec.copy()


def test_compress_decompress_bounded_honours_the_tolerance_on_a_fake_codec(leaves):
    rng = np.random.default_rng(5)
    x = np.ascontiguousarray(leaves[:64])
    noise = (rng.standard_normal(x.shape) * rng.uniform(1e-4, 1e-1, size=(64, 1, 1))).astype(np.float32)
    noise[9] = 0.0
    fake = _FakeCodec(x, noise)
    worst = np.abs(x - fake._rec).reshape(64, -1).max(axis=1)
    for tol in (float(np.median(worst)), float(worst[3]), 0.0, float("inf"), 1e-3):
        idx, ids, raw = fake.compress_bounded(x, tol)
        assert ids.dtype == np.int64 and raw.shape == (len(ids), 512, 3) and (np.diff(ids) > 0).all()
        assert np.array_equal(ids, np.flatnonzero(~(worst <= np.float32(tol))))
        out = fake.decompress_bounded(idx, ids, raw)
        assert float(np.abs(x - out).max()) <= tol
        assert np.array_equal(out[ids], x[ids])
        keep = np.setdiff1d(np.arange(64), ids)
        assert np.array_equal(out[keep], fake._rec[keep])
    idx, ids, raw = fake.compress_bounded(x, 0.0)
    assert 9 not in ids and len(ids) == 63 and np.array_equal(fake.decompress_bounded(idx, ids, raw), x)
    idx, ids, raw, err = fake.compress_bounded(x, float(worst[3]), return_leaf_err=True)
    assert 3 not in ids and np.array_equal(err[:, 0], worst)
    with pytest.raises(ValueError, match="outlier ids but"):
        fake.decompress_bounded(idx, ids, raw[:-1])
    with pytest.raises(ValueError, match="outlier ids must be in"):
        fake.decompress_bounded(idx, np.array([64]), raw[:1])


def test_wrapper_checks_its_arguments_before_any_device():
    ck = codec.HipVec3Codec.check_tol
    assert ck(0.5) == 0.5 and ck(0) == 0.0 and ck(float("inf")) == float("inf") and np.isnan(ck(float("nan")))
    assert ck(np.float32(0.1)) == float(np.float32(0.1))
    assert ck(0.1) <= 0.1 and ck(0.1) == float(np.nextafter(np.float32(0.1), np.float32(0)))   # never rounded up
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(TypeError, match="tol must be a real number"):
            ck(bad)
    fake = _FakeCodec(np.zeros((1, 512, 3), np.float32), np.zeros((1, 512, 3), np.float32))
    with pytest.raises(TypeError, match="float32 numpy array"):
        fake.compress_bounded(np.zeros((1, 512, 3), np.float64), 0.1)
    with pytest.raises(TypeError, match="float32 numpy array or a contiguous float32 torch tensor"):
        fake.roundtrip(torch.zeros((1, 512, 3)))
    with pytest.raises(ValueError, match="leaf_err_ptr is NULL"):
        fake.roundtrip_device(1, 1, 0)
    with pytest.raises(ValueError, match="count_ptr is NULL"):
        fake.select_outliers_device(1, 1, 0.5, 1, 0)
