"""Error-bounded compression of the scalar handle without a GPU: the C ABI of include/vqvdb_hip_bounded.h
(declarations, exports, bindings, NULL handle), the .vqres sidecar in numpy, the numpy restatement
tests/torch_ref_bounded.py against numpy's maximum and a float64 sum on the oracle's reconstructions, non-finite voxels, and
the argument checks of the wrapper on a codec without a device."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_bounded as tbd  # noqa: E402
from vqvdb_amd import codec, synth, vqvdbfile  # noqa: E402

HEADER = os.path.join(ROOT, "include", "vqvdb_hip_bounded.h")
NAMES = ["vqhip_roundtrip_device", "vqhip_select_outliers_device", "vqhip_compress_bounded", "vqhip_decompress_bounded",
         "vqhip_compress_file_bounded", "vqhip_decompress_file_bounded"]
ARITY = {"vqhip_roundtrip_device": 7, "vqhip_select_outliers_device": 7, "vqhip_compress_bounded": 8, "vqhip_decompress_bounded": 7,
         "vqhip_compress_file_bounded": 9, "vqhip_decompress_file_bounded": 8}


@pytest.fixture(scope="module")
def leaves():
    return np.concatenate([synth.make_leaves(64), synth.edge_leaves(), synth.sparse_leaves(64)])


@pytest.fixture(scope="module")
def recon(leaves, oracle):
    """The oracle's encode -> decode of the leaves."""
    t = min(16, os.cpu_count() or 1)
    return oracle.decode(oracle.encode(leaves, threads=t), threads=t)


def test_header_library_and_bindings_hold_exactly_the_six_names():
    assert codec.BOUNDED_SYMBOLS == NAMES
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(NAMES)
    assert re.search(r"#define\s+VQHIP_ERR_FLOATS\s+2\b", text) and codec.ERR_FLOATS == 2
    for name in NAMES:   # the arity of every declaration: the commas of its parameter list
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert params.count(",") + 1 == ARITY[name], name
    for other in (codec.ABI_SYMBOLS, codec.VEC3_TRAIN_SYMBOLS, codec.VEC3_FULLTRAIN_SYMBOLS, codec.VEC3_PRECISION_SYMBOLS, codec.VEC3_BOUNDED_SYMBOLS):
        assert not set(NAMES) & set(other)
    main = open(os.path.join(ROOT, "include", "vqvdb_hip.h")).read()
    for name in NAMES:
        assert not re.search(r"\b" + name + r"\s*\(", main), name
    lib = codec.load_library()
    for name in NAMES:
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == ARITY[name] and f.restype == ctypes.c_int, name
    assert lib.vqhip_select_outliers_device.argtypes[3] == ctypes.c_float
    assert lib.vqhip_compress_bounded.argtypes[3] == ctypes.c_float
    assert lib.vqhip_compress_file_bounded.argtypes[6] == ctypes.c_float
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_\w+)\b", out))
    assert set(NAMES) <= exported
    # a NULL handle is refused by every call, without a device
    assert lib.vqhip_roundtrip_device(None, None, 1, None, None, None, None) == -1
    assert lib.vqhip_select_outliers_device(None, None, 1, 0.0, None, None, None) == -1
    assert lib.vqhip_compress_bounded(None, None, 1, 0.0, None, None, None, None) == -1
    assert lib.vqhip_decompress_bounded(None, None, 1, None, 0, None, None) == -1
    assert lib.vqhip_compress_file_bounded(None, b"a", b"b", None, 1, 0, 0.0, None, None) == -1
    assert lib.vqhip_decompress_file_bounded(None, b"a", b"b", 0, codec.GRID_BEGIN_FN(), codec.LEAF_ALLOC_FN(), None, None) == -1
    assert ctypes.sizeof(codec.BoundedStats) == 32


def test_residual_file_round_trips_in_numpy(tmp_path, leaves):
    ids0 = np.array([0, 3, 69], dtype=np.int64)
    raw0 = leaves[[5, 70, 100]].copy()
    raw0[1, 17] = np.float32(np.nan)
    raw0.view(np.uint32)[2, 9] = 0x7FC12345                     # a NaN payload survives
    grids = [(ids0, raw0), (np.zeros(0, np.int64), np.zeros((0, 512), np.float32))]
    buf = vqvdbfile.dumps_residual(0.125, grids)
    assert len(buf) == 11 + 4 + 3 * 2052 + 4
    assert buf[:7] == b"VQRES\x01\x02" and struct.unpack_from("<f", buf, 7)[0] == 0.125
    assert struct.unpack_from("<I", buf, 11)[0] == 3 and struct.unpack_from("<I", buf, 15)[0] == 0
    assert struct.unpack_from("<I", buf, 15 + 2052)[0] == 3 and struct.unpack_from("<I", buf, len(buf) - 4)[0] == 0
    assert buf[19:19 + 2048] == raw0[0].tobytes()
    tol, got = vqvdbfile.loads_residual(buf)
    assert tol == 0.125 and len(got) == 2
    assert np.array_equal(got[0][0], ids0) and got[0][0].dtype == np.int64
    assert np.array_equal(got[0][1].view(np.uint32), raw0.view(np.uint32))
    assert got[1][0].shape == (0,) and got[1][1].shape == (0, 512)
    path = tmp_path / "a.vqres"
    vqvdbfile.save_residual(path, 0.125, grids)
    assert path.read_bytes() == buf
    tol2, got2 = vqvdbfile.load_residual(path)
    assert tol2 == tol and np.array_equal(got2[0][1].view(np.uint32), raw0.view(np.uint32))
    assert np.isnan(vqvdbfile.loads_residual(vqvdbfile.dumps_residual(float("nan"), grids))[0])
    for cut in (5, 10, 13, 15 + 2051, len(buf) - 1):
        with pytest.raises(ValueError, match="truncated|header"):
            vqvdbfile.loads_residual(buf[:cut])
    with pytest.raises(ValueError, match="magic"):
        vqvdbfile.loads_residual(b"VQVDB" + buf[5:])
    with pytest.raises(ValueError, match="version 2"):
        vqvdbfile.loads_residual(buf[:5] + b"\x02" + buf[6:])
    with pytest.raises(ValueError, match="past its last grid"):
        vqvdbfile.loads_residual(buf + b"\0")
    with pytest.raises(ValueError, match="ascending"):
        vqvdbfile.dumps_residual(0.1, [(np.array([3, 3]), raw0[:2])])
    with pytest.raises(ValueError, match="ascending"):
        vqvdbfile.loads_residual(buf[:15] + struct.pack("<I", 7) + buf[19:])       # 7, 3, 69
    with pytest.raises(ValueError, match="record indices but"):
        vqvdbfile.dumps_residual(0.1, [(ids0, raw0[:2])])


def test_fixed_order_max_is_numpys_and_sum_is_within_1e5_of_float64(leaves, recon):
    """13 chained float32 additions per leaf (7 in the lane, 6 wave levels) of non-negative terms, each term two roundings
    (difference, square): at most about (13 + 3) * 2^-24 = 9.5e-7 relative against the float64 sum of the exact differences,
    inside the issue's 1e-5."""
    assert leaves.shape == (136, 512) and recon.shape == (136, 512)
    got, ref = tbd.leaf_err_fixed(leaves, recon), tbd.leaf_err_f64(leaves, recon)
    assert got.dtype == np.float32 and got.shape == (136, 2)
    assert np.array_equal(got[:, 0], np.abs(leaves - recon).max(axis=1))
    assert (ref[:, 1] > 0).all()
    rel = np.abs(got[:, 1].astype(np.float64) - ref[:, 1]) / ref[:, 1]
    print(f"fixed-order float32 sum against float64: largest relative difference {rel.max():.2e}")
    assert rel.max() <= 1e-5
    assert (np.abs(got[:, 0].astype(np.float64) - ref[:, 0]) <= 2.0 ** -24 * np.maximum(ref[:, 0], 1.0)).all()
    # a leaf's numbers depend on that leaf only
    p = np.random.default_rng(0).permutation(136)
    assert np.array_equal(tbd.leaf_err_fixed(leaves[p], recon[p]).view(np.uint32), got[p].view(np.uint32))
    assert np.array_equal(tbd.leaf_err_fixed(leaves[7:8], recon[7:8]).view(np.uint32), got[7:8].view(np.uint32))
    # the stated voxel order, spelled out for one leaf with scalar float32 operations
    d = leaves[70] - recon[70]
    lane = []
    for L in range(64):
        vox = [4 * L + k for k in range(4)] + [256 + 4 * L + k for k in range(4)]
        q = np.float32(d[vox[0]] * d[vox[0]])
        for v in vox[1:]:
            q = np.float32(q + np.float32(d[v] * d[v]))
        lane.append(q)
    for m in (32, 16, 8, 4, 2, 1):
        lane = [np.float32(lane[i] + lane[i ^ m]) for i in range(64)]
    assert len({x.tobytes() for x in lane}) == 1 and lane[0].tobytes() == got[70, 1].tobytes()


def test_non_finite_voxels_give_a_nan_maximum(leaves, recon):
    a = tbd.leaf_err_fixed(leaves[:4], recon[:4])
    x = leaves[:4].copy()
    x[1, 100] = np.nan
    x[2, 511] = np.inf
    x[3, 0] = -np.inf
    e = tbd.leaf_err_fixed(x, recon[:4])
    assert np.array_equal(e[0].view(np.uint32), a[0].view(np.uint32))
    assert np.isnan(e[1:, 0]).all() and np.isnan(e[1, 1]) and np.isposinf(e[2:, 1]).all()
    for tol in (0.0, 1e30, float("inf")):
        assert set(tbd.select_outliers(e, tol)) >= {1, 2, 3}
    assert tbd.select_outliers(e, float("inf")).tolist() == [1, 2, 3]
    assert tbd.select_outliers(e, float("nan")).tolist() == [0, 1, 2, 3]
    z = tbd.leaf_err_fixed(leaves[:2], leaves[:2])              # exact reconstruction: zero error, not selected at tol 0
    assert not z.any() and tbd.select_outliers(z, 0.0).size == 0
    e2 = np.array([[0.5, 9], [0.25, 9], [0.25, 1]], dtype=np.float32)
    assert tbd.select_outliers(e2, 0.25).tolist() == [0]        # equality is not an outlier


class _FakeCodec(codec.HipCodec):
    """The wrapper's bookkeeping around a codec without a device: 'decode' returns a stored lossy copy of the leaves."""

    def __init__(self, leaves, noise):
        self._x = leaves
        self._rec = (leaves + noise).astype(np.float32)

    def _compress_bounded_host(self, leaves, tol):
        assert np.array_equal(leaves, self._x)
        err = tbd.leaf_err_fixed(leaves, self._rec)
        return np.zeros((len(leaves), 64), np.uint8), err, tbd.select_outliers(err, tol)

    def _decompress_bounded_host(self, indices, ids, raw):
        assert indices.dtype == np.uint8 and ids.dtype == np.int64 and raw.dtype == np.float32
        return tbd.decompress_bounded(self._rec, ids, raw)


def test_compress_decompress_bounded_honours_the_tolerance_on_a_fake_codec(leaves):
    rng = np.random.default_rng(5)
    x = np.ascontiguousarray(leaves[:64])
    noise = (rng.standard_normal(x.shape) * rng.uniform(1e-4, 1e-1, size=(64, 1))).astype(np.float32)
    noise[9] = 0.0
    fake = _FakeCodec(x, noise)
    worst = np.abs(x - fake._rec).max(axis=1)
    for tol in (float(np.median(worst)), float(worst[3]), 0.0, float("inf"), 1e-3):
        idx, ids, raw = fake.compress_bounded(x, tol)
        assert ids.dtype == np.int64 and raw.shape == (len(ids), 512) and (np.diff(ids) > 0).all()
        assert np.array_equal(ids, np.flatnonzero(~(worst <= np.float32(tol))))
        out = fake.decompress_bounded(idx, ids, raw)
        assert float(np.abs(x - out).max()) <= tol
        assert np.array_equal(out[ids], x[ids])
        keep = np.setdiff1d(np.arange(64), ids)
        assert np.array_equal(out[keep], fake._rec[keep])
    idx, ids, raw, err = fake.compress_bounded(x, float(worst[3]), return_leaf_err=True)
    assert 3 not in ids and np.array_equal(err[:, 0], worst)
    idx, ids, raw = fake.compress_bounded(x, float("nan"))
    assert np.array_equal(ids, np.arange(64)) and np.array_equal(fake.decompress_bounded(idx, ids, raw), x)


def test_wrapper_checks_its_arguments_before_any_device():
    ck = codec.HipCodec.check_bound
    assert ck(0.5) == 0.5 and ck(0) == 0.0 and ck(float("inf")) == float("inf") and np.isnan(ck(float("nan")))
    assert ck(0.1) <= 0.1 and ck(0.1) == float(np.nextafter(np.float32(0.1), np.float32(0)))   # never rounded up
    assert codec.HipCodec.check_tol(0.1) == codec.HipVec3Codec.check_tol(0.1)
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(TypeError, match="tol must be a real number"):
            ck(bad)
    for bad in (-1.0, -1e-30, float("-inf")):
        with pytest.raises(ValueError, match="tol must be >= 0"):
            ck(bad)
    x = np.zeros((2, 512), np.float32)
    fake = _FakeCodec(x, np.zeros((2, 512), np.float32))
    with pytest.raises(ValueError, match="tol must be >= 0"):
        fake.compress_bounded(x, -0.5)
    with pytest.raises(ValueError, match="tol must be >= 0"):
        fake.compress_file_bounded("a", "b", [], -0.5)
    with pytest.raises(TypeError, match="float32 numpy array"):
        fake.compress_bounded(np.zeros((2, 512), np.float64), 0.1)
    with pytest.raises(ValueError, match=r"shape \[n,512\] or \[n,8,8,8\]"):
        fake.compress_bounded(np.zeros((2, 511), np.float32), 0.1)
    with pytest.raises(ValueError, match="C-contiguous"):
        fake.compress_bounded(np.zeros((512, 2), np.float32).T, 0.1)
    assert fake.check_leaves(np.zeros((3, 8, 8, 8), np.float32)).shape == (3, 512)
    with pytest.raises(TypeError, match="float32 numpy array or a contiguous float32 torch tensor"):
        fake.roundtrip(torch.zeros((1, 512)))
    with pytest.raises(ValueError, match="leaf_err_ptr is NULL"):
        fake.roundtrip_device(1, 1, 0)
    with pytest.raises(ValueError, match="count_ptr is NULL"):
        fake.select_outliers_device(1, 1, 0.5, 1, 0)
    idx = np.zeros((2, 64), np.uint8)
    with pytest.raises(TypeError, match="uint8 numpy array"):
        fake.decompress_bounded(idx.astype(np.uint16), [], np.zeros((0, 512), np.float32))
    with pytest.raises(ValueError, match=r"shape \[n,64\] or \[n,4,4,4\]"):
        fake.decompress_bounded(np.zeros((2, 63), np.uint8), [], np.zeros((0, 512), np.float32))
    with pytest.raises(ValueError, match="outlier ids but"):
        fake.decompress_bounded(idx, [0, 1], x[:1])
    with pytest.raises(ValueError, match=r"outlier ids must be in \[0, 2\)"):
        fake.decompress_bounded(idx, [2], x[:1])
    with pytest.raises(ValueError, match=r"outlier ids must be in \[0, 2\)"):
        fake.decompress_bounded(idx, [-1], x[:1])
    with pytest.raises(ValueError, match="ascending and unique"):
        fake.decompress_bounded(idx, [1, 0], x)
    with pytest.raises(ValueError, match="ascending and unique"):
        fake.decompress_bounded(idx, [1, 1], x)
    with pytest.raises(TypeError, match="outlier ids must be integers"):
        fake.decompress_bounded(idx, [0.5], x[:1])
    with pytest.raises(TypeError, match="outlier leaves must be float32"):
        fake.decompress_bounded(idx, [0], x[:1].astype(np.float64))
    with pytest.raises(ValueError, match="512 values each"):
        fake.decompress_bounded(idx, [0], np.zeros(100, np.float32))
    assert np.array_equal(fake.decompress_bounded(idx, [1], x[:1] + 2)[1], x[0] + 2)
