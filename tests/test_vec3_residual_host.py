"""Quantised residuals of the Vec3 handle without a GPU: the numpy restatement
tests/torch_ref_vec3_residual.py (the tolerance guarantee, one bit width per channel, every width in every channel, ties, the edge
tolerances, the record layout bit by bit), the C ABI of include/vqvdb_hip_vec3_residual.h (declarations, exports, bindings, NULL
handle) and the wrapper's argument checks."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_residual as trr  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import codec  # noqa: E402

HEADER = os.path.join(ROOT, "include", "vqvdb_hip_vec3_residual.h")
NAMES = ["vqhip_vec3_residual_encode_device", "vqhip_vec3_residual_apply_device", "vqhip_vec3_residual_compress", "vqhip_vec3_residual_decompress"]
ARITY = {"vqhip_vec3_residual_encode_device": 11, "vqhip_vec3_residual_apply_device": 8, "vqhip_vec3_residual_compress": 9,
         "vqhip_vec3_residual_decompress": 8}
F = np.float32


def synthetic(tol, n=1024, seed=3):
    """x^ ~ N(0,1) [n,512,3], d uniform in +-(40, 4, 400) tol per channel; the error is numpy's float32 maximum (what
    final_err_k reports for finite leaves)."""
    rng = np.random.default_rng(seed)
    recon = rng.standard_normal((n, 512, 3)).astype(F)
    scale = np.array([40.0, 4.0, 400.0], F) * F(tol)
    x = (recon + rng.uniform(-1.0, 1.0, (n, 512, 3)).astype(F) * scale).astype(F)
    err = np.abs(x - recon).reshape(n, -1).max(axis=1)
    return x, recon, np.stack([err, err], axis=1)


@pytest.mark.parametrize("tol", (0.66, 1e-3, 1e-5))
def test_restatement_keeps_the_tolerance_with_one_width_per_channel(tol):
    x, recon, err = synthetic(tol)
    code, off = t3r.classify(x, recon, err, tol)
    payload = t3r.pack(x, recon, tol, code)
    assert len(payload) == off[-1] == t3r.record_size(code).sum()
    out = t3r.apply(recon, tol, code, payload)
    worst = np.abs(x - out).reshape(len(x), -1).max(axis=1)
    selected = code != t3r.KEPT
    raw = code == t3r.RAW
    b = t3r.widths(code[selected & ~raw])
    print(f"tol {tol:g}: {selected.sum()} selected, {raw.sum()} raw, largest error {worst.max():.3g}, "
          f"{len(payload) / max(selected.sum(), 1):.0f} B per selected leaf, widths {np.unique(b, axis=0).tolist()}")
    assert np.isfinite(x).all() and (worst <= F(tol)).all()
    assert selected.sum() > 1000 and raw.sum() <= 0.01 * selected.sum()
    assert raw.sum() == 0                                            # where the reference stands: 0 of 1024
    assert np.array_equal(out[raw].view(np.uint32), x[raw].view(np.uint32))
    assert np.array_equal(out[~selected].view(np.uint32), recon[~selected].view(np.uint32))
    assert (b.sum(axis=1) < 3 * b.max(axis=1)).all()                 # a shared width would pay the widest channel three times
    assert (b == [6, 3, 9]).all(axis=1).mean() > 0.9                 # 18 planes where a shared width needs 27
    # a kept leaf among them is untouched and has no record
    err2 = err.copy()
    err2[5] = 0.0
    code2, off2 = t3r.classify(x[:8], recon[:8], err2[:8], tol)
    assert code2[5] == t3r.KEPT and off2[6] == off2[5]
    out2 = t3r.apply(recon[:8], tol, code2, t3r.pack(x[:8], recon[:8], tol, code2))
    assert np.array_equal(out2[5].view(np.uint32), recon[5].view(np.uint32))


def test_every_width_in_every_channel_and_a_seventeen_bit_channel():
    x, recon, err, w = t3r.format_leaves()
    code, off = t3r.classify(x, recon, err, 0.5)
    assert np.array_equal(t3r.widths(code), w) and (code < 0x8000).all()
    assert np.array_equal(code, w[:, 0] | w[:, 1] << 5 | w[:, 2] << 10)
    assert np.array_equal(np.diff(off), 64 * w.sum(axis=1))
    payload = t3r.pack(x, recon, 0.5, code)
    assert len(payload) == off[-1]
    out = t3r.apply(recon, 0.5, code, payload)
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32))    # exact products: the round trip is lossless here
    # the widest q that fits, +-32767: zz = 65534 / 65533, 16 bits, in each channel
    for ch in range(3):
        for neg in (False, True):
            q3, n3 = [1, 1, 1], [False] * 3
            q3[ch], n3[ch] = 32767, neg
            xe, re_ = t3r.leaf_with_max_q(q3, 0.5, negative=n3)
            c = int(t3r.classify(xe[None], re_[None], [[9.0, 0.0]], 0.5)[0][0])
            assert t3r.widths(c).tolist() == [16 if k == ch else 2 for k in range(3)]
        # 32768 needs 17 bits: that one channel sends the whole leaf to raw
        q3 = [1, 1, 1]
        q3[ch] = 32768
        xe, re_ = t3r.leaf_with_max_q(q3, 0.5)
        c, o = t3r.classify(xe[None], re_[None], [[9.0, 0.0]], 0.5)
        assert c.tolist() == [t3r.RAW] and o.tolist() == [0, 6144]
        assert t3r.pack(xe[None], re_[None], 0.5, c) == xe.tobytes()
    # 16 / 16 / 16: the largest quantised record, half a raw leaf
    xe, re_ = t3r.leaf_with_max_q([32767, 32767, 32767], 0.5, negative=[False, True, False])
    c, o = t3r.classify(xe[None], re_[None], [[9.0, 0.0]], 0.5)
    assert c.tolist() == [t3r.make_code(16, 16, 16)] and o.tolist() == [0, 3072]


@pytest.mark.parametrize("voxel,ch,q,want_code,byte,bit", (
    (0, 0, -1, 1, 0, 0),                                             # zz 1: plane 0 of channel 0, word 0, bit 0
    (511, 2, -1, 1 << 10, 7 * 8, 63),                                # plane 0 of channel 2 (no planes before it), word 7, bit 63
    (200, 1, 2, 3 << 5, (8 * 2 + 3) * 8, 8),                         # zz 4: plane 2 of channel 1, word 3 (200 = 64 * 3 + 8), bit 8
))
def test_a_single_residual_sets_exactly_one_bit(voxel, ch, q, want_code, byte, bit):
    x = np.zeros((1, 512, 3), F)
    x[0, voxel, ch] = F(q) * trr.step_of(0.5)
    code, off = t3r.classify(x, np.zeros_like(x), [[9.0, 0.0]], 0.5)
    assert code.tolist() == [want_code]
    rec = t3r.pack(x, np.zeros_like(x), 0.5, code)
    assert len(rec) == off[-1] == 64 * int(t3r.widths(want_code).sum())
    want = bytearray(len(rec))
    want[byte + bit // 8] = 1 << (bit % 8)                           # little-endian words
    assert rec == bytes(want)
    assert struct.unpack_from("<Q", rec, byte)[0] == 1 << bit
    assert np.array_equal(t3r.apply(np.zeros_like(x), 0.5, code, rec).view(np.uint32), x.view(np.uint32))


def test_record_layout_bit_by_bit():
    rng = np.random.default_rng(8)
    q = np.stack([rng.integers(-300, 301, 512), rng.integers(-3, 4, 512), rng.integers(-20000, 20001, 512)], axis=1).astype(np.int32)
    x, recon = (q.astype(F) * trr.step_of(0.5)).astype(F)[None], np.zeros((1, 512, 3), F)
    code, _ = t3r.classify(x, recon, [[300.0, 0.0]], 0.5)
    b = t3r.widths(int(code[0])).tolist()
    assert b == [int(trr.zigzag(q[:, ch]).max()).bit_length() for ch in range(3)] and b[1] == 3 and b[2] == 16 and 9 <= b[0] <= 10
    rec = t3r.pack(x, recon, 0.5, code)
    assert len(rec) == 64 * sum(b)
    for ch in range(3):
        zz = [((int(v) << 1) ^ (int(v) >> 31)) & 0xFFFFFFFF for v in q[:, ch]]
        first = 8 * sum(b[:ch])                                      # the channel's first word
        for k in range(b[ch]):
            for j in range(8):
                (word,) = struct.unpack_from("<Q", rec, (first + 8 * k + j) * 8)
                for lane in range(64):
                    assert (word >> lane) & 1 == (zz[64 * j + lane] >> k) & 1, (ch, k, j, lane)
    assert np.array_equal(t3r.unpack_leaf(rec, int(code[0])), q)


def test_code_zero_ties_and_edge_tolerances():
    # code 0: a selected leaf whose residuals all round to 0 has a record of 0 bytes
    recon = np.random.default_rng(1).standard_normal((1, 512, 3)).astype(F)
    x = recon + F(0.01)
    code, off = t3r.classify(x, recon, [[9.0, 0.0]], 0.5)
    assert code.tolist() == [0] and off.tolist() == [0, 0] and t3r.pack(x, recon, 0.5, code) == b""
    assert np.array_equal(t3r.apply(recon, 0.5, code, b""), recon + F(0) * trr.step_of(0.5))
    # ties round to even, in every channel
    x = np.zeros((1, 512, 3), F)
    halves = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 1e3 + 0.5], F)
    for ch in range(3):
        x[0, 8 * ch:8 * ch + 8, ch] = halves * trr.step_of(0.5)      # exact: t = the halves
    q, ok = t3r.quantise(x, np.zeros_like(x), 0.5)
    for ch in range(3):
        assert q[0, 8 * ch:8 * ch + 8, ch].tolist() == [0, 2, 2, 4, 0, -2, -2, 1000]
    assert ok.all() and q.shape == (1, 512, 3)                       # half a step is 0.9375 tol: a tie stays within the tolerance
    # tol 0 and NaN: every leaf raw; tol +inf: every finite leaf kept
    x, recon, err = synthetic(0.66, n=16)
    for tol in (0.0, float("nan")):
        code, off = t3r.classify(x, recon, err, tol)
        assert (code == t3r.RAW).all() and off[-1] == 16 * 6144
        assert t3r.pack(x, recon, tol, code) == x.tobytes()
        assert np.array_equal(t3r.apply(recon, tol, code, x.tobytes()).view(np.uint32), x.view(np.uint32))
    code, off = t3r.classify(x, recon, err, float("inf"))
    assert (code == t3r.KEPT).all() and off[-1] == 0 and t3r.pack(x, recon, float("inf"), code) == b""
    # a non-finite value: the reported error is NaN, the leaf is selected at every tolerance and raw, NaN payload included
    bad = x.copy()
    bad.view(np.uint32)[3, 100, 1] = 0x7FC12345
    bad[5, 7, 2] = -np.inf
    berr = err.copy()
    berr[[3, 5], 0] = np.nan
    for tol in (0.66, 1e30, float("inf")):
        code, _ = t3r.classify(bad, recon, berr, tol)
        assert code[3] == t3r.RAW and code[5] == t3r.RAW
    code, off = t3r.classify(bad, recon, berr, float("inf"))
    assert (code == t3r.KEPT).sum() == 14
    out = t3r.apply(recon, float("inf"), code, t3r.pack(bad, recon, float("inf"), code))
    assert np.array_equal(out[[3, 5]].view(np.uint32), bad[[3, 5]].view(np.uint32))


def test_header_library_and_bindings_hold_exactly_the_vec3_residual_names():
    assert codec.VEC3_RESIDUAL_SYMBOLS == NAMES
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(NAMES)
    assert re.search(r"#define\s+VQHIP_VEC3_RES_KEPT\s+0xFFFE\b", text) and re.search(r"#define\s+VQHIP_VEC3_RES_RAW\s+0xFFFF\b", text)
    assert (codec.VEC3_RES_KEPT, codec.VEC3_RES_RAW) == (0xFFFE, 0xFFFF) == (t3r.KEPT, t3r.RAW)
    for name in NAMES:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert params.count(",") + 1 == ARITY[name], name
    for other in (codec.ABI_SYMBOLS, codec.VEC3_TRAIN_SYMBOLS, codec.VEC3_FULLTRAIN_SYMBOLS, codec.VEC3_PRECISION_SYMBOLS, codec.VEC3_BOUNDED_SYMBOLS,
                  codec.BOUNDED_SYMBOLS, codec.RESIDUAL_SYMBOLS):
        assert not set(NAMES) & set(other)
    for h in ("vqvdb_hip.h", "vqvdb_hip_vec3_bounded.h", "vqvdb_hip_residual.h"):
        other = open(os.path.join(ROOT, "include", h)).read()
        for name in NAMES:
            assert not re.search(r"\b" + name + r"\s*\(", other), (h, name)
    lib = codec.load_library()
    for name in NAMES:
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == ARITY[name] and f.restype == ctypes.c_int, name
    assert lib.vqhip_vec3_residual_encode_device.argtypes[5] == ctypes.c_float and lib.vqhip_vec3_residual_apply_device.argtypes[3] == ctypes.c_float
    assert lib.vqhip_vec3_residual_compress.argtypes[3] == ctypes.c_float and lib.vqhip_vec3_residual_decompress.argtypes[3] == ctypes.c_float
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r"\b(vqhip_\w+)\b", out))
    # a NULL handle is refused by every call, without a device
    assert lib.vqhip_vec3_residual_encode_device(None, None, None, None, 1, 0.5, None, None, None, 0, None) == -1
    assert lib.vqhip_vec3_residual_apply_device(None, None, 1, 0.5, None, None, None, None) == -1
    assert lib.vqhip_vec3_residual_compress(None, None, 1, 0.5, None, None, None, None, None) == -1
    assert lib.vqhip_vec3_residual_decompress(None, None, 1, 0.5, None, None, 0, None) == -1


def test_wrapper_checks_its_arguments_before_any_device():
    H = codec.HipVec3Codec
    fake = object.__new__(H)                                         # no handle: every check below runs before the library is called
    x, idx = np.zeros((2, 512, 3), F), np.zeros((2, 64), np.uint16)
    kept = np.full(2, 0xFFFE, np.uint16)
    for bad in ("1", None, True):
        with pytest.raises(TypeError, match="tol must be a real number"):
            fake.compress_residual(x, bad)
        with pytest.raises(TypeError, match="tol must be a real number"):
            fake.decompress_residual(idx, bad, kept, b"")
        with pytest.raises(TypeError, match="tol must be a real number"):
            fake.residual_encode_device(1, 1, 1, 2, bad, 1, 1, 1, 0)
        with pytest.raises(TypeError, match="tol must be a real number"):
            fake.residual_apply_device(1, 2, bad, 1, 1, 1)
    with pytest.raises(TypeError, match="float32"):
        fake.compress_residual(x.astype(np.float64), 0.5)
    with pytest.raises(ValueError, match="shape"):
        fake.compress_residual(np.zeros((2, 512), F), 0.5)
    with pytest.raises(TypeError, match="uint16"):
        fake.decompress_residual(idx.astype(np.uint8), 0.5, kept, b"")
    with pytest.raises(TypeError, match="leaf_code must be a uint16"):
        fake.decompress_residual(idx, 0.5, [0xFFFE, 0xFFFE], b"")
    with pytest.raises(TypeError, match="leaf_code must be a uint16"):
        fake.decompress_residual(idx, 0.5, kept.astype(np.uint8), b"")
    with pytest.raises(ValueError, match="2 leaves but 3 codes"):
        fake.decompress_residual(idx, 0.5, np.full(3, 0xFFFE, np.uint16), b"")
    for bad in (17, 17 << 5, 17 << 10, 31 << 10, 0x8000, 0x8000 | 3, 0xFFFD):   # a field of 17, bit 15 on a code that is no sentinel
        with pytest.raises(ValueError, match="leaf codes must be"):
            fake.decompress_residual(idx, 0.5, np.array([bad, 0xFFFE], np.uint16), b"")
        with pytest.raises(ValueError, match="leaf codes must be"):
            H.residual_record_sizes(np.array([bad], np.uint16))
    with pytest.raises(ValueError, match="need 6464 payload bytes, got 64"):
        fake.decompress_residual(idx, 0.5, np.array([t3r.make_code(1, 1, 3), 0xFFFF], np.uint16), bytes(64))
    with pytest.raises(TypeError, match="payload must be bytes"):
        fake.decompress_residual(idx, 0.5, np.array([1, 0xFFFE], np.uint16), np.zeros(64, np.int8))
    with pytest.raises(ValueError, match="NULL device pointer"):
        fake.residual_encode_device(1, 0, 1, 2, 0.5, 1, 1, 1, 0)
    with pytest.raises(ValueError, match="payload_capacity"):
        fake.residual_encode_device(1, 1, 1, 2, 0.5, 1, 1, 1, -1)
    with pytest.raises(ValueError, match="NULL device pointer"):
        fake.residual_apply_device(1, 2, 0.5, 0, 1, 1)
    lc, pl = H.check_residual(3, np.array([0, 0xFFFE, 2 << 5], np.uint16), bytes(128))
    assert lc.dtype == np.uint16 and pl.dtype == np.uint8 and len(pl) == 128
    codes = np.array([0, 1, 16, 1 << 5, 16 << 10, t3r.make_code(6, 3, 9), t3r.make_code(16, 16, 16), 0xFFFE, 0xFFFF], np.uint16)
    assert H.residual_record_sizes(codes).tolist() == [0, 64, 1024, 64, 1024, 1152, 3072, 0, 6144]
    every = np.array([t3r.make_code(a, b, c) for a in range(17) for b in (0, 7, 16) for c in (0, 1, 16)] + [0xFFFE, 0xFFFF], np.uint16)
    assert np.array_equal(H.residual_record_sizes(every), t3r.record_size(every))
