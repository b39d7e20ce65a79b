"""numpy restatement of the active-voxel masks (include/vqvdb_hip_vec3_mask.h) — TEST INFRASTRUCTURE, written from the contract by its direct definition: an inactive value adds
+0.0f to both error numbers, has q = 0 and verifies without any arithmetic on it.  C = 1 is the scalar handle (leaves [n,512]),
C = 3 the Vec3 handle (leaves [n,512,3], one mask bit per voxel).  Everything unmasked (quantise, zigzag, record sizes, the
reduction orders restated once more here only so that the masked terms can enter them) comes from the existing torch_ref_* modules;
``substitute`` gives the x' = where(active, x, x^) of the substitution principle, which the tests hold against this file."""
import numpy as np

import torch_ref_rate as trt
import torch_ref_residual as trr
import torch_ref_vec3_rate as t3t
import torch_ref_vec3_residual as t3r

F = np.float32
WORDS = 8


def pack_masks(active) -> np.ndarray:
    """bool [n,512] (or [n,8,8,8]) -> uint64 [n,8]: bit L of word j of a leaf is voxel 64 j + L."""
    a = np.asarray(active, bool).reshape(-1, WORDS, 64)
    out = np.zeros(a.shape[:2], np.uint64)
    for L in range(64):
        out |= a[:, :, L].astype(np.uint64) << np.uint64(L)
    return out


def unpack_masks(masks) -> np.ndarray:
    """uint64 [n,8] -> bool [n,512]."""
    m = np.asarray(masks, np.uint64).reshape(-1, WORDS, 1)
    return ((m >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool).reshape(-1, 512)


def _values(a, C):
    return np.asarray(a, F).reshape(-1, 512) if C == 1 else np.asarray(a, F).reshape(-1, 512, 3)


def _active(active, C):
    """bool [n,512] -> the shape of the values: one bit covers the C channels of its voxel"""
    a = np.asarray(active, bool).reshape(-1, 512)
    return a if C == 1 else np.repeat(a[:, :, None], 3, axis=2)


def substitute(x, recon, active, C=1):
    """x' = where(active, x, x^)"""
    return np.where(_active(active, C), _values(x, C), _values(recon, C)).astype(F)


def leaf_err_fixed(x, recon, active, C=1) -> np.ndarray:
    """float32 [n,2] = {max |d|, sum d^2} over the active values: the sq and |d| of an inactive value are +0.0f, whatever x and x^
    hold there, and the terms go through the reduction order of the handle's unmasked error (C = 1: leaf_err_k, lane L chains the
    voxels 4L .. 4L+3, 256+4L .. 256+4L+3, then the wave halves; C = 3: final_err_k, a lane chains its three channels, a wave of
    64 consecutive voxels halves, the eight waves are chained in order)."""
    x, r, act = _values(x, C), _values(recon, C), _active(active, C)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - r
        sq = np.where(act, d * d, F(0)).astype(F)
        a = np.where(act, np.where(np.isfinite(d), np.abs(d), F(np.nan)), F(0)).astype(F)
        if C == 1:
            sq, a = sq.reshape(-1, 2, 64, 4), a.reshape(-1, 2, 64, 4)             # [leaf, load, lane, component]
            q, am = sq[:, 0, :, 0], a[:, 0, :, 0]
            for k in range(1, 8):
                q = q + sq[:, k // 4, :, k % 4]
                am = np.maximum(am, a[:, k // 4, :, k % 4])                       # np.maximum keeps NaN
            for m in (32, 16, 8, 4, 2, 1):
                q = q[:, :m] + q[:, m:2 * m]
                am = np.maximum(am[:, :m], am[:, m:2 * m])
            qs, am = q[:, 0], am[:, 0]
        else:
            q = sq[:, :, 0]
            q = q + sq[:, :, 1]
            q = q + sq[:, :, 2]
            am = np.maximum(np.maximum(a[:, :, 0], a[:, :, 1]), a[:, :, 2])
            q, am = q.reshape(-1, 8, 64), am.reshape(-1, 8, 64)
            for m in (32, 16, 8, 4, 2, 1):
                q = q[:, :, :m] + q[:, :, m:2 * m]
                am = np.maximum(am[:, :, :m], am[:, :, m:2 * m])
            q, am = q[:, :, 0], am[:, :, 0]
            qs, a8 = q[:, 0], am[:, 0]
            for k in range(1, 8):
                qs = qs + q[:, k]
                a8 = np.maximum(a8, am[:, k])
            am = a8
    assert qs.dtype == F and am.dtype == F
    return np.stack([am, qs], axis=1)


def _sentinels(C):
    return (trr.KEPT, trr.RAW) if C == 1 else (t3r.KEPT, t3r.RAW)


def record_size(code, C=1):
    return trr.record_size(code) if C == 1 else t3r.record_size(code)


def quantise(x, recon, tol, active, C=1):
    """-> (zz uint32 of every value, 0 at inactive voxels; verified bool, True at inactive voxels)"""
    act = _active(active, C)
    q, ok = trr.quantise(_values(x, C), _values(recon, C), tol)
    return np.where(act, trr.zigzag(q), np.uint32(0)).astype(np.uint32), ok | ~act


def classify(x, recon, leaf_err, tol, active, C=1):
    """-> (code [n] (uint8 classes for C = 1, uint16 codes for C = 3), offsets int64 [n+1]): kept iff leaf_err[0] <= tol; otherwise
    quantised iff every active value verifies, one width per channel from zz(q) of the active values; otherwise raw.  A selected
    leaf without active voxels therefore has code 0."""
    KEPT, RAW = _sentinels(C)
    zz, ok = quantise(x, recon, tol, active, C)
    n = len(zz)
    with np.errstate(invalid="ignore"):
        kept = np.asarray(leaf_err, F).reshape(n, -1)[:, 0] <= F(tol)
    top = zz.reshape(n, 512, C).max(axis=1) if n else np.zeros((0, C), np.uint32)
    bits = np.array([[int(v).bit_length() for v in row] for row in top], dtype=np.int64).reshape(n, C)
    quant = sum(bits[:, ch] << (5 * ch) for ch in range(C))
    code = np.where(kept, KEPT, np.where(ok.reshape(n, -1).all(axis=1), quant, RAW)).astype(np.uint8 if C == 1 else np.uint16)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(record_size(code, C), out=off[1:])
    return code, off


def _planes(zz, b):
    """the 64 * b bytes of one channel: zz uint32 [512] -> planes 0 .. b-1, eight little-endian u64 words each"""
    z = zz.astype(np.uint64).reshape(8, 64)
    words = np.zeros((int(b), 8), dtype="<u8")
    for k in range(int(b)):
        plane = (z >> np.uint64(k)) & np.uint64(1)
        words[k] = (plane << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return words.tobytes()


def pack(x, recon, tol, code, active, C=1):
    """-> payload bytes: a quantised record has the existing layout with an inactive voxel's bits 0; a raw record is the leaf's
    2048 * C bytes of x as given, inactive voxels included."""
    KEPT, RAW = _sentinels(C)
    xs = _values(x, C)
    zz, _ = quantise(x, recon, tol, active, C)
    zz = zz.reshape(len(xs), 512, C)
    out = []
    for i, c in enumerate(code):
        c = int(c)
        if c == KEPT:
            continue
        if c == RAW:
            out.append(np.ascontiguousarray(xs[i], "<f4").tobytes())
            continue
        for ch in range(C):
            out.append(_planes(zz[i, :, ch], (c >> (5 * ch)) & 31))
    return b"".join(out)


def records(code, payload, C=1):
    return trr.records(code, payload) if C == 1 else t3r.records(code, payload)


def apply(recon, tol, code, payload, C=1):
    """the existing decoder's arithmetic on masked records: nothing of it knows a mask"""
    return trr.apply(recon, tol, code, payload) if C == 1 else t3r.apply(recon, tol, code, payload)


def columns(code, C=1):
    c = np.asarray(code).astype(np.int64)
    if C == 1:
        return np.where(c == trr.KEPT, trt.KEPT_COL, np.where(c == trr.RAW, trt.RAW_COL, c))
    return t3t.columns(code)


def sweep(x, recon, leaf_err, tols, active, C=1):
    """-> hist int64 [T, 16 C + 3]: the counts of classify's codes at every rung"""
    classes = trt.CLASSES if C == 1 else t3t.CLASSES
    hist = np.zeros((len(tols), classes), np.int64)
    for t, tol in enumerate(tols):
        hist[t] = np.bincount(columns(classify(x, recon, leaf_err, tol, active, C)[0], C), minlength=classes)
    return hist


# ---- the designed input: built and checked on the CPU by tests/test_masked_host.py, reused by the GPU tests ----
TOL_D = 0.5   # step 0.9375: x = x^ + q * step and t = q are exact for the small integers below
KINDS = ("kept_by_mask", "narrower_by_mask", "raw_to_quantised", "raw_either_way", "all_inactive", "single_0", "single_63", "single_64",
         "single_511")


def designed(C=1):
    """(x, x^, active bool [9,512], kinds) at tolerance TOL_D, x^ = a small finite pattern, x = x^ + q * step:
    kept_by_mask      q = 0 at active voxels (error 0), q = 5 at some inactive ones: selected without the mask, kept with it
    narrower_by_mask  active q in -1 .. 1 with one active q = 2, an inactive q = 1000: fewer bits with the mask
    raw_to_quantised  a NaN and an over-range value (q = 40000) in inactive voxels, active q = 3: raw without, quantised with
    raw_either_way    a NaN in an active voxel
    all_inactive      every voxel inactive, q = 7 everywhere
    single_v          the one active voxel v (0, 63, 64, 511) has q = 9, every other voxel q = 300 and is inactive
    With C = 3 every channel of a voxel carries the same q but channel c of the special values is scaled by (c + 1) where that
    stays in range."""
    step = trr.step_of(TOL_D)
    n = len(KINDS)
    q = np.zeros((n, 512), np.int64)
    active = np.ones((n, 512), bool)
    rng = np.random.default_rng(21)
    active[0, 100:140] = False
    q[0, 100:140] = 5
    q[1] = rng.integers(-1, 2, 512)
    q[1, 17], q[1, 400] = 2, 1000
    active[1, 400] = False
    q[2, :] = 3
    active[2, [5, 77]] = False
    q[2, 77] = 40000
    q[3] = rng.integers(-2, 3, 512)
    active[4, :] = False
    q[4, :] = 7
    for k, v in zip((5, 6, 7, 8), (0, 63, 64, 511)):
        active[k, :] = False
        active[k, v] = True
        q[k, :] = 300
        q[k, v] = 9
    recon = (rng.integers(-8, 9, (n, 512)).astype(F) * F(0.25)).astype(F)
    x = (recon + q.astype(F) * step).astype(F)
    x[2, 5] = np.nan
    x[3, 300] = np.nan
    if C == 3:
        scale = np.array([1, 2, 3], F)
        r3 = np.repeat(recon[:, :, None], 3, axis=2).astype(F)
        q3 = q[:, :, None] * np.where(np.abs(q[:, :, None]) < 10000, scale[None, None, :], F(1))
        x3 = (r3 + q3.astype(F) * step).astype(F)
        x3[2, 5, 1] = np.nan
        x3[3, 300, 2] = np.nan
        return np.ascontiguousarray(x3), np.ascontiguousarray(r3), active, KINDS
    return np.ascontiguousarray(x), np.ascontiguousarray(recon), active, KINDS
