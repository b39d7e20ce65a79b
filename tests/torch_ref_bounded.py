"""Numpy restatement of the scalar handle's error-bounded round trip (include/vqvdb_hip_bounded.h) — TEST
INFRASTRUCTURE.  The per-leaf error of a reconstruction in leaf_err_k's stated order (float32, to the bit) and in float64, the
selection rule, and the bookkeeping of compress_bounded / decompress_bounded."""
from __future__ import annotations

import numpy as np


def _leaves(a) -> np.ndarray:
    return np.asarray(a).reshape(-1, 512)


def leaf_err_fixed(x, recon) -> np.ndarray:
    """float32 [n,2] = {max |d|, sum d^2}, d = x - recon in float32, in leaf_err_k's order (vqvdb_amd/csrc/vq_bounded.h):
    lane L of 64 chains its eight voxels 4L .. 4L+3, 256+4L .. 256+4L+3 in that order; the wave halves 64 -> 32 -> ... -> 1
    (lane i + lane i+m, what the xor butterfly with masks 32..1 leaves in lane 0).  Every product and sum is a rounded float32
    operation of its own; a non-finite |d| counts as NaN and the maximum keeps NaN."""
    x, r = _leaves(x).astype(np.float32), _leaves(recon).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - r
        sq = (d * d).reshape(-1, 2, 64, 4)                    # [leaf, load, lane, component]: voxel = load*256 + lane*4 + component
        a = np.where(np.isfinite(d), np.abs(d), np.float32(np.nan)).reshape(-1, 2, 64, 4)
        q, am = sq[:, 0, :, 0], a[:, 0, :, 0]
        for k in range(1, 8):
            q = q + sq[:, k // 4, :, k % 4]
            am = np.maximum(am, a[:, k // 4, :, k % 4])       # np.maximum keeps NaN
        for m in (32, 16, 8, 4, 2, 1):
            q = q[:, :m] + q[:, m:2 * m]
            am = np.maximum(am[:, :m], am[:, m:2 * m])
    q, am = q[:, 0], am[:, 0]
    assert q.dtype == np.float32 and am.dtype == np.float32
    return np.stack([am, q], axis=1)


def leaf_err_f64(x, recon) -> np.ndarray:
    """float64 [n,2] = {max |d|, sum d^2} of the exact differences of the float32 inputs."""
    d = _leaves(x).astype(np.float64) - _leaves(recon).astype(np.float64)
    return np.stack([np.abs(d).max(axis=1), (d * d).sum(axis=1)], axis=1)


def select_outliers(leaf_err, tol) -> np.ndarray:
    """Ascending ids of the leaves with !(max error <= tol): equality stays in, NaN (error or tol) selects."""
    e = np.asarray(leaf_err, dtype=np.float32).reshape(-1, 2)[:, 0]
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~(e <= np.float32(tol))).astype(np.int64)


def compress_bounded(x, recon, tol):
    """(outlier_ids, outlier_leaves) of leaves x whose reconstruction is recon."""
    ids = select_outliers(leaf_err_fixed(x, recon), tol)
    return ids, _leaves(x)[ids].copy()


def decompress_bounded(recon, outlier_ids, outlier_leaves) -> np.ndarray:
    out = _leaves(recon).copy()
    out[np.asarray(outlier_ids, dtype=np.int64)] = outlier_leaves
    return out
