"""numpy restatement of the size sweep (include/vqvdb_hip_rate.h): the class histogram of a batch of leaves at
every rung of a tolerance ladder, as counts of tests/torch_ref_residual.classify, the payload and .vqres v2 sidecar sizes that
follow from a histogram row, and the choice of the tightest rung within a byte budget."""
import numpy as np

import torch_ref_residual as trr

CLASSES, RAW_COL, KEPT_COL = 19, 17, 18


def sweep(x, recon, err, tols):
    """-> hist int64 [T,19]: hist[t, k] = the leaves of class k at tols[t]; columns 0 .. 16 quantised, 17 raw (255), 18 kept (254)."""
    hist = np.zeros((len(tols), CLASSES), np.int64)
    for t, tol in enumerate(tols):
        cls = trr.classify(x, recon, err, tol)[0].astype(np.int64)
        col = np.where(cls == trr.KEPT, KEPT_COL, np.where(cls == trr.RAW, RAW_COL, cls))
        hist[t] = np.bincount(col, minlength=CLASSES)
    return hist


def payload_bytes(row):
    row = np.asarray(row, np.int64)
    return int((64 * np.arange(17) * row[:17]).sum() + 2048 * row[RAW_COL])


def sidecar_bytes(row, n_grids):
    """file header 11, a count of 4 per grid, {u32 index, u8 class} per selected leaf, the records."""
    return 11 + 4 * int(n_grids) + 5 * int(np.asarray(row, np.int64)[:18].sum()) + payload_bytes(row)


def pick(hist, tols, n_grids, budget):
    """-> the index of the smallest tols[t] by value whose sidecar fits the budget; NaN rungs are never chosen; ValueError if none fits."""
    best = None
    for t, tol in enumerate(tols):
        if np.isnan(tol) or sidecar_bytes(hist[t], n_grids) > budget:
            continue
        if best is None or tol < tols[best]:
            best = t
    if best is None:
        raise ValueError(f"no rung fits {budget} bytes")
    return best
