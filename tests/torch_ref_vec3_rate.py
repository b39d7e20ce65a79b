"""numpy restatement of the Vec3 handle's size sweep (include/vqvdb_hip_vec3_rate.h): the histogram of a batch of
leaves over their record sizes at every rung of a tolerance ladder, as counts of tests/torch_ref_vec3_residual.classify, the
payload size that follows from a histogram row, and the choice of the tightest rung within a byte budget."""
import numpy as np

import torch_ref_vec3_residual as t3r

CLASSES, RAW_COL, KEPT_COL = 51, 49, 50


def columns(code):
    """codes of classify -> the histogram's columns: b0 + b1 + b2 of a quantised leaf, 49 raw, 50 kept."""
    c = np.asarray(code).astype(np.int64)
    return np.where(c == t3r.KEPT, KEPT_COL, np.where(c == t3r.RAW, RAW_COL, t3r.widths(c).sum(axis=-1)))


def sweep(x, recon, err, tols):
    """-> hist int64 [T,51]: hist[t, s] = the leaves whose record at tols[t] has s planes; column 49 raw, column 50 kept."""
    hist = np.zeros((len(tols), CLASSES), np.int64)
    for t, tol in enumerate(tols):
        hist[t] = np.bincount(columns(t3r.classify(x, recon, err, tol)[0]), minlength=CLASSES)
    return hist


def payload_bytes(row):
    row = [int(v) for v in np.asarray(row).reshape(CLASSES)]          # Python integers: no overflow whatever the counts
    return sum(64 * s * row[s] for s in range(RAW_COL)) + t3r.RAW_BYTES * row[RAW_COL]


def pick(hist, tols, budget):
    """-> the index of the smallest tols[t] by value whose payload fits the budget (the first of equal rungs); NaN rungs are
    never chosen; ValueError if none fits."""
    best = None
    for t, tol in enumerate(tols):
        if np.isnan(tol) or payload_bytes(hist[t]) > budget:
            continue
        if best is None or tol < tols[best]:
            best = t
    if best is None:
        raise ValueError(f"no rung fits {budget} bytes")
    return best


def every_column_leaves(tol=0.5):
    """(x, x^, err) whose row at ``tol`` has every one of the 51 columns >= 1, without a model (x^ = 0, x = q * step; with tol 0.5
    every product is exact): 49 leaves of the widths (min(s, 16), min(max(s - 16, 0), 16), max(s - 32, 0)), s = 0 .. 48, selected
    by a reported error of 9 tol; a leaf with one 17-bit channel and a leaf with a NaN value (both raw; the NaN leaf reports a
    NaN error); and a leaf whose reported error equals tol (kept: equality keeps)."""
    xs = []
    for s in range(49):
        q = [t3r.qmax_of_width(b) for b in (min(s, 16), min(max(s - 16, 0), 16), max(s - 32, 0))]
        xs.append(t3r.leaf_with_max_q([abs(v) for v in q], tol, np.random.default_rng(s), negative=[v < 0 for v in q])[0])
    xs.append(t3r.leaf_with_max_q([3, 32768, 3], tol, np.random.default_rng(49))[0])
    nan_leaf = xs[20].copy()
    nan_leaf[300, 1] = np.nan
    xs += [nan_leaf, xs[7].copy()]
    x = np.ascontiguousarray(np.stack(xs), t3r.F)
    err = np.full((len(x), 2), 9.0 * tol, t3r.F)
    err[50], err[51] = np.nan, tol
    return x, np.zeros_like(x), err
