"""Size sweep of the scalar handle on the GPU: the histogram of rate_sweep_device against tests/torch_ref_rate.py
and against the classes residual_encode_device itself returns, invariance under batch, place, stream and split, every class, the
host and file sweeps, and rate_compress_file against compress_file_residual byte for byte.  Every comparison is exact.  Every case
runs with the automatic small-batch kernels and with set_small_batch_tiles(0), on the 136 leaves of tests/test_gpu_residual.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_rate as trt  # noqa: E402
import torch_ref_residual as trr  # noqa: E402
from test_gpu_residual import N, SIZES, TOL_S, cat, codec, dev_encode, dev_roundtrip, grids_of, leaves, pack, same, synthetic_leaves  # noqa: E402,F401
from vqvdb_amd.codec import RATE_CLASSES, HipCodec, rate_payload_bytes, rate_sidecar_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -(1 << 40) - 7


def columns(cls):
    """classes of residual_encode_device -> the histogram's columns"""
    c = np.asarray(cls).astype(np.int64)
    return np.where(c == trr.KEPT, trt.KEPT_COL, np.where(c == trr.RAW, trt.RAW_COL, c))


def counts(cls):
    return np.bincount(columns(cls), minlength=RATE_CLASSES)


class Resident:
    """leaves, reconstruction and errors on the device, swept in slices"""

    def __init__(self, x, recon, err):
        self.x, self.r = torch.from_numpy(np.ascontiguousarray(x, F)).cuda(), torch.from_numpy(np.ascontiguousarray(recon, F)).cuda()
        self.e = torch.from_numpy(np.ascontiguousarray(err, F)).cuda()

    def sweep(self, codec, tols, lo=0, n=None, hist=None, stream=None, rows=None):
        n = len(self.x) - lo if n is None else n
        if hist is None:
            hist = torch.zeros((len(tols) if rows is None else rows, RATE_CLASSES), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        codec.rate_sweep_device(self.x[lo:].data_ptr(), self.r[lo:].data_ptr(), self.e[lo:].data_ptr(), n, tols, hist.data_ptr(),
                                stream.cuda_stream if stream is not None else 0)
        torch.cuda.synchronize()
        return hist


def ladder(err):
    e = err[:, 0]
    return [0.0, float(e.min()), float(np.quantile(e, 0.25, method="lower")), float(np.median(e)), float(e.max()), float("inf"), float("nan")]


def test_sweep_device_equals_the_restatement_and_the_encoder_on_model_output(codec, leaves):
    _, err, rec = dev_roundtrip(codec, leaves)
    tols = ladder(err)
    dev = Resident(leaves, rec, err)
    hist = dev.sweep(codec, tols).cpu().numpy()
    assert np.array_equal(hist, trt.sweep(leaves, rec, err, tols)), hist
    cls = np.stack([dev_encode(codec, leaves, rec, err, tol)[0] for tol in tols])   # [T,N]: what the encoder itself says at each rung
    for t in range(len(tols)):
        assert np.array_equal(hist[t], counts(cls[t])), tols[t]
    assert (hist.sum(axis=1) == N).all()
    assert hist[3, :18].sum() == 68 and hist[3, 18] == 68            # the median rung selects half, as the residual tests' fixture does
    assert hist[6, 17] == N and hist[4, 18] == N and hist[5, 18] == N   # NaN: every leaf raw; the largest error and +inf: every leaf kept
    for n in SIZES:                                                  # every batch size, place and stream
        for lo, stream in ((0, None), (N - n, torch.cuda.Stream())):
            got = dev.sweep(codec, tols, lo, n, stream=stream).cpu().numpy()
            assert np.array_equal(got, np.stack([counts(c[lo:lo + n]) for c in cls])), (n, lo)
    both = dev.sweep(codec, tols, 0, N // 2)                         # two calls on the two halves add up to the one call
    both = dev.sweep(codec, tols, N // 2, N - N // 2, hist=both).cpu().numpy()
    assert np.array_equal(both, hist)
    full = torch.full((64, RATE_CLASSES), SENTINEL, dtype=torch.int64, device="cuda")   # the call adds, and only to its own rows
    full = dev.sweep(codec, tols, hist=full).cpu().numpy()
    assert np.array_equal(full[:len(tols)], hist + SENTINEL) and (full[len(tols):] == SENTINEL).all()
    one = dev.sweep(codec, tols[3:4], rows=64).cpu().numpy()
    assert np.array_equal(one[0], hist[3]) and not one[1:].any()
    med = tols[3]
    many = [float(v) for v in np.geomspace(med / 64, med * 8, 57).astype(F)] + tols
    assert len(many) == 64
    got = dev.sweep(codec, many).cpu().numpy()
    assert np.array_equal(got, trt.sweep(leaves, rec, err, many))
    assert len({r.tobytes() for r in got}) > 20                      # the rungs do differ
    lib, h = codec._lib, codec._h
    t1 = np.array([0.5], F)
    assert lib.vqhip_rate_sweep_device(h, None, None, None, 0, t1.ctypes.data, 1, None, None) == 0
    for bad in (0, 65, -1):
        assert lib.vqhip_rate_sweep_device(h, dev.x.data_ptr(), dev.r.data_ptr(), dev.e.data_ptr(), N, t1.ctypes.data, bad, both.ctypes.data, None) == -1
        assert "n_tols" in lib.vqhip_last_error(h).decode()
    assert lib.vqhip_rate_sweep_device(h, dev.x.data_ptr(), None, dev.e.data_ptr(), N, t1.ctypes.data, 1, None, None) == -1
    assert "null pointer" in lib.vqhip_last_error(h).decode()
    assert np.array_equal(dev.sweep(codec, tols).cpu().numpy(), hist)   # the handle still works


def every_class_ladder():
    """64 rungs: TOL_S first, its neighbours times 2^+-k, 0 and +inf"""
    tols = [TOL_S] + [float(F(TOL_S) * F(2.0) ** k) for k in range(-31, 32) if k != 0][:61] + [0.0, float("inf")]
    assert len(tols) == 64
    return tols


def test_sweep_device_with_every_class(codec):
    x, recon, err = synthetic_leaves()
    tols = every_class_ladder()
    got = Resident(x, recon, err).sweep(codec, tols).cpu().numpy()
    assert np.array_equal(got, trt.sweep(x, recon, err, tols))
    assert got[0, :17].tolist() == [1] * 17 and got[0, 17] == 4 and got[0, 18] == 0
    # more than two scan steps of 8192 leaves, kept leaves in between, every class at changing places: every column counts
    n = 2 * 8192 + 1500
    rng = np.random.default_rng(4)
    pick = rng.integers(0, len(x), n)
    bx, br, be = x[pick], recon[pick], err[pick].copy()
    keep = rng.random(n) < 0.4
    keep[8000:8400] = True
    keep[16380:16390] = False
    be[keep & np.isfinite(be[:, 0])] = 0.25
    got = Resident(bx, br, be).sweep(codec, tols).cpu().numpy()
    # the restatement once per distinct (leaf, error) pair instead of once per pick: a class depends on the leaf and its error alone
    ux, ur, ue = np.concatenate([x, x]), np.concatenate([recon, recon]), np.concatenate([err, np.full_like(err, 0.25)])
    which = pick + len(x) * (keep & np.isfinite(err[pick][:, 0]))
    weight = np.bincount(which, minlength=len(ux))
    want = np.zeros_like(got)
    for t, tol in enumerate(tols):
        np.add.at(want[t], columns(trr.classify(ux, ur, ue, tol)[0]), weight)
    assert np.array_equal(got, want)
    assert (got.sum(axis=1) == n).all() and (got[0] > 0).all() and got[0, 18] > 5000, got[0]
    cls = dev_encode(codec, bx, br, be, TOL_S)[0]                    # ... and the encoder agrees on the whole batch
    assert np.array_equal(got[0], counts(cls))


def test_sweep_device_on_unsorted_ladders_without_zero_and_with_a_nan_rung(codec):
    """The shortcut "kept at every rung" beside finite rungs only, then switched off by a NaN rung.  Ladder A: unsorted, the
    smallest rung (0.3) neither first nor last, no 0.0 and no NaN, so the leaves whose error is 0.25 take the shortcut and are
    counted by lanes 0 .. 4; ladder B: A with a NaN rung in the middle."""
    x, recon, err = synthetic_leaves()
    x, recon, err = np.concatenate([x, x]), np.concatenate([recon, recon]), np.concatenate([err, err])
    n = len(x)
    forced = (np.arange(n) % 3 == 1) & np.isfinite(err[:, 0])
    err[forced] = 0.25
    assert n == 42 and forced.sum() >= 12 and np.isnan(err[:, 0]).any()
    a = [TOL_S, float(F(0.75) * F(TOL_S)), float(F(4) * F(TOL_S)), float(F(0.3)), float("inf")]
    b = a[:2] + [float("nan")] + a[2:]
    assert min(a) == a[3] > 0.25
    want_a, want_b = trt.sweep(x, recon, err, a), trt.sweep(x, recon, err, b)
    assert (want_a[:, 18] >= forced.sum()).all() and want_a[3, 18] == forced.sum() < want_a[2, 18] < n   # the case tests something
    dev = Resident(x, recon, err)
    got_a, got_b = dev.sweep(codec, a).cpu().numpy(), dev.sweep(codec, b).cpu().numpy()
    assert np.array_equal(got_a, want_a), got_a
    assert np.array_equal(got_b, want_b), got_b
    assert (got_a.sum(axis=1) == n).all() and (got_b.sum(axis=1) == n).all()
    assert got_b[2, 17] == n                                         # the NaN rung: every leaf raw
    assert np.array_equal(np.delete(got_b, 2, axis=0), got_a)        # ... and every other rung as without it


def test_rate_sweep_on_host_leaves_at_two_chunk_sizes(codec, pack, leaves):
    _, err, rec = dev_roundtrip(codec, leaves)
    tols = ladder(err)
    want = trt.sweep(leaves, rec, err, tols)
    before = codec.compress_residual(leaves, tols[3], return_leaf_err=True)
    hist = codec.rate_sweep(leaves, tols)
    assert hist.dtype == np.int64 and np.array_equal(hist, want)
    assert np.array_equal(codec.rate_sweep(leaves[:33], tols), trt.sweep(leaves[:33], rec[:33], err[:33], tols))
    assert not codec.rate_sweep(leaves[:0], tols).any()
    after = codec.compress_residual(leaves, tols[3], return_leaf_err=True)
    assert all(same(a, b) for a, b in zip(before, after))           # indices, classes, payload and errors: unchanged by having swept
    assert np.array_equal(counts(after[1]), hist[3])
    small = HipCodec(pack)                                           # chunks of 32, 32, 32, 32, 8 add up to the same histogram
    try:
        small.set_chunk_leaves(32)
        assert np.array_equal(small.rate_sweep(leaves, tols), want)
    finally:
        small.close()


def test_rate_sweep_file_predicts_every_compress_to_the_byte(codec, leaves, tmp_path, monkeypatch):
    _, err, rec = dev_roundtrip(codec, leaves)
    tols = ladder(err)
    grids = grids_of(leaves)
    want = trt.sweep(leaves, rec, err, tols)
    monkeypatch.chdir(tmp_path)
    for batch in (32, 0):
        hist, st = codec.rate_sweep_file(grids, tols, batch_leaves=batch)
        assert np.array_equal(hist, want), batch
        assert st["leaves"] == N and st["grids"] == 2
    assert os.listdir(tmp_path) == []                                # the sweep creates no file
    for t, tol in enumerate(tols):
        lossy, res = tmp_path / f"t{t}.vqvdb", tmp_path / f"t{t}.vqres"
        _, bst, rst = codec.compress_file_residual(lossy, res, grids, tol, batch_leaves=32)
        assert os.path.getsize(res) == rate_sidecar_bytes(hist[t], 2) == trt.sidecar_bytes(hist[t], 2), tol
        assert rst["payload_bytes"] == rate_payload_bytes(hist[t]), tol
        assert rst["quantised"] == hist[t, :17].sum() and rst["raw"] == hist[t, 17] and bst["outliers"] == hist[t, :18].sum(), tol
    lib, h = codec._lib, codec._h
    t1, h1 = np.array([0.5], F), np.zeros(19, np.int64)
    assert lib.vqhip_rate_sweep_file(h, None, 2, 0, t1.ctypes.data, 1, h1.ctypes.data, None) == -1 and "null" in lib.vqhip_last_error(h).decode()
    with pytest.raises(RuntimeError, match="1..255 grids"):
        codec.rate_sweep_file([], tols)


def test_rate_compress_file_fits_the_budget_and_equals_the_compress_at_its_tolerance(codec, leaves, tmp_path):
    _, err, rec = dev_roundtrip(codec, leaves)
    tols = ladder(err)
    grids = grids_of(leaves)
    hist0, _ = codec.rate_sweep_file(grids, tols, batch_leaves=32)
    sizes = [rate_sidecar_bytes(r, 2) for r in hist0]
    budget = sizes[3]                                                # what the median rung needs
    plain, lossy, res, ref, refres = (tmp_path / f for f in ("plain.vqvdb", "b.vqvdb", "b.vqres", "ref.vqvdb", "ref.vqres"))
    tol_used, hist, st, bst, rst = codec.rate_compress_file(lossy, res, grids, tols, budget, batch_leaves=32)
    t = trt.pick(hist0, np.array(tols, F), 2, budget)
    assert np.array_equal(hist, hist0) and tol_used == HipCodec.check_tol(tols[t]) and tol_used <= HipCodec.check_tol(tols[3])
    assert all(s > budget for s, v in zip(sizes, tols) if v < tol_used)   # no smaller rung fits
    rstats = codec.compress_file_residual(ref, refres, grids, tol_used, batch_leaves=32)
    assert lossy.read_bytes() == ref.read_bytes() and res.read_bytes() == refres.read_bytes()
    assert (bst, rst) == rstats[1:] and st["leaves"] == N
    codec.compress_file(plain, grids, batch_leaves=32)
    assert lossy.read_bytes() == plain.read_bytes()
    assert os.path.getsize(res) == sizes[t] <= budget
    out = cat(codec.decompress_file_residual(lossy, res, batch_leaves=32)[0])
    assert np.isfinite(leaves).all() and np.abs(leaves - out).max() <= F(tol_used)
    # one byte under the smallest size any rung reaches: refused with both numbers, before a file is opened
    finite = [s for s, v in zip(sizes, tols) if not np.isnan(v)]
    no1, no2 = tmp_path / "no.vqvdb", tmp_path / "no.vqres"
    with pytest.raises(RuntimeError) as refusal:
        codec.rate_compress_file(no1, no2, grids, tols, min(finite) - 1, batch_leaves=32)
    assert str(min(finite)) in str(refusal.value) and str(min(finite) - 1) in str(refusal.value)
    assert not no1.exists() and not no2.exists()
    # a second round refines between the rung that did not fit and the chosen one: never a larger tolerance, still within the budget
    two1, two2 = tmp_path / "two.vqvdb", tmp_path / "two.vqres"
    budget2 = (sizes[2] + sizes[3]) // 2                             # between the sizes of two neighbouring rungs
    tol1 = codec.rate_compress_file(two1, two2, grids, tols, budget2, batch_leaves=32)[0]
    size1 = os.path.getsize(two2)
    tol2, hist2, _, _, _ = codec.rate_compress_file(two1, two2, grids, tols, budget2, batch_leaves=32, rounds=2)
    print(f"budget {budget2}: one round tol {tol1:.5f} ({size1} B), two rounds tol {tol2:.5f} ({os.path.getsize(two2)} B)")
    assert tol2 <= tol1 and os.path.getsize(two2) <= budget2 and hist2.shape == (64, 19)
    assert same(cat(codec.decompress_file_residual(lossy, res, batch_leaves=32)[0]), out)   # the handle still works
