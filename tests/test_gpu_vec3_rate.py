"""Size sweep of the Vec3 handle on the GPU: the histogram of rate_sweep_device against
tests/torch_ref_vec3_rate.py and against the codes residual_encode_device itself returns, invariance under batch, place, stream
and split, every column with the stride loop of the capped grid, the host sweep, rate_compress against compress_residual byte for
byte, and the untouched neighbours.  Every comparison is exact.  Both precision modes, on the 136 leaves of
tests/test_gpu_vec3_residual.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3_rate as t3t  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from test_gpu_vec3_residual import N, SIZES, codec, dev_encode, dev_roundtrip, leaves, pack, same  # noqa: E402,F401
from vqvdb_amd.codec import VEC3_RATE_CLASSES, HipVec3Codec, vec3_rate_payload_bytes, vec3_rate_pick  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -(1 << 40) - 7
FILL = 0xA5
TOL_S = 0.5


def counts(code):
    return np.bincount(HipVec3Codec.rate_columns(code), minlength=VEC3_RATE_CLASSES)


class Resident:
    """leaves, reconstruction and errors on the device, swept in slices"""

    def __init__(self, x, recon, err):
        self.x, self.r = torch.from_numpy(np.ascontiguousarray(x, F)).cuda(), torch.from_numpy(np.ascontiguousarray(recon, F)).cuda()
        self.e = torch.from_numpy(np.ascontiguousarray(err, F)).cuda()

    def sweep(self, codec, tols, lo=0, n=None, hist=None, stream=None, rows=None):
        n = len(self.x) - lo if n is None else n
        if hist is None:
            hist = torch.zeros((len(tols) if rows is None else rows, VEC3_RATE_CLASSES), dtype=torch.int64, device="cuda")
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
    assert np.isfinite(err).all()
    tols = ladder(err)
    dev = Resident(leaves, rec, err)
    hist = dev.sweep(codec, tols).cpu().numpy()
    assert np.array_equal(hist, t3t.sweep(leaves, rec, err, tols)), hist
    code = np.stack([dev_encode(codec, leaves, rec, err, tol)[0] for tol in tols])   # [T,N]: what the encoder itself says at each rung
    for t in range(len(tols)):
        assert np.array_equal(hist[t], counts(code[t])), tols[t]
    assert (hist.sum(axis=1) == N).all()
    assert hist[0, 49] == (err[:, 0] > 0).sum() and hist[0, :49].sum() == 0   # tol 0 quantises nothing: raw, or kept where the error is 0
    assert hist[6, 49] == N and hist[4, 50] == N and hist[5, 50] == N   # NaN: every leaf raw; the largest error and +inf: every leaf kept
    assert 0 < hist[3, :50].sum() <= 68 and hist[3, :49].sum() > 0   # the median rung selects about half and quantises
    for n in SIZES:                                                  # every batch size, place and stream
        for lo, stream in ((0, None), (N - n, torch.cuda.Stream())):
            got = dev.sweep(codec, tols, lo, n, stream=stream).cpu().numpy()
            assert np.array_equal(got, np.stack([counts(c[lo:lo + n]) for c in code])), (n, lo)
    both = dev.sweep(codec, tols, 0, N // 2)                         # two calls on the two halves add up to the one call
    both = dev.sweep(codec, tols, N // 2, N - N // 2, hist=both).cpu().numpy()
    assert np.array_equal(both, hist)
    full = torch.full((64, VEC3_RATE_CLASSES), SENTINEL, dtype=torch.int64, device="cuda")   # the call adds, and only to its own rows
    full = dev.sweep(codec, tols, hist=full).cpu().numpy()
    assert np.array_equal(full[:len(tols)], hist + SENTINEL) and (full[len(tols):] == SENTINEL).all()
    med = tols[3]
    many = [float(v) for v in np.geomspace(med / 64, med * 8, 57).astype(F)] + tols
    assert len(many) == 64
    got = dev.sweep(codec, many).cpu().numpy()
    assert np.array_equal(got, t3t.sweep(leaves, rec, err, many))
    assert len({r.tobytes() for r in got}) > 20                      # the rungs do differ
    lib, h = codec._lib, codec._h
    t1 = np.array([0.5], F)
    assert lib.vqhip_vec3_rate_sweep_device(h, None, None, None, 0, t1.ctypes.data, 1, None, None) == 0
    for bad in (0, 65, -1):
        assert lib.vqhip_vec3_rate_sweep_device(h, dev.x.data_ptr(), dev.r.data_ptr(), dev.e.data_ptr(), N, t1.ctypes.data, bad, both.ctypes.data, None) == -1
        assert "n_tols" in lib.vqhip_vec3_last_error(h).decode()
        assert lib.vqhip_vec3_rate_sweep_device(h, None, None, None, 0, t1.ctypes.data, bad, None, None) == -1   # the count is checked before n == 0
    assert lib.vqhip_vec3_rate_sweep_device(h, dev.x.data_ptr(), None, dev.e.data_ptr(), N, t1.ctypes.data, 1, None, None) == -1
    assert "null pointer" in lib.vqhip_vec3_last_error(h).decode()
    assert np.array_equal(dev.sweep(codec, tols).cpu().numpy(), hist)   # the handle still works


def every_column_ladder():
    """64 rungs: TOL_S first, then TOL_S * 2^k for 61 other k, 0 and +inf"""
    tols = [TOL_S] + [float(F(TOL_S) * F(2.0) ** k) for k in range(-31, 32) if k != 0][:61] + [0.0, float("inf")]
    assert len(tols) == 64
    return tols


def test_sweep_device_with_every_column_and_the_stride_loop(codec):
    x, recon, err = t3t.every_column_leaves(TOL_S)
    tols = every_column_ladder()
    got = Resident(x, recon, err).sweep(codec, tols).cpu().numpy()
    assert np.array_equal(got, t3t.sweep(x, recon, err, tols))
    assert (got[0] >= 1).all() and got[0, :49].tolist() == [1] * 49 and got[0, 49] == 2 and got[0, 50] == 1
    # more than two steps of the capped grid (1024 workgroups of 4 leaves), kept leaves in between (a run of 400 across the first
    # step's end), every column at changing places.  2 * 4096 + 1500 = 9692 leaves are a multiple of 4, so the same batch
    # without its last leaf follows: its last workgroup holds three leaves.
    n = 2 * 4096 + 1500
    rng = np.random.default_rng(4)
    pick = rng.integers(0, len(x), n)
    bx, br, be = x[pick], recon[pick], err[pick].copy()
    keep = rng.random(n) < 0.4
    keep[3900:4300] = True
    keep[8186:8196] = False
    forced = keep & np.isfinite(be[:, 0])
    be[forced] = 0.25
    assert 0.35 < forced.mean() < 0.45
    dev = Resident(bx, br, be)
    # the restatement once per distinct (leaf, error) pair instead of once per pick: a code depends on the leaf and its error alone
    ux, ur, ue = np.concatenate([x, x]), np.concatenate([recon, recon]), np.concatenate([err, np.full_like(err, 0.25)])
    which = pick + len(x) * forced
    cols = np.stack([t3t.columns(t3r.classify(ux, ur, ue, tol)[0]) for tol in tols])   # [T, 104]
    code = dev_encode(codec, bx, br, be, TOL_S)[0]                   # what the encoder says on the whole batch at rung 0
    for m in (n, n - 1):
        assert (m % 4 != 0) == (m == n - 1) and m > 2 * 4096
        got = dev.sweep(codec, tols, 0, m).cpu().numpy()
        weight = np.bincount(which[:m], minlength=len(ux))
        want = np.zeros_like(got)
        for t in range(len(tols)):
            np.add.at(want[t], cols[t], weight)
        assert np.array_equal(got, want), m
        assert (got.sum(axis=1) == m).all() and (got[0] > 0).all() and got[0, 50] > 3000, got[0]
        assert np.array_equal(got[0], counts(code[:m])), m


def test_sweep_device_on_unsorted_ladders_without_zero_and_with_a_nan_rung(codec):
    """The shortcut "kept at every rung" beside finite rungs only, then switched off by a NaN rung.  Ladder A: unsorted, the
    smallest rung (0.3) neither first nor last, no 0.0 and no NaN, so the leaves whose error is 0.25 take the shortcut and are
    counted by lanes 0 .. 4; ladder B: A with a NaN rung in the middle."""
    x, recon, err = t3t.every_column_leaves(TOL_S)
    n = len(x)
    forced = (np.arange(n) % 3 == 1) & np.isfinite(err[:, 0])
    err[forced] = 0.25
    assert n == 52 and forced.sum() >= 17 and np.isnan(err[:, 0]).any()
    a = [TOL_S, float(F(0.75) * F(TOL_S)), float(F(4) * F(TOL_S)), float(F(0.3)), float("inf")]
    b = a[:2] + [float("nan")] + a[2:]
    assert min(a) == a[3] > 0.25
    want_a, want_b = t3t.sweep(x, recon, err, a), t3t.sweep(x, recon, err, b)
    assert (want_a[:, 50] >= forced.sum()).all() and want_a[3, 50] == forced.sum() < want_a[2, 50] < n   # the case tests something
    dev = Resident(x, recon, err)
    got_a, got_b = dev.sweep(codec, a).cpu().numpy(), dev.sweep(codec, b).cpu().numpy()
    assert np.array_equal(got_a, want_a), got_a
    assert np.array_equal(got_b, want_b), got_b
    assert (got_a.sum(axis=1) == n).all() and (got_b.sum(axis=1) == n).all()
    assert got_b[2, 49] == n                                         # the NaN rung: every leaf raw
    assert np.array_equal(np.delete(got_b, 2, axis=0), got_a)        # ... and every other rung as without it


def test_rate_sweep_on_host_leaves_at_two_chunk_sizes(codec, pack, leaves):
    _, err, rec = dev_roundtrip(codec, leaves)
    tols = ladder(err)
    want = t3t.sweep(leaves, rec, err, tols)
    before = codec.compress_residual(leaves, tols[3], return_leaf_err=True)
    hist = codec.rate_sweep(leaves, tols)
    assert hist.dtype == np.int64 and hist.shape == (7, 51) and np.array_equal(hist, want)
    assert np.array_equal(codec.rate_sweep(leaves[:33], tols), t3t.sweep(leaves[:33], rec[:33], err[:33], tols))
    assert not codec.rate_sweep(leaves[:0], tols).any()
    after = codec.compress_residual(leaves, tols[3], return_leaf_err=True)
    assert all(same(a, b) for a, b in zip(before, after))           # indices, codes, payload and errors: unchanged by having swept
    assert np.array_equal(counts(after[1]), hist[3]) and len(after[2]) == vec3_rate_payload_bytes(hist[3])
    small = HipVec3Codec(pack, precision=codec.precision)            # chunks of 32, 32, 32, 32, 8 add up to the same histogram
    try:
        small.set_chunk_leaves(32)
        assert np.array_equal(small.rate_sweep(leaves, tols), want)
    finally:
        small.close()


def test_rate_compress_fits_the_budget_and_equals_the_compress_at_its_tolerance(codec, pack, leaves):
    _, err, rec = dev_roundtrip(codec, leaves)
    tols = ladder(err)
    tf = np.array(tols, F)
    hist0 = codec.rate_sweep(leaves, tols)
    sizes = [vec3_rate_payload_bytes(r) for r in hist0]
    assert sizes == [t3t.payload_bytes(r) for r in hist0]
    budget = sizes[3]                                                # what the median rung needs
    tol_used, hist, idx, code, payload, lerr = codec.rate_compress(leaves, tols, budget, return_leaf_err=True)
    t = t3t.pick(hist0, tf, budget)
    assert np.array_equal(hist, hist0) and t == vec3_rate_pick(hist0, tols, budget)
    assert tol_used == HipVec3Codec.check_tol(tols[t]) and tol_used <= HipVec3Codec.check_tol(tols[3])
    assert all(s > budget for s, v in zip(sizes, tols) if v < tol_used)   # no smaller rung fits
    ref = codec.compress_residual(leaves, tol_used, return_leaf_err=True)
    assert same(idx, ref[0]) and same(code, ref[1]) and same(payload, ref[2]) and same(lerr, ref[3])
    assert len(payload) <= budget and len(payload) == vec3_rate_payload_bytes(hist[t]) == sizes[t]
    print(f"{codec.precision}: budget {budget} B -> tol {tol_used:.6g}, payload {len(payload)} B, sizes {sizes}")
    out = codec.decompress_residual(idx, tol_used, code, payload)
    assert np.isfinite(leaves).all() and np.abs(leaves - out).max() <= F(tol_used)
    assert len(codec.rate_compress(leaves, tols, budget)) == 5
    small = HipVec3Codec(pack, precision=codec.precision)            # chunks of 32, 32, 32, 32, 8: the same bytes
    try:
        small.set_chunk_leaves(32)
        got = small.rate_compress(leaves, tols, budget, return_leaf_err=True)
        assert got[0] == tol_used and np.array_equal(got[1], hist)
        assert same(got[2], idx) and same(got[3], code) and same(got[4], payload) and same(got[5], lerr)
    finally:
        small.close()
    # one byte under the smallest size a rung that is not NaN reaches: refused with both numbers before pass 2; leaf_code, payload
    # and tol_used stay as they were, indices and leaf_err hold pass 1's values
    finite = [s for s, v in zip(sizes, tols) if not np.isnan(v)]
    many = [float(v) for v in np.geomspace(tols[3] / 8, tols[3], 5).astype(F)] + [float("nan")]
    sizes_many = [vec3_rate_payload_bytes(r) for r in codec.rate_sweep(leaves, many)]
    least = min(sizes_many[:5])
    assert min(finite) == 0 and least > 0 and sizes_many[5] == N * 6144
    with pytest.raises(RuntimeError) as refusal:
        codec.rate_compress(leaves, many, least - 1)
    assert str(least) in str(refusal.value) and str(least - 1) in str(refusal.value)
    lib, h = codec._lib, codec._h
    p = lambda a: a.ctypes.data   # noqa: E731
    tm = np.array(many, F)
    used, nb = ctypes.c_float(-3.0), ctypes.c_int64(-5)
    h5 = np.full((6, 51), SENTINEL, np.int64)
    i5, e5 = np.full((N, 64), 0x7777, np.uint16), np.full((N, 2), -9.0, F)
    c5, p5 = np.full(N, 0x7777, np.uint16), np.full(N * 6144, FILL, np.uint8)
    args = lambda budget: (h, p(leaves), N, p(tm), 6, budget, ctypes.byref(used), p(h5), p(i5), p(e5), p(c5), p(p5), ctypes.byref(nb))   # noqa: E731
    assert lib.vqhip_vec3_rate_compress(*args(least - 1)) == -1
    msg = lib.vqhip_vec3_last_error(h).decode()
    assert str(least) in msg and str(least - 1) in msg
    assert used.value == -3.0 and nb.value == 0 and (c5 == 0x7777).all() and (p5 == FILL).all()
    assert same(i5, idx) and same(e5, lerr) and [vec3_rate_payload_bytes(r) for r in h5] == sizes_many
    assert lib.vqhip_vec3_rate_compress(*args(-1)) == -1 and "payload_budget < 0" in lib.vqhip_vec3_last_error(h).decode()
    assert lib.vqhip_vec3_rate_compress(h, p(leaves), N, p(tm), 6, least, None, None, p(i5), None, p(c5), p(p5), ctypes.byref(nb)) == -1
    assert lib.vqhip_vec3_rate_compress(h, p(leaves), N, p(tm), 65, least, ctypes.byref(used), None, p(i5), None, p(c5), p(p5), ctypes.byref(nb)) == -1
    assert "n_tols" in lib.vqhip_vec3_last_error(h).decode()
    assert lib.vqhip_vec3_rate_compress(h, None, 0, p(tm), 6, 0, ctypes.byref(used), p(h5), None, None, None, None, ctypes.byref(nb)) == 0
    assert nb.value == 0 and not h5.any() and (c5 == 0x7777).all()
    # hist and leaf_err may be NULL: the same bytes at the budget that just fits
    assert lib.vqhip_vec3_rate_compress(h, p(leaves), N, p(tm), 6, least, ctypes.byref(used), None, p(i5), None, p(c5), p(p5), ctypes.byref(nb)) == 0
    t5 = sizes_many.index(least)
    ref5 = codec.compress_residual(leaves, float(tm[t5]))
    assert used.value == tm[t5] and nb.value == least and same(i5, ref5[0]) and same(c5, ref5[1]) and same(p5[:least], ref5[2]) and (p5[least:] == FILL).all()
    again = codec.rate_compress(leaves, tols, budget, return_leaf_err=True)   # the handle still works
    assert again[0] == tol_used and all(same(a, b) for a, b in zip(again[1:], (hist, idx, code, payload, lerr)))


def test_the_new_calls_move_nothing_of_their_neighbours(codec, leaves):
    x = np.ascontiguousarray(leaves[:100])

    def neighbours():
        idx = codec.encode(x)
        ridx, rerr, rrec = codec.roundtrip(x, return_recon=True)
        return [idx, codec.decode(idx), ridx, rerr, rrec, *codec.compress_residual(x, 0.1, return_leaf_err=True)]

    before = neighbours()
    tols = ladder(before[3])
    hist = codec.rate_sweep(leaves, tols)
    codec.rate_compress(leaves, tols, vec3_rate_payload_bytes(hist[3]))
    _, derr, drec = dev_roundtrip(codec, leaves)
    Resident(leaves, drec, derr).sweep(codec, tols, stream=torch.cuda.Stream())
    after = neighbours()
    assert len(before) == len(after) == 9
    for k, (a, b) in enumerate(zip(before, after)):
        assert same(a, b), k
