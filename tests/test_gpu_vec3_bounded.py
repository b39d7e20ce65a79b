"""Error-bounded round trip of the Vec3 handle on the GPU: bit equality with encode_device / decode_device,
the leaf errors against tests/torch_ref_vec3_bounded.py (to the bit) and float64, invariance under batch, place, chunk and
stream, the selection, non-finite leaves, the host entry point, the tolerance guarantee, and the untouched neighbours."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3_bounded as tbd  # noqa: E402
from vqvdb_amd import synth_vec3, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("fp32", "bf16")


@pytest.fixture(scope="module")
def W():
    return synth_vec3.make_weights(0)


@pytest.fixture(scope="module")
def leaves():
    """The 520 leaves of tests/golden/golden_vec3_v1.npz (generated: 512 random, 8 edge cases)."""
    return np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])


@pytest.fixture()
def codec(W):
    c = HipVec3Codec(weightpack.dumps(W))
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def dev_roundtrip(codec, x, recon=True, indices=True, stream=None):
    """vqhip_vec3_roundtrip_device on host array x -> (idx uint16 | None, err, recon | None) as numpy."""
    n = len(x)
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = torch.zeros((n, 64), dtype=torch.int16, device="cuda") if indices else None
    dr = torch.zeros((n, 512, 3), dtype=torch.float32, device="cuda") if recon else None
    de = torch.full((n, 2), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.roundtrip_device(dx.data_ptr(), n, de.data_ptr(), di.data_ptr() if indices else 0, dr.data_ptr() if recon else 0,
                           stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return (di.cpu().numpy().view(np.uint16) if indices else None, de.cpu().numpy(), dr.cpu().numpy() if recon else None)


def dev_encode_decode(codec, x):
    n = len(x)
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = torch.zeros((n, 64), dtype=torch.int16, device="cuda")
    do = torch.zeros((n, 512, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.encode_device(dx.data_ptr(), n, di.data_ptr())
    codec.decode_device(di.data_ptr(), n, do.data_ptr())
    torch.cuda.synchronize()
    return di.cpu().numpy().view(np.uint16), do.cpu().numpy()


def dev_select(codec, err, tol, stream=None):
    n = len(err)
    de = torch.from_numpy(np.ascontiguousarray(err, dtype=np.float32)).cuda()
    ids = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    codec.select_outliers_device(de.data_ptr(), n, tol, ids.data_ptr(), cnt.data_ptr(), stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    c = int(cnt.item())
    assert 0 <= c <= n
    ids = ids.cpu().numpy()
    assert (ids[c:] == -7).all(), "ids written past the count"
    return ids[:c]


@pytest.mark.parametrize("mode", MODES)
def test_roundtrip_equals_encode_then_decode_bit_for_bit(codec, leaves, mode):
    codec.precision = mode
    for n in (1, 3, 129, 520):
        x = leaves[:n]
        idx, rec = dev_encode_decode(codec, x)
        for stream in (None, torch.cuda.Stream()):
            ridx, _, rrec = dev_roundtrip(codec, x, stream=stream)
            assert np.array_equal(ridx, idx), (mode, n)
            assert same(rrec, rec), (mode, n)
    # the torch-tensor form of the wrapper is the same call
    dx = torch.from_numpy(leaves).cuda()
    ti, te, trc = codec.roundtrip(dx, return_recon=True)
    torch.cuda.synchronize()
    assert np.array_equal(ti.cpu().numpy().view(np.uint16), idx) and same(trc.cpu().numpy(), rec)
    assert same(te.cpu().numpy(), dev_roundtrip(codec, leaves)[1])


@pytest.mark.parametrize("mode", MODES)
def test_leaf_errors_equal_the_restatement_and_do_not_depend_on_the_store(codec, leaves, mode):
    """max |x - x^|: equal to numpy's on the returned reconstruction (a maximum of float32 differences is exact).
    sum (x - x^)^2: equal to the fixed-order restatement bit for bit, and to float64 within 1e-5 relative (the order has at
    most 15 chained additions of non-negative terms: 18 * 2^-24 = 1.1e-6 with the two roundings of a term)."""
    codec.precision = mode
    _, err, rec = dev_roundtrip(codec, leaves)
    assert same(err[:, 0], np.abs(leaves - rec).reshape(520, -1).max(axis=1))
    ref = tbd.leaf_err_fixed(leaves, rec)
    assert same(err[:, 0], ref[:, 0])
    assert same(err[:, 1], ref[:, 1])
    f64 = tbd.leaf_err_f64(leaves, rec)
    rel = np.abs(err[:, 1].astype(np.float64) - f64[:, 1]) / f64[:, 1]
    print(f"{mode}: sum of squares against float64, largest relative difference {rel.max():.2e}; largest leaf error {err[:, 0].max():.4f}")
    assert rel.max() <= 1e-5
    for recon, indices in ((False, True), (False, False), (True, False)):
        assert same(dev_roundtrip(codec, leaves, recon=recon, indices=indices)[1], err), (recon, indices)


@pytest.mark.parametrize("mode", MODES)
def test_leaf_error_bits_do_not_depend_on_batch_place_or_chunk(codec, W, leaves, mode):
    codec.precision = mode
    _, err, _ = dev_roundtrip(codec, leaves, recon=False)
    assert same(dev_roundtrip(codec, leaves, recon=False)[1], err)
    for i in (0, 77, 519):
        assert same(dev_roundtrip(codec, leaves[i:i + 1], recon=False)[1], err[i:i + 1]), i
    moved = np.concatenate([leaves[100:], leaves[:100]])
    assert same(dev_roundtrip(codec, moved, recon=False)[1], np.concatenate([err[100:], err[:100]]))
    many = synth_vec3.make_leaves(2500, 99)
    midx, merr, mrec = dev_roundtrip(codec, many)
    small = HipVec3Codec(weightpack.dumps(W), precision=mode)
    try:
        small.set_chunk_leaves(1024)
        sidx, serr, srec = dev_roundtrip(small, many, stream=torch.cuda.Stream())
        assert small.chunk_leaves() == 1024
        assert np.array_equal(sidx, midx) and same(serr, merr) and same(srec, mrec)
        assert same(dev_roundtrip(small, many, recon=False, indices=False)[1], merr)
        assert same(dev_roundtrip(small, leaves, recon=False)[1], err)
    finally:
        small.close()


def test_selection_equals_the_rule_exactly(codec, leaves):
    _, err, _ = dev_roundtrip(codec, leaves, recon=False)
    e = err[:, 0]
    tols = [float(np.percentile(e, p, method="lower")) for p in (0, 50, 90, 100)] + [float(e[123]), 0.0, float("inf"), float("nan")]
    for tol in tols:
        for stream in (None, torch.cuda.Stream()):
            ids = dev_select(codec, err, tol, stream)
            with np.errstate(invalid="ignore"):
                want = np.flatnonzero(~(e <= np.float32(tol)))
            assert np.array_equal(ids, want), tol
            assert np.array_equal(ids, tbd.select_outliers(err, tol))
    assert 123 not in dev_select(codec, err, float(e[123]))
    assert len(dev_select(codec, err, float(e.max()))) == 0                       # none is an outlier
    assert np.array_equal(dev_select(codec, err, -1.0), np.arange(520))           # every leaf is one
    assert len(dev_select(codec, err, float(np.percentile(e, 50, method="lower")))) == 520 - 260
    assert len(dev_select(codec, np.zeros((0, 2), np.float32), 0.5)) == 0


def test_selection_over_several_scan_blocks(codec):
    """Synthetic errors, no model run: 70 001 and 1 300 003 entries (69 and 1270 blocks of 1024: the scan's second step)."""
    rng = np.random.default_rng(11)
    for n in (70001, 1300003):
        err = rng.random((n, 2), dtype=np.float32)
        err[rng.integers(0, n, 50), 0] = np.nan
        err[rng.integers(0, n, 50), 0] = np.inf
        err[1024 * 3:1024 * 5, 0] = 0.0      # two blocks without an outlier
        err[1024 * 7:1024 * 9, 0] = 2.0      # two blocks of outliers only
        for tol in (0.5, 0.999, 0.0, float(err[4242, 0]), float("inf"), float("nan")):
            ids = dev_select(codec, err, tol)
            assert np.array_equal(ids, tbd.select_outliers(err, tol)), (n, tol)
        assert np.array_equal(dev_select(codec, err, -1.0), np.arange(n))


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_leaves_are_always_selected_and_touch_no_other_leaf(codec, leaves, mode):
    codec.precision = mode
    x = np.ascontiguousarray(leaves[:64])
    idx, err, rec = dev_roundtrip(codec, x)
    bad = x.copy()
    bad[5, 300, 1] = np.nan
    bad[41, 17, 2] = np.inf
    bidx, berr, brec = dev_roundtrip(codec, bad)
    ok = np.setdiff1d(np.arange(64), [5, 41])
    assert np.array_equal(bidx[ok], idx[ok]) and same(berr[ok], err[ok]) and same(brec[ok], rec[ok])
    assert np.isnan(berr[[5, 41], 0]).all()
    for tol in (0.0, float(err[:, 0].max()), 1e30, float("inf")):
        ids = dev_select(codec, berr, tol)
        assert 5 in ids and 41 in ids, tol
    assert np.array_equal(dev_select(codec, berr, float("inf")), [5, 41])
    hidx, hids, hraw, herr = codec.compress_bounded(bad, float("inf"), return_leaf_err=True)
    assert np.array_equal(hids, [5, 41]) and same(herr, berr) and np.array_equal(hidx, bidx)
    out = codec.decompress_bounded(hidx, hids, hraw)
    assert same(out[[5, 41]], bad[[5, 41]]) and same(out[ok], rec[ok])


@pytest.mark.parametrize("mode", MODES)
def test_host_entry_point_equals_the_device_calls(codec, W, leaves, mode):
    codec.precision = mode
    idx, err, rec = dev_roundtrip(codec, leaves)
    tol = float(np.percentile(err[:, 0], 50, method="lower"))
    ids = dev_select(codec, err, tol)
    hidx, hids, hraw, herr = codec.compress_bounded(leaves, tol, return_leaf_err=True)
    assert np.array_equal(hidx, idx) and same(herr, err) and np.array_equal(hids, ids) and same(hraw, leaves[ids])
    ridx, rerr, rrec = codec.roundtrip(leaves, return_recon=True)      # numpy in, numpy out: the host entry points
    assert np.array_equal(ridx, idx) and same(rerr, err) and same(rrec, rec)
    small = HipVec3Codec(weightpack.dumps(W), precision=mode)          # several chunks: ids carry the chunk offset
    try:
        small.set_chunk_leaves(100)
        sidx, sids, _, serr = small.compress_bounded(leaves, tol, return_leaf_err=True)
        assert np.array_equal(sidx, idx) and same(serr, err) and np.array_equal(sids, ids)
    finally:
        small.close()


def test_host_entry_point_argument_errors(codec, leaves):
    lib, h = codec._lib, codec._h
    x = np.ascontiguousarray(leaves[:4])
    idx, ids, err = np.zeros((4, 64), np.uint16), np.full(4, -1, np.int64), np.zeros((4, 2), np.float32)
    cnt = ctypes.c_int64(-5)
    p = lambda a: a.ctypes.data   # noqa: E731
    msg = lambda: lib.vqhip_vec3_last_error(h).decode()   # noqa: E731
    assert lib.vqhip_vec3_compress_bounded(h, p(x), -1, 0.5, p(idx), p(err), p(ids), ctypes.byref(cnt)) == -1 and "n_leaves < 0" in msg()
    assert lib.vqhip_vec3_compress_bounded(h, None, 4, 0.5, p(idx), p(err), p(ids), ctypes.byref(cnt)) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_compress_bounded(h, p(x), 4, 0.5, None, p(err), p(ids), ctypes.byref(cnt)) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_compress_bounded(h, p(x), 4, 0.5, p(idx), p(err), None, ctypes.byref(cnt)) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_compress_bounded(h, p(x), 4, 0.5, p(idx), p(err), p(ids), None) == -1 and "n_outliers is NULL" in msg()
    assert lib.vqhip_vec3_compress_bounded(h, None, 0, 0.5, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
    cnt = ctypes.c_int64(-5)
    assert lib.vqhip_vec3_compress_bounded(h, p(x), 4, -1.0, p(idx), None, p(ids), ctypes.byref(cnt)) == 0      # leaf_err may be NULL
    assert cnt.value == 4 and ids.tolist() == [0, 1, 2, 3]
    # the device calls
    assert lib.vqhip_vec3_roundtrip_device(h, None, -1, None, None, None, None) == -1 and "n_leaves < 0" in msg()
    assert lib.vqhip_vec3_roundtrip_device(h, None, 0, None, None, None, None) == 0
    assert lib.vqhip_vec3_roundtrip_device(h, None, 4, None, None, None, None) == -1 and "null pointer" in msg()
    de = torch.zeros((4, 2), device="cuda")
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    assert lib.vqhip_vec3_roundtrip_device(h, dx.data_ptr(), 4, None, None, None, None) == -1 and "leaf_err_dev" in msg()
    assert lib.vqhip_vec3_select_outliers_device(h, de.data_ptr(), -1, 0.5, None, None, None) == -1 and "n_leaves < 0" in msg()
    assert lib.vqhip_vec3_select_outliers_device(h, de.data_ptr(), 4, 0.5, None, None, None) == -1 and "count_dev is NULL" in msg()
    dc = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.vqhip_vec3_select_outliers_device(h, de.data_ptr(), 4, 0.5, None, dc.data_ptr(), None) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_select_outliers_device(h, None, 0, 0.5, None, dc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(dc.item()) == 0
    assert np.array_equal(codec.encode(x), dev_roundtrip(codec, x)[0])      # the handle still works


@pytest.mark.parametrize("mode", MODES)
def test_the_pair_keeps_every_leaf_within_the_tolerance(codec, leaves, mode):
    codec.precision = mode
    _, err = codec.roundtrip(leaves)
    tol = float(np.median(err[:, 0]))
    idx, ids, raw = codec.compress_bounded(leaves, tol)
    assert 0 < len(ids) < 520
    out = codec.decompress_bounded(idx, ids, raw)
    worst = np.abs(leaves - out).reshape(520, -1).max(axis=1)
    print(f"{mode}: tol {tol:.4f}, {len(ids)} of 520 leaves kept raw, largest remaining error {worst.max():.4f}")
    assert (worst <= tol).all()
    assert same(out[ids], leaves[ids])
    # tol = 0: every leaf whose reconstruction is not exact is stored raw, the pair is lossless
    idx0, ids0, raw0 = codec.compress_bounded(leaves, 0.0)
    rec = codec.decode(idx0)
    inexact = np.flatnonzero((leaves != rec).reshape(520, -1).any(axis=1))
    assert np.array_equal(ids0, inexact)
    assert np.array_equal(codec.decompress_bounded(idx0, ids0, raw0), leaves)


@pytest.mark.parametrize("mode", MODES)
def test_a_roundtrip_moves_nothing_of_its_neighbours(W, leaves, mode):
    """encode / decode / train_eval_device on a handle before and after a round trip (with and without a stored
    reconstruction, with and without caller's indices: the internal index slot lives in the second half of R8, where
    train_eval_device puts its reconstruction)."""
    c = HipVec3Codec(weightpack.dumps(W), precision=mode)
    try:
        c.train_begin()
        x = np.ascontiguousarray(leaves[:200])
        dx = torch.from_numpy(x).cuda()
        stats = torch.zeros(c.train_stats_floats(), dtype=torch.float32, device="cuda")
        sums = torch.zeros(3, dtype=torch.float32, device="cuda")

        def neighbours():
            idx = c.encode(x)
            rec = c.decode(idx)
            out = []
            for keep in (False, True):
                r = torch.zeros((200, 512, 3), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                c.train_eval_device(dx.data_ptr(), 200, stats.data_ptr(), sums.data_ptr(), r.data_ptr() if keep else 0)
                torch.cuda.synchronize()
                out += [stats.cpu().numpy().copy(), sums.cpu().numpy().copy(), r.cpu().numpy()]
            return [idx, rec] + out

        before = neighbours()
        for recon, indices in ((True, True), (False, False), (False, True), (True, False)):
            dev_roundtrip(c, leaves, recon=recon, indices=indices)
            c.compress_bounded(leaves[:300], 0.1)
            after = neighbours()
            for a, b in zip(before, after):
                assert same(a, b), (recon, indices)
    finally:
        c.close()
