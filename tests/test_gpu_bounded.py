"""Error-bounded compression of the scalar handle on the GPU: bit equality with encode_device / decode_device,
the leaf errors against tests/torch_ref_bounded.py (to the bit), invariance under batch, place, chunk and store, the selection,
non-finite leaves, the tolerance guarantee, the .vqvdb + .vqres file pair and the argument errors.  Every case runs with the
automatic small-batch kernels and with set_small_batch_tiles(0) (the kernels of full chunks)."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_bounded as tbd  # noqa: E402
from vqvdb_amd import synth, vqvdbfile, weightpack  # noqa: E402
from vqvdb_amd.codec import GRID_BEGIN_FN, LEAF_ALLOC_FN, HipCodec  # noqa: E402

pytestmark = pytest.mark.gpu

N = 136
SIZES = (1, 3, 33, 136)


@pytest.fixture(scope="module")
def pack():
    return weightpack.dumps(synth.make_weights(0))


@pytest.fixture(scope="module")
def leaves():
    return np.ascontiguousarray(np.concatenate([synth.make_leaves(64), synth.edge_leaves(), synth.sparse_leaves(64)]))


@pytest.fixture(params=(-1, 0), ids=("small_batch_auto", "full_chunk_kernels"))
def codec(request, pack):
    c = HipCodec(pack)
    c.set_small_batch_tiles(request.param)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def dev_roundtrip(codec, x, recon=True, indices=True, stream=None):
    """vqhip_roundtrip_device on host array x -> (idx | None, err, recon | None) as numpy."""
    n = len(x)
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = torch.zeros((n, 64), dtype=torch.uint8, device="cuda") if indices else None
    dr = torch.zeros((n, 512), dtype=torch.float32, device="cuda") if recon else None
    de = torch.full((n, 2), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.roundtrip_device(dx.data_ptr(), n, de.data_ptr(), di.data_ptr() if indices else 0, dr.data_ptr() if recon else 0,
                           stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return (di.cpu().numpy() if indices else None, de.cpu().numpy(), dr.cpu().numpy() if recon else None)


def dev_encode_decode(codec, x):
    n = len(x)
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    do = torch.zeros((n, 512), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.encode_device(dx.data_ptr(), n, di.data_ptr())
    codec.decode_device(di.data_ptr(), n, do.data_ptr())
    torch.cuda.synchronize()
    return di.cpu().numpy(), do.cpu().numpy()


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


def rule(e, tol):
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~(e <= np.float32(tol)))


def test_roundtrip_equals_encode_then_decode_bit_for_bit(codec, leaves):
    for n in SIZES:
        x = leaves[:n]
        idx, rec = dev_encode_decode(codec, x)
        _, err, _ = dev_roundtrip(codec, x)
        for stream in (None, torch.cuda.Stream()):
            for recon, indices in ((True, True), (False, True), (True, False), (False, False)):
                ridx, rerr, rrec = dev_roundtrip(codec, x, recon=recon, indices=indices, stream=stream)
                assert ridx is None or np.array_equal(ridx, idx), (n, recon, indices)
                assert rrec is None or same(rrec, rec), (n, recon, indices)
                assert same(rerr, err), (n, recon, indices)
    # the torch-tensor and the numpy form of the wrapper are the same call
    ti, te, trc = codec.roundtrip(torch.from_numpy(leaves).cuda(), return_recon=True)
    torch.cuda.synchronize()
    assert np.array_equal(ti.cpu().numpy(), idx) and same(trc.cpu().numpy(), rec) and same(te.cpu().numpy(), err)
    hi, he, hr = codec.roundtrip(leaves, return_recon=True)
    assert np.array_equal(hi, idx) and same(hr, rec) and same(he, err)


def test_leaf_errors_equal_the_restatement_bit_for_bit(codec, leaves):
    """max |x - x^|: numpy's float32 maximum on the returned reconstruction (a maximum of float32 differences is exact).
    sum (x - x^)^2: the fixed-order restatement bit for bit; against float64 within 1e-5 relative (13 chained additions of
    non-negative terms, two roundings per term: below 1e-6)."""
    for n in SIZES:
        x = leaves[:n]
        _, err, rec = dev_roundtrip(codec, x)
        assert same(err[:, 0], np.abs(x - rec).max(axis=1)), n
        assert same(err, tbd.leaf_err_fixed(x, rec)), n
    f64 = tbd.leaf_err_f64(leaves, rec)
    rel = np.abs(err[:, 1].astype(np.float64) - f64[:, 1]) / f64[:, 1]
    print(f"sum of squares against float64, largest relative difference {rel.max():.2e}; leaf errors {err[:, 0].min():.4g} .. {err[:, 0].max():.4g}")
    assert rel.max() <= 1e-5


def test_leaf_error_bits_do_not_depend_on_batch_place_chunk_or_store(codec, pack, leaves):
    _, err, rec = dev_roundtrip(codec, leaves)
    for n in SIZES:
        assert same(dev_roundtrip(codec, leaves[:n], recon=False)[1], err[:n]), n
        assert same(dev_roundtrip(codec, leaves[N - n:], recon=False, indices=False)[1], err[N - n:]), n
    ridx, rerr, rrec = dev_roundtrip(codec, leaves[::-1])
    assert same(rerr, err[::-1]) and same(rrec, rec[::-1])
    small = HipCodec(pack)
    try:
        small.set_chunk_leaves(32)          # 136 leaves: chunks of 32, 32, 32, 32, 8
        for tiles in (-1, 0):
            small.set_small_batch_tiles(tiles)
            sidx, serr, srec = dev_roundtrip(small, leaves, stream=torch.cuda.Stream())
            assert small.chunk_leaves() == 32
            assert same(serr, err) and same(srec, rec), tiles
            assert same(dev_roundtrip(small, leaves, recon=False, indices=False)[1], err), tiles
        hidx, hids, hraw, herr = small.compress_bounded(leaves, float(np.median(err[:, 0])), return_leaf_err=True)   # ids carry the chunk offset
        assert same(herr, err) and np.array_equal(hids, rule(err[:, 0], float(np.median(err[:, 0]))))
    finally:
        small.close()


def test_selection_equals_the_rule_at_five_tolerances(codec, leaves):
    _, err, _ = dev_roundtrip(codec, leaves, recon=False)
    e = err[:, 0]
    below = float(np.nextafter(e.min(), np.float32(-np.inf)))
    above = float(np.nextafter(e.max(), np.float32(np.inf)))
    for tol in (below, float(e[77]), float(np.median(e)), above, float("nan")):
        for stream in (None, torch.cuda.Stream()):
            ids = dev_select(codec, err, tol, stream)
            assert np.array_equal(ids, rule(e, tol)), tol
            assert np.array_equal(ids, tbd.select_outliers(err, tol))
    assert np.array_equal(dev_select(codec, err, below), np.arange(N))
    assert 77 not in dev_select(codec, err, float(e[77]))            # equality is not an outlier
    assert len(dev_select(codec, err, above)) == 0
    assert np.array_equal(dev_select(codec, err, float("nan")), np.arange(N))
    assert 0 < len(dev_select(codec, err, float(np.median(e)))) < N
    assert len(dev_select(codec, np.zeros((0, 2), np.float32), 0.5)) == 0


def test_selection_over_more_than_two_blocks(codec):
    """3000 synthetic error values, no model run: three selection blocks of 1024, a scattered pattern, one block without an
    outlier and a stretch of outliers only across a block boundary."""
    rng = np.random.default_rng(11)
    err = rng.random((3000, 2), dtype=np.float32)
    err[rng.integers(0, 3000, 20), 0] = np.nan
    err[rng.integers(0, 3000, 20), 0] = np.inf
    err[1024:2048, 0] = 0.0
    err[2040:2060, 0] = 2.0
    for tol in (0.5, 0.999, 0.0, float(err[42, 0]), float("inf"), float("nan")):
        assert np.array_equal(dev_select(codec, err, tol), tbd.select_outliers(err, tol)), tol


def test_non_finite_leaves_are_always_selected_and_touch_no_other_leaf(codec, leaves):
    for n in SIZES[1:]:
        x = np.ascontiguousarray(leaves[:n])
        idx, err, rec = dev_roundtrip(codec, x)
        i_nan, i_inf = (0, 2) if n == 3 else (5, n - 2)
        bad = x.copy()
        bad[i_nan, 300] = np.nan
        bad[i_inf, 17] = np.inf
        bidx, berr, brec = dev_roundtrip(codec, bad)
        ok = np.setdiff1d(np.arange(n), [i_nan, i_inf])
        assert np.array_equal(bidx[ok], idx[ok]) and same(berr[ok], err[ok]) and same(brec[ok], rec[ok]), n
        assert np.isnan(berr[[i_nan, i_inf], 0]).all()
        for tol in (0.0, float(err[:, 0].max()), 1e30, float("inf")):
            ids = dev_select(codec, berr, tol)
            assert i_nan in ids and i_inf in ids, (n, tol)
        assert np.array_equal(dev_select(codec, berr, float("inf")), [i_nan, i_inf])
    bad.view(np.uint32)[i_nan, 300] = 0x7FC12345                     # a NaN payload comes back as it went in
    hidx, hids, hraw, herr = codec.compress_bounded(bad, float("inf"), return_leaf_err=True)
    assert np.array_equal(hids, [i_nan, i_inf]) and same(herr[ok], berr[ok]) and np.array_equal(hidx[ok], bidx[ok])
    out = codec.decompress_bounded(hidx, hids, hraw)
    assert same(out[[i_nan, i_inf]], bad[[i_nan, i_inf]]) and same(out[ok], rec[ok])


@pytest.fixture()
def bounded(codec, leaves):
    """tol = the median leaf error; what compress_bounded -> decompress_bounded returns for the 136 leaves."""
    _, err = codec.roundtrip(leaves)
    tol = float(np.median(err[:, 0]))
    idx, ids, raw = codec.compress_bounded(leaves, tol)
    return tol, err, idx, ids, raw, codec.decompress_bounded(idx, ids, raw)


def test_the_pair_keeps_every_leaf_within_the_tolerance(codec, leaves, bounded):
    tol, err, idx, ids, raw, out = bounded
    assert 0 < len(ids) < N
    assert np.array_equal(ids, rule(err[:, 0], tol))
    worst = np.abs(leaves - out).max(axis=1)
    print(f"tol {tol:.4f}, {len(ids)} of {N} leaves kept raw, largest remaining error {worst.max():.4f}")
    assert np.isfinite(leaves).all() and (worst <= tol).all()
    assert same(raw, leaves[ids]) and same(out[ids], leaves[ids])
    keep = np.setdiff1d(np.arange(N), ids)
    plain = codec.decode(codec.encode(leaves))
    assert np.array_equal(idx, codec.encode(leaves)) and same(out[keep], plain[keep])
    assert not same(out[ids], plain[ids])
    for n in SIZES[:3]:                                              # the same leaves at the other batch sizes
        i2, ids2, raw2 = codec.compress_bounded(leaves[:n], tol)
        assert np.array_equal(ids2, ids[ids < n]) and np.array_equal(i2, idx[:n])
        assert same(codec.decompress_bounded(i2, ids2, raw2), out[:n])


def grids_of(leaves):
    org = np.arange(N * 3, dtype=np.int32).reshape(N, 3) * 8
    tr = np.arange(16, dtype=np.float32)
    return [("density", org[:70], np.ascontiguousarray(leaves[:70]), tr), ("temperature", org[70:], np.ascontiguousarray(leaves[70:]), None)]


def test_file_pair_writes_the_same_vqvdb_and_the_selected_leaves_raw(codec, leaves, bounded, tmp_path):
    tol, err, idx, ids, raw, out = bounded
    grids = grids_of(leaves)
    plain, lossy, res = tmp_path / "plain.vqvdb", tmp_path / "bounded.vqvdb", tmp_path / "bounded.vqres"
    st0 = codec.compress_file(plain, grids, batch_leaves=32)
    st, bst = codec.compress_file_bounded(lossy, res, grids, tol, batch_leaves=32)
    assert lossy.read_bytes() == plain.read_bytes()
    assert st["leaves"] == st0["leaves"] == N and st["grids"] == 2
    rtol, rg = vqvdbfile.load_residual(res)
    assert rtol == HipCodec.check_tol(tol) and len(rg) == 2
    for (rids, rleaves), lo, hi in zip(rg, (0, 70), (70, N)):
        want = ids[(ids >= lo) & (ids < hi)]
        assert np.array_equal(rids, want - lo)
        assert same(rleaves, leaves[want])
    keep = np.setdiff1d(np.arange(N), ids)
    assert bst["leaves"] == N and bst["outliers"] == len(ids)
    assert bst["max_err_kept"] == err[keep, 0].max() and bst["max_err_kept"] <= tol
    assert abs(bst["sum_sq_kept"] - err[keep, 1].astype(np.float64).sum()) <= 1e-12 * bst["sum_sq_kept"]
    got, dst = codec.decompress_file_bounded(lossy, res, batch_leaves=32)
    assert [g[0] for g in got] == ["density", "temperature"] and dst["leaves"] == N
    assert same(np.concatenate([g[3] for g in got]), out)
    assert np.array_equal(np.concatenate([g[2] for g in got]), np.concatenate([g[1] for g in grids]))
    whole, _ = codec.decompress_file_bounded(lossy, res)              # one batch per grid
    assert same(np.concatenate([g[3] for g in whole]), out)
    lossy_only, _ = codec.decompress_file(lossy, batch_leaves=32)     # ignoring the sidecar: the plain decode
    assert same(np.concatenate([g[3] for g in lossy_only]), codec.decode(idx))
    # tol = NaN: every leaf raw, the pair is lossless; tol = +inf: an empty sidecar
    codec.compress_file_bounded(lossy, res, grids, float("nan"), batch_leaves=32)
    assert same(np.concatenate([g[3] for g in codec.decompress_file_bounded(lossy, res, batch_leaves=32)[0]]), leaves)
    _, binf = codec.compress_file_bounded(lossy, res, grids, float("inf"), batch_leaves=32)
    assert binf["outliers"] == 0 and res.read_bytes()[11:] == struct.pack("<II", 0, 0)
    assert binf["max_err_kept"] == err[:, 0].max()


def test_file_pair_refuses_a_sidecar_that_does_not_fit(codec, leaves, bounded, tmp_path):
    tol, err, idx, ids, raw, out = bounded
    grids = grids_of(leaves)
    lossy, res, bad = tmp_path / "b.vqvdb", tmp_path / "b.vqres", tmp_path / "bad.vqres"
    plain = codec.decode(idx)
    codec.compress_file_bounded(lossy, res, grids, tol, batch_leaves=32)
    rtol, rg = vqvdbfile.load_residual(res)
    assert len(rg[1][0]) >= 2

    def refused(grids_, match):
        vqvdbfile.save_residual(bad, rtol, grids_)
        with pytest.raises(RuntimeError, match=match):
            codec.decompress_file_bounded(lossy, bad, batch_leaves=32)

    refused(rg[:1], "holds 1 grids, the .vqvdb file 2")
    refused(rg + [rg[0]], "holds 3 grids, the .vqvdb file 2")
    past = rg[1][0].copy()
    past[-1] = 66                                                    # the second grid has 66 leaves: 0 .. 65
    refused([rg[0], (past, rg[1][1])], "record index 66 in grid 'temperature' of 66 leaves")
    buf = bytearray(res.read_bytes())                                # not ascending: the first grid's second index repeats its first
    assert len(rg[0][0]) >= 2
    buf[15 + 2052:15 + 2052 + 4] = buf[15:19]
    bad.write_bytes(bytes(buf))
    with pytest.raises(RuntimeError, match="is not ascending"):
        codec.decompress_file_bounded(lossy, bad, batch_leaves=32)
    bad.write_bytes(res.read_bytes()[:-100])
    with pytest.raises(RuntimeError, match="truncated"):
        codec.decompress_file_bounded(lossy, bad, batch_leaves=32)
    bad.write_bytes(b"VQVDB" + res.read_bytes()[5:])
    with pytest.raises(RuntimeError, match="magic"):
        codec.decompress_file_bounded(lossy, bad, batch_leaves=32)
    with pytest.raises(RuntimeError, match="Cannot open residual file"):
        codec.decompress_file_bounded(lossy, tmp_path / "absent.vqres")
    # the handle still works
    assert same(np.concatenate([g[3] for g in codec.decompress_file_bounded(lossy, res, batch_leaves=32)[0]]), out)
    # ... and a refused sidecar leaves no mode behind: the plain calls on the same handle
    assert same(np.concatenate([g[3] for g in codec.decompress_file(lossy, batch_leaves=32)[0]]), plain) and same(codec.decode(idx), plain)
    assert np.array_equal(codec.encode(leaves), idx) and same(codec.decode(codec.encode(leaves)), plain)
    keep = np.setdiff1d(np.arange(N), ids)
    assert same(plain[keep], out[keep]) and not same(plain, out)


def test_file_pair_on_a_grid_whose_single_batch_is_cut_into_pieces(codec, leaves, bounded, tmp_path):
    """16 400 leaves in one grid and one batch: the host pipeline cuts a call of >= 16 384 leaves that fits one chunk into
    pieces, so the stream's consumer sees offsets inside the batch (sidecar indices included)."""
    tol, err, idx, ids, raw, out = bounded
    reps = 16400 // N + 1
    x = np.ascontiguousarray(np.tile(leaves, (reps, 1))[:16400])
    want = np.tile(out, (reps, 1))[:16400]
    grids = [("density", np.zeros((16400, 3), np.int32), x, None)]
    lossy, res = tmp_path / "big.vqvdb", tmp_path / "big.vqres"
    _, bst = codec.compress_file_bounded(lossy, res, grids, tol)
    assert bst["outliers"] == np.isin(np.arange(16400) % N, ids).sum()
    got, _ = codec.decompress_file_bounded(lossy, res)
    assert same(got[0][3], want)
    plain, _ = codec.decompress_file(lossy)
    assert same(plain[0][3], np.tile(codec.decode(idx), (reps, 1))[:16400])


def test_argument_errors_leave_the_handle_usable(codec, leaves):
    lib, h = codec._lib, codec._h
    x = np.ascontiguousarray(leaves[:4])
    idx, ids, err = np.zeros((4, 64), np.uint8), np.full(4, -1, np.int64), np.zeros((4, 2), np.float32)
    out = np.zeros((4, 512), np.float32)
    cnt = ctypes.c_int64(-5)
    p = lambda a: a.ctypes.data   # noqa: E731
    msg = lambda: lib.vqhip_last_error(h).decode()   # noqa: E731
    assert lib.vqhip_compress_bounded(h, p(x), -1, 0.5, p(idx), p(err), p(ids), ctypes.byref(cnt)) == -1 and "n_leaves < 0" in msg()
    assert lib.vqhip_compress_bounded(h, None, 4, 0.5, p(idx), p(err), p(ids), ctypes.byref(cnt)) == -1 and "null pointer" in msg()
    assert lib.vqhip_compress_bounded(h, p(x), 4, 0.5, None, p(err), p(ids), ctypes.byref(cnt)) == -1 and "null pointer" in msg()
    assert lib.vqhip_compress_bounded(h, p(x), 4, 0.5, p(idx), p(err), None, ctypes.byref(cnt)) == -1 and "null pointer" in msg()
    assert lib.vqhip_compress_bounded(h, p(x), 4, 0.5, p(idx), p(err), p(ids), None) == -1 and "n_outliers is NULL" in msg()
    assert lib.vqhip_compress_bounded(h, None, 0, 0.5, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
    cnt = ctypes.c_int64(-5)
    assert lib.vqhip_compress_bounded(h, p(x), 4, -1.0, p(idx), None, p(ids), ctypes.byref(cnt)) == 0      # leaf_err may be NULL
    assert cnt.value == 4 and ids.tolist() == [0, 1, 2, 3]
    # decompress_bounded validates the ids before any GPU work
    two = np.array([2, 1], np.int64)
    assert lib.vqhip_decompress_bounded(h, p(idx), 4, p(two), 2, p(x), p(out)) == -1 and "not ascending" in msg()
    two[:] = (1, 1)
    assert lib.vqhip_decompress_bounded(h, p(idx), 4, p(two), 2, p(x), p(out)) == -1 and "not ascending" in msg()
    two[:] = (1, 4)
    assert lib.vqhip_decompress_bounded(h, p(idx), 4, p(two), 2, p(x), p(out)) == -1 and "is not in [0, 4)" in msg()
    assert lib.vqhip_decompress_bounded(h, p(idx), -1, p(two), 2, p(x), p(out)) == -1 and "n_leaves < 0" in msg()
    assert lib.vqhip_decompress_bounded(h, None, 4, p(two), 2, p(x), p(out)) == -1 and "null pointer" in msg()
    assert lib.vqhip_decompress_bounded(h, p(idx), 4, None, 2, p(x), p(out)) == -1 and "null pointer" in msg()
    assert lib.vqhip_decompress_bounded(h, p(idx), 4, p(two), 5, p(x), p(out)) == -1 and "more outliers than leaves" in msg()
    assert not out.any()
    assert lib.vqhip_decompress_bounded(h, None, 0, None, 0, None, None) == 0
    # the device calls
    assert lib.vqhip_roundtrip_device(h, None, -1, None, None, None, None) == -1 and "n_leaves < 0" in msg()
    assert lib.vqhip_roundtrip_device(h, None, 0, None, None, None, None) == 0
    assert lib.vqhip_roundtrip_device(h, None, 4, None, None, None, None) == -1 and "null pointer" in msg()
    de = torch.zeros((4, 2), device="cuda")
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    assert lib.vqhip_roundtrip_device(h, dx.data_ptr(), 4, None, None, None, None) == -1 and "leaf_err_dev" in msg()
    assert lib.vqhip_select_outliers_device(h, de.data_ptr(), -1, 0.5, None, None, None) == -1 and "n_leaves < 0" in msg()
    assert lib.vqhip_select_outliers_device(h, de.data_ptr(), 4, 0.5, None, None, None) == -1 and "count_dev is NULL" in msg()
    dc = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.vqhip_select_outliers_device(h, de.data_ptr(), 4, 0.5, None, dc.data_ptr(), None) == -1 and "null pointer" in msg()
    assert lib.vqhip_select_outliers_device(h, None, 0, 0.5, None, dc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(dc.item()) == 0
    # the file pair
    assert lib.vqhip_compress_file_bounded(h, b"a", None, None, 1, 0, 0.5, None, None) == -1 and "null path" in msg()
    assert lib.vqhip_decompress_file_bounded(h, b"a", None, 0, GRID_BEGIN_FN(), LEAF_ALLOC_FN(), None, None) == -1 and "null path" in msg()
    assert np.array_equal(codec.encode(x), dev_roundtrip(codec, x)[0])      # the handle still works
