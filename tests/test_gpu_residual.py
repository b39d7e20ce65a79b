"""Quantised residuals of the scalar handle on the GPU: classes, offsets and payload of residual_encode_device
against tests/torch_ref_residual.py to the bit, invariance under batch, place and stream, a synthetic call with every class,
residual_apply_device, the host pair's tolerance guarantee, the .vqvdb + .vqres v2 file pair and the refusals.  Every case runs
with the automatic small-batch kernels and with set_small_batch_tiles(0), on the 136 leaves of tests/test_gpu_bounded.py."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_residual as trr  # noqa: E402
from vqvdb_amd import synth, vqvdbfile, weightpack  # noqa: E402
from vqvdb_amd.codec import HipCodec  # noqa: E402

pytestmark = pytest.mark.gpu

N = 136
SIZES = (1, 3, 33, 136)
F = np.float32
FILL = 0xA5


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


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def dev_roundtrip(codec, x):
    n = len(x)
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    dr = torch.zeros((n, 512), dtype=torch.float32, device="cuda")
    de = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.roundtrip_device(dx.data_ptr(), n, de.data_ptr(), di.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    return di.cpu().numpy(), de.cpu().numpy(), dr.cpu().numpy()


def dev_encode(codec, x, recon, err, tol, capacity=None, stream=None):
    """vqhip_residual_encode_device -> (class [n], offsets [n+1], the whole payload buffer of n * 2048 bytes, filled with FILL before)."""
    n = len(x)
    dx, dr = torch.from_numpy(np.ascontiguousarray(x, F)).cuda(), torch.from_numpy(np.ascontiguousarray(recon, F)).cuda()
    de = torch.from_numpy(np.ascontiguousarray(err, F)).cuda()
    dc = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    do = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    dp = torch.full((n * 2048,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    codec.residual_encode_device(dx.data_ptr(), dr.data_ptr(), de.data_ptr(), n, tol, dc.data_ptr(), do.data_ptr(), dp.data_ptr(),
                                 n * 2048 if capacity is None else capacity, stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return dc.cpu().numpy(), do.cpu().numpy(), dp.cpu().numpy()


def dev_apply(codec, recon, tol, cls, off, payload, stream=None):
    n = len(recon)
    dr = torch.from_numpy(np.ascontiguousarray(recon, F)).cuda()
    dc, do = torch.from_numpy(np.ascontiguousarray(cls)).cuda(), torch.from_numpy(np.ascontiguousarray(off)).cuda()
    dp = torch.from_numpy(np.frombuffer(bytes(payload) + bytes(8), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    codec.residual_apply_device(dr.data_ptr(), n, tol, dc.data_ptr(), do.data_ptr(), dp.data_ptr(), stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return dr.cpu().numpy()


def check_against_restatement(codec, x, recon, err, tol, capacity=None, stream=None):
    cls, off, buf = dev_encode(codec, x, recon, err, tol, capacity, stream)
    rcls, roff = trr.classify(x, recon, err, tol)
    assert np.array_equal(cls, rcls), (tol, np.flatnonzero(cls != rcls)[:8], cls[cls != rcls][:8], rcls[cls != rcls][:8])
    assert np.array_equal(off, roff), tol
    total = int(off[-1])
    if capacity is not None:                                         # the caller compares the bytes with a full call's
        return cls, off, buf, None
    want = np.frombuffer(trr.pack(x, recon, tol, rcls), dtype=np.uint8)
    assert len(want) == total
    assert np.array_equal(buf[:total], want), tol
    assert (buf[total:] == FILL).all(), "bytes written beyond the total"
    return cls, off, buf, want


def test_encode_device_equals_the_restatement_at_five_tolerances(codec, leaves):
    _, err, rec = dev_roundtrip(codec, leaves)
    e = err[:, 0]
    med = float(np.median(e))
    for tol in (float(e.min()), float(np.quantile(e, 0.25, method="lower")), med, float(e.max()), float("inf")):
        cls, off, buf, want = check_against_restatement(codec, leaves, rec, err, tol)
        for n in SIZES:                                              # the same bits at every batch size, place and stream
            for lo, stream in ((0, None), (N - n, torch.cuda.Stream())):
                c2, o2, b2 = dev_encode(codec, leaves[lo:lo + n], rec[lo:lo + n], err[lo:lo + n], tol, stream=stream)
                assert np.array_equal(c2, cls[lo:lo + n]) and np.array_equal(o2, off[lo:lo + n + 1] - off[lo]), (tol, n, lo)
                assert np.array_equal(b2[:o2[-1]], buf[off[lo]:off[lo + n]]) and (b2[o2[-1]:] == FILL).all(), (tol, n, lo)
        if tol == med:
            sel = cls != trr.KEPT
            hist = {int(c): int((cls == c).sum()) for c in np.unique(cls)}
            print(f"tol {tol:.4f}: classes {hist}, payload {off[-1]} B against {sel.sum()} x 2048 = {sel.sum() * 2048} B")
            assert sel.sum() == 68 and ((cls <= 16).sum()) >= 66
        if tol == float("inf"):
            assert (cls == trr.KEPT).all() and off[-1] == 0
        if tol == float(e.max()):
            assert (cls == trr.KEPT).all()


TOL_S = float(np.float32(0.66))   # a float32 value: the wrapper rounds a tolerance down to float32, never up


def synthetic_leaves():
    """19 leaves that need no model, (x, x^, err) for tol = TOL_S: classes 0 .. 16 (x^ = 0, x = q * step, so x~ = x), a 17-bit
    leaf (raw), and a leaf whose only failure is one voxel beside a rounding tie (x^ so large that x^ + q * step rounds a
    whole ulp away from x); then a NaN and an inf leaf appended (21 in all)."""
    qmax = [0, -1] + [1 << (b - 2) for b in range(2, 17)] + [32768]
    pairs = [trr.leaf_with_max_q(abs(q), TOL_S, np.random.default_rng(b), negative=q < 0) for b, q in enumerate(qmax)]
    x, recon = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    tx, tr = trr.leaf_with_max_q(3, TOL_S, np.random.default_rng(99))
    found = None
    for base in (2.0 ** 21, 2.0 ** 22, 2.0 ** 23):
        ulp = float(np.spacing(F(base)))
        for j in range(1, 64):
            cx, cr = tx.copy(), tr.copy()
            cr[300], cx[300] = F(base), F(base + j * ulp)
            t = (cx[300] - cr[300]) / trr.step_of(TOL_S)
            _, ok = trr.quantise(cx[None], cr[None], TOL_S)
            if not ok[0, 300] and ok[0].sum() == 511 and abs(abs(float(t)) % 1.0 - 0.5) < 0.07:
                found = (cx, cr)
                break
        if found:
            break
    assert found is not None, "no tie voxel found that the rounding of x^ + q * step pushes past tol"
    x, recon = np.concatenate([x, found[0][None]]), np.concatenate([recon, found[1][None]])
    nan_leaf, inf_leaf = x[5].copy(), x[6].copy()
    nan_leaf.view(np.uint32)[300] = 0x7FC12345
    inf_leaf[17] = -np.inf
    x, recon = np.concatenate([x, nan_leaf[None], inf_leaf[None]]), np.concatenate([recon, recon[5:7]])
    with np.errstate(invalid="ignore"):
        d = np.abs(x - recon)
    err = np.where(np.isfinite(d).all(axis=1), d.max(axis=1), np.nan).astype(F)
    err[0] = 1.0
    return np.ascontiguousarray(x), np.ascontiguousarray(recon), np.stack([err, err], axis=1)


def test_synthetic_call_with_every_class(codec):
    x, recon, err = synthetic_leaves()
    cls, off, buf, want = check_against_restatement(codec, x[:19], recon[:19], err[:19], TOL_S)
    assert cls.tolist() == list(range(17)) + [trr.RAW, trr.RAW]
    cls, off, buf, want = check_against_restatement(codec, x, recon, err, TOL_S)
    assert cls[19:].tolist() == [trr.RAW, trr.RAW]
    assert same(buf[off[19]:off[20]], x[19].view(np.uint8))         # the NaN payload as it went in
    # more than two scan steps of 8192 leaves, kept leaves in between, every class at changing places
    n = 2 * 8192 + 1500
    rng = np.random.default_rng(4)
    pick = rng.integers(0, len(x), n)
    bx, br, be = x[pick], recon[pick], err[pick].copy()
    keep = rng.random(n) < 0.4
    keep[8000:8400] = True
    keep[16380:16390] = False
    be[keep & np.isfinite(be[:, 0])] = 0.25
    cls, off, buf, want = check_against_restatement(codec, bx, br, be, TOL_S)
    assert (cls == trr.KEPT).sum() > 5000 and len(np.unique(cls)) == 19 and off[-1] > 2 * 8192 * 64
    out = dev_apply(codec, br, TOL_S, cls, off, buf[:off[-1]])
    assert same(out, trr.apply(br, TOL_S, cls, want.tobytes()))
    # one byte short: the last record is not written at all, everything else is identical
    last = int(np.flatnonzero(trr.record_size(cls) > 0)[-1])
    c2, o2, b2, _ = check_against_restatement(codec, bx, br, be, TOL_S, capacity=int(off[-1]) - 1)
    assert np.array_equal(c2, cls) and np.array_equal(o2, off)
    assert np.array_equal(b2[:off[last]], buf[:off[last]]) and (b2[off[last]:] == FILL).all()
    c3, o3, b3 = dev_encode(codec, bx, br, be, TOL_S, capacity=0)
    assert np.array_equal(c3, cls) and np.array_equal(o3, off) and (b3 == FILL).all()


def test_apply_device_equals_the_restatement(codec, leaves):
    idx, err, rec = dev_roundtrip(codec, leaves)
    tol = float(np.median(err[:, 0]))
    cls, off = trr.classify(leaves, rec, err, tol)
    payload = trr.pack(leaves, rec, tol, cls)
    want = trr.apply(rec, tol, cls, payload)
    for stream in (None, torch.cuda.Stream()):
        out = dev_apply(codec, rec, tol, cls, off, payload, stream)
        assert same(out, want)
    kept = cls == trr.KEPT
    assert same(out[kept], rec[kept]) and not same(out[~kept], rec[~kept])
    raw = np.full(N, trr.RAW, np.uint8)                              # every leaf raw: bit-exact copies
    out = dev_apply(codec, rec, tol, raw, np.arange(N + 1, dtype=np.int64) * 2048, leaves.tobytes())
    assert same(out, leaves)
    for n in SIZES[:3]:
        assert same(dev_apply(codec, rec[N - n:], tol, cls[N - n:], off[N - n:] - off[N - n], payload[off[N - n]:]), want[N - n:]), n


@pytest.fixture()
def resid(codec, leaves):
    """tol = the median leaf error; what compress_residual -> decompress_residual returns for the 136 leaves."""
    _, err = codec.roundtrip(leaves)
    tol = float(np.median(err[:, 0]))
    idx, cls, payload = codec.compress_residual(leaves, tol)
    return tol, err, idx, cls, payload, codec.decompress_residual(idx, tol, cls, payload)


def test_the_host_pair_keeps_every_leaf_within_the_tolerance(codec, pack, leaves, resid):
    tol, err, idx, cls, payload, out = resid
    worst = np.abs(leaves - out).max(axis=1)
    sel = cls != trr.KEPT
    print(f"tol {tol:.4f}: {sel.sum()} of {N} leaves selected, {(cls == trr.RAW).sum()} raw, {len(payload)} payload bytes, largest error {worst.max():.4f}")
    assert np.isfinite(leaves).all() and (worst <= F(tol)).all()
    assert np.array_equal(idx, codec.encode(leaves))
    plain = codec.decode(idx)
    assert same(out[~sel], plain[~sel]) and not same(out[sel], plain[sel])
    _, derr, drec = dev_roundtrip(codec, leaves)
    dcls, doff, dbuf = dev_encode(codec, leaves, drec, derr, tol)
    assert np.array_equal(cls, dcls) and same(payload, dbuf[:doff[-1]])
    assert same(out, trr.apply(drec, tol, dcls, payload.tobytes()))
    i2, c2, p2, e2 = codec.compress_residual(leaves[:33], tol, return_leaf_err=True)
    assert same(e2, err[:33]) and np.array_equal(c2, cls[:33]) and same(p2, payload[:doff[33]])
    assert same(codec.decompress_residual(i2, tol, c2, p2), out[:33])
    small = HipCodec(pack)                                           # chunks of 32, 32, 32, 32, 8: records concatenated over the call
    try:
        small.set_chunk_leaves(32)
        si, sc, sp = small.compress_residual(leaves, tol)
        assert np.array_equal(si, idx) and np.array_equal(sc, cls) and same(sp, payload)
        assert same(small.decompress_residual(si, tol, sc, sp), out)
    finally:
        small.close()
    # non-finite leaves come back bit for bit and touch no other leaf
    bad = leaves.copy()
    bad.view(np.uint32)[5, 300] = 0x7FC12345
    bad[N - 2, 17] = np.inf
    bi, bc, bp = codec.compress_residual(bad, tol)
    ok = np.setdiff1d(np.arange(N), [5, N - 2])
    assert bc[5] == trr.RAW and bc[N - 2] == trr.RAW and np.array_equal(bc[ok], cls[ok])
    bout = codec.decompress_residual(bi, tol, bc, bp)
    assert same(bout[[5, N - 2]], bad[[5, N - 2]]) and same(bout[ok], out[ok])
    ic, icls, ip = codec.compress_residual(bad, float("inf"))
    assert np.array_equal(np.flatnonzero(icls != trr.KEPT), [5, N - 2]) and len(ip) == 4096
    # a wrong class or payload length is refused before any GPU work and the handle stays usable
    lib, h = codec._lib, codec._h
    o4 = np.zeros((N, 512), F)
    wrong = cls.copy()
    wrong[3] = 17
    p = lambda a: a.ctypes.data   # noqa: E731
    assert lib.vqhip_decompress_residual(h, p(idx), N, tol, p(wrong), p(payload), len(payload), p(o4)) == -1
    assert "class 17 of leaf 3" in lib.vqhip_last_error(h).decode()
    assert lib.vqhip_decompress_residual(h, p(idx), N, tol, p(cls), p(payload), len(payload) - 64, p(o4)) == -1
    assert "payload bytes" in lib.vqhip_last_error(h).decode() and not o4.any()
    assert lib.vqhip_decompress_residual(h, None, 0, tol, None, None, 0, None) == 0
    nb = np.zeros(1, np.int64)
    assert lib.vqhip_compress_residual(h, None, 0, tol, None, None, None, None, p(nb)) == 0
    assert lib.vqhip_compress_residual(h, p(leaves), N, tol, None, None, p(wrong), p(o4), p(nb)) == -1 and "null pointer" in lib.vqhip_last_error(h).decode()
    assert lib.vqhip_residual_encode_device(h, None, None, None, 0, tol, None, None, None, 0, None) == 0
    assert lib.vqhip_residual_encode_device(h, None, None, None, 4, tol, None, None, None, 0, None) == -1
    assert lib.vqhip_residual_apply_device(h, None, 4, tol, None, None, None, None) == -1 and "null pointer" in lib.vqhip_last_error(h).decode()
    assert same(codec.decompress_residual(idx, tol, cls, payload), out)


def grids_of(leaves):
    org = np.arange(N * 3, dtype=np.int32).reshape(N, 3) * 8
    tr = np.arange(16, dtype=np.float32)
    return [("density", org[:70], np.ascontiguousarray(leaves[:70]), tr), ("temperature", org[70:], np.ascontiguousarray(leaves[70:]), None)]


def cat(got):
    return np.concatenate([g[3] for g in got])


@pytest.mark.parametrize("batch", (32, 0), ids=("batches_of_32", "one_batch_per_grid"))
def test_file_pair(codec, leaves, resid, tmp_path, batch):
    tol, err, idx, cls, payload, out = resid
    grids = grids_of(leaves)
    plain, lossy, res = tmp_path / "plain.vqvdb", tmp_path / "r.vqvdb", tmp_path / "r.vqres"
    codec.compress_file(plain, grids, batch_leaves=batch)
    st, bst, rst = codec.compress_file_residual(lossy, res, grids, tol, batch_leaves=batch)
    assert lossy.read_bytes() == plain.read_bytes()
    sel = cls != trr.KEPT
    assert st["leaves"] == N and bst["leaves"] == N and bst["outliers"] == sel.sum()
    assert rst == {"quantised": int((cls <= 16).sum()), "raw": int((cls == trr.RAW).sum()), "payload_bytes": len(payload)}
    assert bst["max_err_kept"] == err[~sel, 0].max() and bst["max_err_kept"] <= tol
    rtol, rg = vqvdbfile.load_residual_v2(res)
    assert rtol == HipCodec.check_tol(tol) and len(rg) == 2
    recs = trr.records(cls, payload.tobytes())
    for (rids, rcls, rrecs), lo, hi in zip(rg, (0, 70), (70, N)):
        want = np.flatnonzero(sel[lo:hi])
        assert np.array_equal(rids, want) and np.array_equal(rcls, cls[lo:hi][want])
        assert rrecs == [recs[lo + i] for i in want]
    got, dst = codec.decompress_file_residual(lossy, res, batch_leaves=batch)
    assert [g[0] for g in got] == ["density", "temperature"] and dst["leaves"] == N
    assert same(cat(got), out)
    assert same(cat(codec.decompress_file_residual(lossy, res, batch_leaves=0 if batch else 32)[0]), out)   # the other batching reads the same file
    assert same(cat(codec.decompress_file(lossy, batch_leaves=batch)[0]), codec.decode(idx))               # ignoring the sidecar
    # tol = NaN: every leaf raw, the pair is lossless; tol = +inf: an empty sidecar
    _, bnan, rnan = codec.compress_file_residual(lossy, res, grids, float("nan"), batch_leaves=batch)
    assert bnan["outliers"] == N and rnan["raw"] == N
    assert same(cat(codec.decompress_file_residual(lossy, res, batch_leaves=batch)[0]), leaves)
    _, binf, rinf = codec.compress_file_residual(lossy, res, grids, float("inf"), batch_leaves=batch)
    assert binf["outliers"] == 0 and rinf["payload_bytes"] == 0 and res.read_bytes()[11:] == struct.pack("<II", 0, 0)
    assert same(cat(codec.decompress_file_residual(lossy, res, batch_leaves=batch)[0]), codec.decode(idx))


def test_file_pair_refuses_a_sidecar_that_does_not_fit(codec, leaves, resid, tmp_path):
    tol, err, idx, cls, payload, out = resid
    grids = grids_of(leaves)
    lossy, res, bad = tmp_path / "b.vqvdb", tmp_path / "b.vqres", tmp_path / "bad.vqres"
    plain = codec.decode(idx)
    codec.compress_file_residual(lossy, res, grids, tol, batch_leaves=32)
    rtol, rg = vqvdbfile.load_residual_v2(res)
    assert len(rg[0][0]) >= 2 and len(rg[1][0]) >= 2

    def refused(match, grids_=None, raw=None):
        if raw is None:
            vqvdbfile.save_residual_v2(bad, rtol, grids_)
        else:
            bad.write_bytes(bytes(raw))
        with pytest.raises(RuntimeError, match=match):
            codec.decompress_file_residual(lossy, bad, batch_leaves=32)

    refused("holds 1 grids, the .vqvdb file 2", rg[:1])
    refused("holds 3 grids, the .vqvdb file 2", rg + [rg[0]])
    past = rg[1][0].copy()
    past[-1] = 66                                                    # the second grid has 66 leaves: 0 .. 65
    refused("record index 66 in grid 'temperature' of 66 leaves", [rg[0], (past, rg[1][1], rg[1][2])])
    buf = bytearray(res.read_bytes())
    first = 5 + trr.record_size(int(rg[0][1][0]))                    # the first entry's bytes; the second entry follows it
    rep = bytearray(buf)
    rep[15 + first:19 + first] = buf[15:19]                          # the second index repeats the first
    refused("is not ascending", raw=rep)
    rep = bytearray(buf)
    rep[19] = 17
    refused("class 17 of record", raw=rep)
    rep[19] = 254
    refused("class 254 of record", raw=rep)
    refused("truncated", raw=buf[:-100])
    refused("truncated", raw=buf[:13])
    refused("magic", raw=b"VQVDB" + bytes(buf[5:]))
    refused(r"version 1 \(expected 2\)", raw=bytes(buf[:5]) + b"\x01" + bytes(buf[6:]))
    with pytest.raises(RuntimeError, match=r"version 2 \(expected 1\)"):
        codec.decompress_file_bounded(lossy, res, batch_leaves=32)   # the v1 reader keeps refusing other versions
    with pytest.raises(RuntimeError, match="Cannot open residual file"):
        codec.decompress_file_residual(lossy, tmp_path / "absent.vqres")
    lib, h = codec._lib, codec._h
    assert lib.vqhip_compress_file_residual(h, b"a", None, None, 1, 0, 0.5, None, None, None) == -1 and "null path" in lib.vqhip_last_error(h).decode()
    assert same(cat(codec.decompress_file_residual(lossy, res, batch_leaves=32)[0]), out)       # the handle still works
    # ... and a refused sidecar leaves no mode behind: the plain calls on the same handle apply no records
    assert same(cat(codec.decompress_file(lossy, batch_leaves=32)[0]), plain) and same(codec.decode(idx), plain)
    assert np.array_equal(codec.encode(leaves), idx) and same(codec.decode(codec.encode(leaves)), plain)
    assert same(plain[cls == trr.KEPT], out[cls == trr.KEPT]) and not same(plain, out)


def test_file_pairs_on_a_batch_cut_into_pieces_of_64_64_and_8(request, codec, pack, leaves, resid, tmp_path, monkeypatch):
    """One grid of all 136 leaves in one batch, through a handle created with VQHIP_HOST_SPLIT=4,32 (32 is the smallest piece size
    the variable accepts): the host pipeline cuts the call into pieces of 64, 64 and 8 leaves, so the consumer and the decode stage
    see offsets inside the batch and both I/O slots.  The v2 pair and the v1 pair write the default handle's bytes and return the
    host pairs' leaves."""
    tol, err, idx, cls, payload, out = resid
    grids = [("density", np.arange(N * 3, dtype=np.int32).reshape(N, 3) * 8, leaves, None)]
    monkeypatch.setenv("VQHIP_HOST_SPLIT", "4,32")
    split = HipCodec(pack)
    monkeypatch.delenv("VQHIP_HOST_SPLIT")
    try:
        split.set_small_batch_tiles(request.node.callspec.params["codec"])
        bidx, ids, raw = codec.compress_bounded(leaves, tol)
        for name, want in (("residual", out), ("bounded", codec.decompress_bounded(bidx, ids, raw))):
            files = [tmp_path / f"{who}_{name}{ext}" for who in ("whole", "split") for ext in (".vqvdb", ".vqres")]
            getattr(codec, "compress_file_" + name)(files[0], files[1], grids, tol, batch_leaves=0)
            getattr(split, "compress_file_" + name)(files[2], files[3], grids, tol, batch_leaves=0)
            assert files[2].read_bytes() == files[0].read_bytes() and files[3].read_bytes() == files[1].read_bytes(), name
            assert len(files[1].read_bytes()) > 15, name                                       # the sidecar holds entries
            got, st = getattr(split, "decompress_file_" + name)(files[2], files[3], batch_leaves=0)
            assert st["leaves"] == N and same(cat(got), want), name
    finally:
        split.close()
