"""The helpers and case bodies of tests/test_gpu_vec3_masked.py — TEST INFRASTRUCTURE: the device calls of
include/vqvdb_hip_vec3_mask.h on numpy arrays, the mask variants, and the cases, each held against tests/torch_ref_masked.py to the
bit.  They take the channel count C as the restatement does; the library has masked calls for C = 3 only."""
import ctypes

import numpy as np
import torch

import torch_ref_masked as trm

F = np.float32
FILL = 0xA5
SIZES = (1, 3, 4, 5, 33)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def sentinels(C):
    return trm._sentinels(C)


def to_dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def stream_of(stream):
    return stream.cuda_stream if stream is not None else 0


def mask_variants(x, C, designed_active, nonzero_from=0):
    """bool [n,512] per name: all ones, all zeros, random at densities 0.5 and 0.05, x != 0 (on the leaves from ``nonzero_from``
    on, ones before), one full word with seven empty, and ones with the designed input's own masks on its leaves (the last 9)."""
    n = len(x)
    rng = np.random.default_rng(77)
    nz = (np.asarray(x).reshape(n, 512, C) != 0).any(axis=2)
    nz[:nonzero_from] = True
    word = np.zeros((n, 512), bool)
    for i in range(n):
        word[i, 64 * (i % 8):64 * (i % 8) + 64] = True
    own = np.ones((n, 512), bool)
    own[n - len(designed_active):] = designed_active
    return {"ones": np.ones((n, 512), bool), "zeros": np.zeros((n, 512), bool), "half": rng.random((n, 512)) < 0.5,
            "sparse": rng.random((n, 512)) < 0.05, "nonzero": nz, "one_word": word, "designed": own}


def tolerances(err):
    """min, q25, median, max of the finite unmasked errors, then inf, 0, NaN"""
    e = err[:, 0]
    e = e[np.isfinite(e)]
    return [float(e.min()), float(np.quantile(e, 0.25, method="lower")), float(np.median(e)), float(e.max()), float("inf"), 0.0, float("nan")]


def dev_err(codec, x, recon, masks, stream=None):
    n = len(x)
    dx, dr, dm = to_dev(x, F), to_dev(recon, F), to_dev(masks)
    de = torch.full((n + 1, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.mask_leaf_err_device(dx.data_ptr(), dr.data_ptr(), dm.data_ptr(), n, de.data_ptr(), stream_of(stream))
    torch.cuda.synchronize()
    out = de.cpu().numpy()
    assert (out[n] == -7.0).all(), "errors written past the batch"
    return out[:n]


def dev_encode(codec, C, x, recon, masks, err, tol, capacity=None, stream=None):
    """-> (code [n], offsets [n+1], the whole payload buffer of n * 2048 C bytes, filled with FILL before)"""
    n = len(x)
    dx, dr, dm, de = to_dev(x, F), to_dev(recon, F), to_dev(masks), to_dev(err, F)
    dc = torch.full((n,), 77, dtype=torch.uint8 if C == 1 else torch.int16, device="cuda")
    do = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    dp = torch.full((n * 2048 * C,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    codec.mask_residual_encode_device(dx.data_ptr(), dr.data_ptr(), dm.data_ptr(), de.data_ptr(), n, tol, dc.data_ptr(), do.data_ptr(), dp.data_ptr(),
                                      n * 2048 * C if capacity is None else capacity, stream_of(stream))
    torch.cuda.synchronize()
    code = dc.cpu().numpy()
    return (code if C == 1 else code.view(np.uint16)), do.cpu().numpy(), dp.cpu().numpy()


def dev_apply(codec, C, recon, tol, code, off, payload):
    """the EXISTING apply call on masked records"""
    n = len(recon)
    dr, dc, do = to_dev(recon, F), to_dev(code), to_dev(off, np.int64)
    dp = to_dev(np.frombuffer(bytes(payload) + bytes(8), dtype=np.uint8).copy())
    torch.cuda.synchronize()
    codec.residual_apply_device(dr.data_ptr(), n, tol, dc.data_ptr(), do.data_ptr(), dp.data_ptr())
    torch.cuda.synchronize()
    return dr.cpu().numpy()


class Resident:
    """leaves, reconstruction, masks and masked errors on the device, swept in slices through the library's own entry point (the
    wrapper refuses the negative rungs that the C call takes)"""

    def __init__(self, codec, C, x, recon, masks, err):
        self.codec, self.C, self.classes = codec, C, 16 * C + 3
        self.x, self.r, self.m, self.e = to_dev(x, F), to_dev(recon, F), to_dev(masks), to_dev(err, F)
        self.call = codec._lib.vqhip_vec3_mask_sweep_device

    def sweep(self, tols, lo=0, n=None, hist=None, stream=None, rows=None):
        n = len(self.x) - lo if n is None else n
        t = np.asarray(tols, F)
        if hist is None:
            hist = torch.zeros((len(t) if rows is None else rows, self.classes), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = self.call(self.codec._h, self.x[lo:].data_ptr(), self.r[lo:].data_ptr(), self.m[lo:].data_ptr(), self.e[lo:].data_ptr(), n, t.ctypes.data,
                       len(t), hist.data_ptr(), stream_of(stream) or None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return hist


# ---- the cases ----
def case_error(codec, C, x, recon, active, uerr):
    """the masked error equals the restatement to the bit: every batch size, front and back, a second stream"""
    n = len(x)
    masks = trm.pack_masks(active)
    want = trm.leaf_err_fixed(x, recon, active, C)
    got = dev_err(codec, x, recon, masks)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (bad[:8], got[bad][:4], want[bad][:4])
    second = torch.cuda.Stream()
    for m in SIZES:
        for lo, stream in ((0, None), (n - m, second)):
            assert same(dev_err(codec, x[lo:lo + m], recon[lo:lo + m], masks[lo:lo + m], stream), want[lo:lo + m]), (m, lo)
    if uerr is not None and active.all():
        assert same(got, uerr)
    if not active.any():
        assert got.tobytes() == np.zeros_like(got).tobytes()
    return got


def case_encode(codec, C, x, recon, active, tols):
    """codes, offsets and payload equal the restatement to the bit; bytes beyond the total are untouched; a capacity one byte short
    of a record leaves that record unwritten; invariance under batch, place and stream"""
    n = len(x)
    KEPT, RAW = sentinels(C)
    masks = trm.pack_masks(active)
    err = trm.leaf_err_fixed(x, recon, active, C)
    second = torch.cuda.Stream()
    out = {}
    for tol in tols:
        code, off, buf = dev_encode(codec, C, x, recon, masks, err, tol)
        rcode, roff = trm.classify(x, recon, err, tol, active, C)
        bad = np.flatnonzero(code != rcode)
        assert len(bad) == 0, (tol, bad[:8], code[bad][:8], rcode[bad][:8])
        assert np.array_equal(off, roff), tol
        total = int(off[-1])
        want = np.frombuffer(trm.pack(x, recon, tol, rcode, active, C), dtype=np.uint8)
        assert len(want) == total and np.array_equal(buf[:total], want), tol
        assert (buf[total:] == FILL).all(), "bytes written beyond the total"
        for m in SIZES:
            for lo, stream in ((0, None), (n - m, second)):
                c2, o2, b2 = dev_encode(codec, C, x[lo:lo + m], recon[lo:lo + m], masks[lo:lo + m], err[lo:lo + m], tol, stream=stream)
                assert np.array_equal(c2, code[lo:lo + m]) and np.array_equal(o2, off[lo:lo + m + 1] - off[lo]), (tol, m, lo)
                assert np.array_equal(b2[:o2[-1]], buf[off[lo]:off[lo + m]]) and (b2[o2[-1]:] == FILL).all(), (tol, m, lo)
        sized = np.flatnonzero(np.diff(off) > 0)
        if len(sized):
            last = int(sized[-1])                                      # the last record that has bytes: one byte short of it
            c3, o3, b3 = dev_encode(codec, C, x, recon, masks, err, tol, capacity=int(off[last + 1]) - 1)
            assert np.array_equal(c3, code) and np.array_equal(o3, off)
            assert np.array_equal(b3[:off[last]], buf[:off[last]]) and (b3[off[last]:] == FILL).all(), tol
        out[tol] = (code, off, buf[:total].copy())
    return err, out


def case_apply(codec, C, x, recon, active, err, tol, code, off, payload):
    """the existing apply call on masked records gives the post-conditions of the contract"""
    KEPT, RAW = sentinels(C)
    out = dev_apply(codec, C, recon, tol, code, off, payload)
    assert same(out, trm.apply(recon, tol, code, payload.tobytes(), C))
    xs, rs, act = trm._values(x, C), trm._values(recon, C), trm._active(active, C)
    out = out.reshape(xs.shape)
    step = F(1.875) * F(tol)
    kept, raw = code == KEPT, code == RAW
    quant = ~kept & ~raw
    assert same(out[kept], rs[kept]) and same(out[raw], xs[raw])
    with np.errstate(invalid="ignore"):
        d = np.abs(xs - out)
    assert (d[quant][act[quant]] <= F(tol)).all(), tol                 # the bound, with the decoder's own arithmetic
    assert same(out[quant][~act[quant]], (rs + F(0) * step)[quant][~act[quant]])
    with np.errstate(invalid="ignore"):
        assert (np.abs(xs - rs)[kept][act[kept]] <= F(tol)).all()      # a kept leaf is within the bound on its active values
    return out


def case_sweep(codec, C, x, recon, active, err, encode_codes, tols):
    """the masked sweep equals the restatement and the masked encoder's own class counts at 1, 16 and 64 rungs; it accumulates"""
    n = len(x)
    masks = trm.pack_masks(active)
    dev = Resident(codec, C, x, recon, masks, err)
    classes = 16 * C + 3
    base = [t for t in tols]
    hist = dev.sweep(base).cpu().numpy()
    assert np.array_equal(hist, trm.sweep(x, recon, err, base, active, C)), hist
    for t, tol in enumerate(base):
        if tol in encode_codes:
            assert np.array_equal(hist[t], np.bincount(trm.columns(encode_codes[tol][0], C), minlength=classes)), tol
    assert (hist.sum(axis=1) == n).all()
    one = dev.sweep(base[2:3], rows=64).cpu().numpy()
    assert np.array_equal(one[0], hist[2]) and not one[1:].any()
    extra = [-1.0, -0.0, float("-inf")]                                # negative rungs and -0 through the C call
    sixteen = (base + extra + [base[2] / 2, base[2] * 2, base[2] / 8, base[2] * 8, base[1] * 3, base[3] / 3])[:16]
    assert len(sixteen) == 16
    got = dev.sweep(sixteen).cpu().numpy()
    assert np.array_equal(got, trm.sweep(x, recon, err, sixteen, active, C))
    med = base[2] if base[2] > 0 else 1e-3
    many = ([float(v) for v in np.geomspace(med / 64, med * 64, 64 - len(sixteen)).astype(F)] + sixteen)
    assert len(many) == 64
    got = dev.sweep(many).cpu().numpy()
    assert np.array_equal(got, trm.sweep(x, recon, err, many, active, C))
    both = dev.sweep(base, 0, n // 2)                                  # two calls on the two halves add up to the one call
    both = dev.sweep(base, n // 2, n - n // 2, hist=both, stream=torch.cuda.Stream()).cpu().numpy()
    assert np.array_equal(both, hist)
    return hist


def case_sweep_4099(codec, C):
    """4 099 leaves with synthetic x^ (the designed input, tiled; the model is not run): the stride loop above RATE_MAX_GRID *
    RATE_WAVES = 4 096 leaves runs"""
    x, recon, active, _ = trm.designed(C)
    n = 4099
    pick = np.arange(n) % len(x)
    err = trm.leaf_err_fixed(x, recon, active, C)
    tols = [trm.TOL_D, trm.TOL_D / 4, 0.0, float("nan"), float("inf"), 4 * trm.TOL_D, -1.0]
    want = np.zeros((len(tols), 16 * C + 3), np.int64)
    weight = np.bincount(pick, minlength=len(x))
    for t, tol in enumerate(tols):
        np.add.at(want[t], trm.columns(trm.classify(x, recon, err, tol, active, C)[0], C), weight)
    dev = Resident(codec, C, x[pick], recon[pick], trm.pack_masks(active[pick]), err[pick])
    got = dev.sweep(tols).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    assert (got.sum(axis=1) == n).all() and got[0, 16 * C + 2] > 0 and got[0, 16 * C + 1] > 0


def case_refusals(codec, C, x, recon, active):
    lib, h = codec._lib, codec._h
    pre, last = "vqhip_vec3_mask_", lib.vqhip_vec3_last_error
    n = len(x)
    masks = trm.pack_masks(active)
    err = trm.leaf_err_fixed(x, recon, active, C)
    dx, dr, dm, de = to_dev(x, F), to_dev(recon, F), to_dev(masks), to_dev(err, F)
    dc, do = torch.zeros(n, dtype=torch.int16, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    dp = torch.zeros(n * 2048 * C, dtype=torch.uint8, device="cuda")
    hist = torch.zeros((64, 16 * C + 3), dtype=torch.int64, device="cuda")
    t1 = np.array([0.5], F)
    p = lambda t: t.data_ptr()                                         # noqa: E731
    assert getattr(lib, pre + "leaf_err_device")(h, p(dx), p(dr), None, n, p(de), None) == -1 and "null pointer" in last(h).decode()
    assert getattr(lib, pre + "residual_encode_device")(h, p(dx), p(dr), None, p(de), n, 0.5, p(dc), p(do), p(dp), n * 2048 * C, None) == -1
    assert "null pointer" in last(h).decode()
    assert getattr(lib, pre + "sweep_device")(h, p(dx), p(dr), None, p(de), n, t1.ctypes.data, 1, p(hist), None) == -1 and "null pointer" in last(h).decode()
    for bad in (0, 65, -1):
        assert getattr(lib, pre + "sweep_device")(h, p(dx), p(dr), p(dm), p(de), n, t1.ctypes.data, bad, p(hist), None) == -1
        assert "n_tols" in last(h).decode()
    # n == 0 returns OK and touches nothing, whatever the pointers
    assert getattr(lib, pre + "leaf_err_device")(h, None, None, None, 0, None, None) == 0
    assert getattr(lib, pre + "residual_encode_device")(h, None, None, None, None, 0, 0.5, None, None, None, 0, None) == 0
    assert getattr(lib, pre + "sweep_device")(h, None, None, None, None, 0, t1.ctypes.data, 1, None, None) == 0
    nbytes = ctypes.c_int64(-1)
    assert getattr(lib, pre + "compress_residual")(h, None, None, 0, 0.5, None, None, None, None, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    hh = np.full((1, 16 * C + 3), -1, np.int64)
    assert getattr(lib, pre + "sweep")(h, None, None, 0, t1.ctypes.data, 1, hh.ctypes.data) == 0 and not hh.any()
    assert getattr(lib, pre + "compress_residual")(h, x.ctypes.data, None, n, 0.5, None, None, None, None, ctypes.byref(nbytes)) == -1
    assert getattr(lib, pre + "sweep")(h, x.ctypes.data, None, n, t1.ctypes.data, 1, hh.ctypes.data) == -1 and "null pointer" in last(h).decode()
    torch.cuda.synchronize()
    assert not hist.any().item()
    assert same(dev_err(codec, x, recon, masks), err)                  # the handle still works
