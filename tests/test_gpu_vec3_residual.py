"""Quantised residuals of the Vec3 handle on the GPU: codes, offsets and payload of residual_encode_device against
tests/torch_ref_vec3_residual.py to the bit, invariance under batch, place and stream, a model-free call with every width in
every channel, the capacity rule, residual_apply_device, the host pair's tolerance guarantee with its refusals, and the untouched
neighbours.  The leaves are synth_vec3.make_leaves(128, 4321) and the 8 edge leaves."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import synth_vec3, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

N = 136
SIZES = (1, 3, 5, 33, 136)
MODES = ("fp32", "bf16")
F = np.float32
FILL = 0xA5
RAW_BYTES = 6144


@pytest.fixture(scope="module")
def pack():
    return weightpack.dumps(synth_vec3.make_weights(0))


@pytest.fixture(scope="module")
def leaves():
    return np.ascontiguousarray(np.concatenate([synth_vec3.make_leaves(128, 4321), synth_vec3.edge_leaves()]))


@pytest.fixture(params=MODES)
def codec(request, pack):
    c = HipVec3Codec(pack, precision=request.param)
    yield c
    c.close()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def dev_roundtrip(codec, x):
    n = len(x)
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = torch.zeros((n, 64), dtype=torch.int16, device="cuda")
    dr = torch.zeros((n, 512, 3), dtype=torch.float32, device="cuda")
    de = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.roundtrip_device(dx.data_ptr(), n, de.data_ptr(), di.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    return di.cpu().numpy().view(np.uint16), de.cpu().numpy(), dr.cpu().numpy()


def dev_decode(codec, idx):
    n = len(idx)
    di = torch.from_numpy(np.ascontiguousarray(idx).view(np.int16)).cuda()
    do = torch.zeros((n, 512, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_device(di.data_ptr(), n, do.data_ptr())
    torch.cuda.synchronize()
    return do.cpu().numpy()


def dev_encode(codec, x, recon, err, tol, capacity=None, stream=None):
    """vqhip_vec3_residual_encode_device -> (code [n], offsets [n+1], the whole payload buffer of n * 6144 bytes, filled with FILL before)."""
    n = len(x)
    dx, dr = torch.from_numpy(np.ascontiguousarray(x, F)).cuda(), torch.from_numpy(np.ascontiguousarray(recon, F)).cuda()
    de = torch.from_numpy(np.ascontiguousarray(err, F)).cuda()
    dc = torch.full((n,), 0x7777, dtype=torch.int16, device="cuda")
    do = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    dp = torch.full((n * RAW_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    codec.residual_encode_device(dx.data_ptr(), dr.data_ptr(), de.data_ptr(), n, tol, dc.data_ptr(), do.data_ptr(), dp.data_ptr(),
                                 n * RAW_BYTES if capacity is None else capacity, stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return dc.cpu().numpy().view(np.uint16), do.cpu().numpy(), dp.cpu().numpy()


def dev_apply(codec, recon, tol, code, off, payload, stream=None):
    n = len(recon)
    dr = torch.from_numpy(np.ascontiguousarray(recon, F)).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(code, np.uint16).view(np.int16)).cuda()
    do = torch.from_numpy(np.ascontiguousarray(off, np.int64)).cuda()
    dp = torch.from_numpy(np.frombuffer(bytes(payload) + bytes(8), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    codec.residual_apply_device(dr.data_ptr(), n, tol, dc.data_ptr(), do.data_ptr(), dp.data_ptr(), stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return dr.cpu().numpy()


def check_against_restatement(codec, x, recon, err, tol, stream=None):
    code, off, buf = dev_encode(codec, x, recon, err, tol, stream=stream)
    rcode, roff = t3r.classify(x, recon, err, tol)
    bad = np.flatnonzero(code != rcode)
    assert len(bad) == 0, (tol, bad[:8], code[bad][:8], rcode[bad][:8])
    assert np.array_equal(off, roff), tol
    total = int(off[-1])
    want = np.frombuffer(t3r.pack(x, recon, tol, rcode), dtype=np.uint8)
    assert len(want) == total
    assert np.array_equal(buf[:total], want), tol
    assert (buf[total:] == FILL).all(), "bytes written beyond the total"
    return code, off, buf, want


def test_encode_device_equals_the_restatement_at_five_tolerances(codec, leaves):
    _, err, rec = dev_roundtrip(codec, leaves)
    e = err[:, 0]
    assert np.isfinite(e).all()
    med = float(np.median(e))
    second = torch.cuda.Stream()
    for tol in (float(e.min()), float(np.quantile(e, 0.25, method="lower")), med, float(e.max()), float("inf")):
        code, off, buf, want = check_against_restatement(codec, leaves, rec, err, tol)
        for n in SIZES:                                              # the same bits at every batch size, place and stream
            for lo, stream in ((0, None), (N - n, second)):
                c2, o2, b2 = dev_encode(codec, leaves[lo:lo + n], rec[lo:lo + n], err[lo:lo + n], tol, stream=stream)
                assert np.array_equal(c2, code[lo:lo + n]) and np.array_equal(o2, off[lo:lo + n + 1] - off[lo]), (tol, n, lo)
                assert np.array_equal(b2[:o2[-1]], buf[off[lo]:off[lo + n]]) and (b2[o2[-1]:] == FILL).all(), (tol, n, lo)
        sel = code != t3r.KEPT
        quant = sel & (code != t3r.RAW)
        b = t3r.widths(code[quant])
        print(f"{codec.precision} tol {tol:.6g}: {sel.sum()} selected, {(code == t3r.RAW).sum()} raw, payload {off[-1]} B against "
              f"{sel.sum()} x 6144 = {sel.sum() * RAW_BYTES} B, one shared width {int(3 * 64 * b.max(axis=1).sum()) if len(b) else 0} B")
        if tol == med:
            assert 0 < sel.sum() <= 68 and quant.sum() > 0
        if tol == float("inf") or tol == float(e.max()):
            assert (code == t3r.KEPT).all() and off[-1] == 0


TOL_S = 0.5   # a float32 value; step 0.9375, so x = q * step and x^ + q * step are exact for the format leaves


def model_free_leaves():
    """(x, x^, err) for tol = TOL_S, no model: the 51 format leaves of the CPU test (every width 0 .. 16 in every channel), a leaf
    of 16/16/16 (3072 bytes), a leaf with one 17-bit channel (raw), a NaN leaf and an inf leaf (raw at every tolerance), and after
    every third of them and at the end a kept leaf (reported error 0.25).  74 leaves: no multiple of the 4 leaves of a workgroup."""
    x, recon, err, _ = t3r.format_leaves(TOL_S)
    wide = t3r.leaf_with_max_q([32767, 32767, 32767], TOL_S, np.random.default_rng(70), negative=[False, True, False])[0]
    over = t3r.leaf_with_max_q([3, 32768, 3], TOL_S, np.random.default_rng(71))[0]
    nan_leaf, inf_leaf = x[20].copy(), x[21].copy()
    nan_leaf.view(np.uint32)[300, 1] = 0x7FC12345
    inf_leaf[17, 2] = -np.inf
    x = np.concatenate([x, wide[None], over[None], nan_leaf[None], inf_leaf[None]])
    recon = np.zeros_like(x)
    err = np.concatenate([err, [[9.0, 9.0], [9.0, 9.0], [np.nan, np.nan], [np.nan, np.inf]]]).astype(F)
    xs, rs, es = [], [], []
    rng = np.random.default_rng(72)
    for i in range(len(x)):
        xs.append(x[i]), rs.append(recon[i]), es.append(err[i])
        if i % 3 == 2 or i == len(x) - 1:
            r = rng.standard_normal((512, 3)).astype(F)
            xs.append(r + F(0.25)), rs.append(r), es.append(np.array([0.25, 1.0], F))
    return np.ascontiguousarray(np.stack(xs)), np.ascontiguousarray(np.stack(rs)), np.stack(es)


def test_model_free_call_with_every_width_in_every_channel(codec):
    x, recon, err = model_free_leaves()
    n = len(x)
    assert n == 74 and n % 4 != 0
    code, off, buf, want = check_against_restatement(codec, x, recon, err, TOL_S)
    kept = code == t3r.KEPT
    assert kept.sum() == 19 and (code == t3r.RAW).sum() == 3 and (code == t3r.make_code(16, 16, 16)).sum() == 1
    b = t3r.widths(code[~kept & (code != t3r.RAW)])
    for ch in range(3):
        assert set(b[:, ch].tolist()) == set(range(17)), ch
    nan_at = int(np.flatnonzero(np.isnan(x).any(axis=(1, 2)))[0])
    assert code[nan_at] == t3r.RAW and same(buf[off[nan_at]:off[nan_at + 1]], x[nan_at].view(np.uint8).reshape(-1))   # the NaN payload as it went in
    out = dev_apply(codec, recon, TOL_S, code, off, buf[:off[-1]])
    assert same(out, t3r.apply(recon, TOL_S, code, want.tobytes()))
    sel = ~kept
    assert same(out[sel], x[sel]) and same(out[kept], recon[kept])     # exact products and raw copies: lossless here
    # capacity one byte short: the last non-empty record is not written at all, everything before it is identical
    last = int(np.flatnonzero(t3r.record_size(code) > 0)[-1])
    c2, o2, b2 = dev_encode(codec, x, recon, err, TOL_S, capacity=int(off[-1]) - 1)
    assert np.array_equal(c2, code) and np.array_equal(o2, off)
    assert np.array_equal(b2[:off[last]], buf[:off[last]]) and (b2[off[last]:] == FILL).all()
    c3, o3, b3 = dev_encode(codec, x, recon, err, TOL_S, capacity=0)
    assert np.array_equal(c3, code) and np.array_equal(o3, off) and (b3 == FILL).all()
    # tol 0 and NaN: every leaf raw, the payload is the input; a negative tol too
    for tol in (0.0, float("nan"), -1.0):
        c4, o4, b4, _ = check_against_restatement(codec, x[:9], recon[:9], err[:9], tol)
        assert (c4 == t3r.RAW).all() and same(b4[:o4[-1]], x[:9].view(np.uint8).reshape(-1))


def test_apply_device_equals_the_restatement(codec, leaves):
    idx, err, rec = dev_roundtrip(codec, leaves)
    tol = float(np.median(err[:, 0]))
    code, off = t3r.classify(leaves, rec, err, tol)
    payload = t3r.pack(leaves, rec, tol, code)
    want = t3r.apply(rec, tol, code, payload)
    plain = dev_decode(codec, idx)
    assert same(plain, rec)
    for stream in (None, torch.cuda.Stream()):
        out = dev_apply(codec, plain, tol, code, off, payload, stream)
        assert same(out, want)
    kept = code == t3r.KEPT
    assert 68 <= kept.sum() < N and same(out[kept], plain[kept]) and not same(out[~kept], plain[~kept])
    bad = leaves.copy()                                              # every leaf raw: bit-exact copies, NaN payloads included
    bad.view(np.uint32)[5, 300, 1] = 0x7FC12345
    bad.view(np.uint32)[77, 0, 0] = 0xFFC00001
    raw = np.full(N, t3r.RAW, np.uint16)
    out = dev_apply(codec, rec, tol, raw, np.arange(N + 1, dtype=np.int64) * RAW_BYTES, bad.tobytes())
    assert same(out, bad)
    for n in SIZES[:4]:
        assert same(dev_apply(codec, rec[N - n:], tol, code[N - n:], off[N - n:] - off[N - n], payload[off[N - n]:]), want[N - n:]), n


def test_the_host_pair_keeps_every_leaf_within_the_tolerance(codec, pack, leaves):
    mode = codec.precision
    _, err = codec.roundtrip(leaves)
    tol = float(np.median(err[:, 0]))
    idx, code, payload = codec.compress_residual(leaves, tol)
    out = codec.decompress_residual(idx, tol, code, payload)
    worst = np.abs(leaves - out).reshape(N, -1).max(axis=1)
    sel = code != t3r.KEPT
    print(f"{mode} tol {tol:.4f}: {sel.sum()} of {N} leaves selected, {(code == t3r.RAW).sum()} raw, {len(payload)} payload bytes, "
          f"largest error {worst.max():.4f}")
    assert np.isfinite(leaves).all() and (worst <= F(tol)).all()
    assert np.array_equal(idx, codec.encode(leaves))
    plain = codec.decode(idx)
    assert same(out[~sel], plain[~sel]) and not same(out[sel], plain[sel])
    didx, derr, drec = dev_roundtrip(codec, leaves)
    dcode, doff, dbuf = dev_encode(codec, leaves, drec, derr, tol)
    assert np.array_equal(idx, didx) and np.array_equal(code, dcode) and same(payload, dbuf[:doff[-1]])
    assert len(payload) == HipVec3Codec.residual_record_sizes(code).sum()
    assert same(out, t3r.apply(drec, tol, dcode, payload.tobytes()))
    i2, c2, p2, e2 = codec.compress_residual(leaves[:33], tol, return_leaf_err=True)
    assert same(e2, err[:33]) and np.array_equal(c2, code[:33]) and same(p2, payload[:doff[33]])
    assert same(codec.decompress_residual(i2, tol, c2, p2), out[:33])
    small = HipVec3Codec(pack, precision=mode)                       # chunks of 32, 32, 32, 32, 8: records concatenated over the call
    try:
        small.set_chunk_leaves(32)
        si, sc, sp = small.compress_residual(leaves, tol)
        assert np.array_equal(si, idx) and np.array_equal(sc, code) and same(sp, payload)
        assert same(small.decompress_residual(si, tol, sc, sp), out)
    finally:
        small.close()
    # non-finite leaves come back bit for bit and touch no other leaf
    bad = leaves.copy()
    bad.view(np.uint32)[5, 300, 1] = 0x7FC12345
    bad[N - 2, 17, 2] = np.inf
    bi, bc, bp = codec.compress_residual(bad, tol)
    ok = np.setdiff1d(np.arange(N), [5, N - 2])
    assert bc[5] == t3r.RAW and bc[N - 2] == t3r.RAW and np.array_equal(bc[ok], code[ok])
    bout = codec.decompress_residual(bi, tol, bc, bp)
    assert same(bout[[5, N - 2]], bad[[5, N - 2]]) and same(bout[ok], out[ok])
    ic, icode, ip = codec.compress_residual(bad, float("inf"))
    assert np.array_equal(np.flatnonzero(icode != t3r.KEPT), [5, N - 2]) and len(ip) == 2 * RAW_BYTES
    # a wrong code or payload length is refused before any GPU work, the outputs stay untouched and the handle stays usable
    lib, h = codec._lib, codec._h
    msg = lambda: lib.vqhip_vec3_last_error(h).decode()   # noqa: E731
    p = lambda a: a.ctypes.data   # noqa: E731
    o4 = np.zeros((N, 512, 3), F)
    for wrong_code, text in ((17, "code 0x0011 of leaf 3"), (17 << 5, "code 0x0220 of leaf 3"), (0x8003, "code 0x8003 of leaf 3"), (0xFFFD, "code 0xFFFD of leaf 3")):
        wrong = code.copy()
        wrong[3] = wrong_code
        assert lib.vqhip_vec3_residual_decompress(h, p(idx), N, tol, p(wrong), p(payload), len(payload), p(o4)) == -1
        assert text in msg() and not o4.any()
        with pytest.raises(ValueError, match="leaf codes must be"):
            codec.decompress_residual(idx, tol, wrong, payload)
    assert lib.vqhip_vec3_residual_decompress(h, p(idx), N, tol, p(code), p(payload), len(payload) - 64, p(o4)) == -1
    assert "payload bytes" in msg() and not o4.any()
    assert lib.vqhip_vec3_residual_decompress(h, p(idx), N, tol, p(code), None, len(payload), p(o4)) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_residual_decompress(h, None, 0, tol, None, None, 0, None) == 0
    nb = np.full(1, -5, np.int64)
    assert lib.vqhip_vec3_residual_compress(h, None, 0, tol, None, None, None, None, p(nb)) == 0 and nb[0] == 0
    c5, i5 = np.full(N, 0x7777, np.uint16), np.full((N, 64), 0x7777, np.uint16)
    assert lib.vqhip_vec3_residual_compress(h, p(leaves), N, tol, None, None, p(c5), p(o4), p(nb)) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_residual_compress(h, p(leaves), N, tol, p(i5), None, p(c5), p(o4), None) == -1 and "payload_bytes is NULL" in msg()
    assert lib.vqhip_vec3_residual_compress(h, p(leaves), -1, tol, p(i5), None, p(c5), p(o4), p(nb)) == -1 and "n_leaves < 0" in msg()
    assert (c5 == 0x7777).all() and (i5 == 0x7777).all() and not o4.any()
    assert lib.vqhip_vec3_residual_encode_device(h, None, None, None, 0, tol, None, None, None, 0, None) == 0
    assert lib.vqhip_vec3_residual_encode_device(h, None, None, None, 4, tol, None, None, None, 0, None) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_residual_apply_device(h, None, 0, tol, None, None, None, None) == 0
    assert lib.vqhip_vec3_residual_apply_device(h, None, 4, tol, None, None, None, None) == -1 and "null pointer" in msg()
    assert lib.vqhip_vec3_residual_compress(h, p(leaves), N, tol, p(i5), None, p(c5), p(o4), p(nb)) == 0   # leaf_err may be NULL
    assert np.array_equal(i5, idx) and np.array_equal(c5, code) and nb[0] == len(payload)
    assert same(codec.decompress_residual(idx, tol, code, payload), out)


def test_the_new_calls_move_nothing_of_their_neighbours(codec, leaves):
    x = np.ascontiguousarray(leaves[:100])

    def neighbours():
        idx = codec.encode(x)
        ridx, rerr, rrec = codec.roundtrip(x, return_recon=True)
        return [idx, codec.decode(idx), ridx, rerr, rrec, *codec.compress_bounded(x, 0.1, return_leaf_err=True)]

    before = neighbours()
    tol = float(np.median(before[3][:, 0]))
    idx, code, payload = codec.compress_residual(leaves, tol)
    codec.decompress_residual(idx, tol, code, payload)
    _, derr, drec = dev_roundtrip(codec, leaves)
    dcode, doff, dbuf = dev_encode(codec, leaves, drec, derr, tol, stream=torch.cuda.Stream())
    dev_apply(codec, drec, tol, dcode, doff, dbuf[:doff[-1]])
    after = neighbours()
    assert len(before) == len(after) == 9
    for k, (a, b) in enumerate(zip(before, after)):
        assert same(a, b), k
