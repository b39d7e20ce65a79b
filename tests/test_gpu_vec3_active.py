"""Compact residual records of the Vec3 handle on the GPU (include/vqvdb_hip_vec3_active.h): encode, apply and
sweep against tests/torch_ref_active.py to the bit and against the masked calls (same codes; the existing apply on the masked
records gives the same active values), the host pair and sweep on a batch cut into chunks in both precision modes, and the
refusals.  The leaves, x^, masks and tolerances are those of tests/test_gpu_vec3_masked.py, with one more mask whose active counts
sit around the word boundaries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import masked_gpu_common as mg  # noqa: E402
import torch_ref_active as tra  # noqa: E402
import torch_ref_masked as trm  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import synth_vec3, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec, pack_masks  # noqa: E402

pytestmark = pytest.mark.gpu

C = 3
N0 = 136
F = np.float32
FILL = mg.FILL
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 511, 512)
VARIANTS = ("ones", "zeros", "half", "sparse", "nonzero", "one_word", "designed", "count_edges")
BACKGROUND = np.array([-0.0, np.nan, 1e30], F)


@pytest.fixture(scope="module")
def pack():
    return weightpack.dumps(synth_vec3.make_weights(0))


@pytest.fixture(scope="module")
def codec(pack):
    c = HipVec3Codec(pack)
    yield c
    c.close()


def dev_roundtrip(codec, x):
    n = len(x)
    dx = mg.to_dev(x, F)
    di = torch.zeros((n, 64), dtype=torch.int16, device="cuda")
    dr = torch.zeros((n, 512, 3), dtype=torch.float32, device="cuda")
    de = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.roundtrip_device(dx.data_ptr(), n, de.data_ptr(), di.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    return di.cpu().numpy().view(np.uint16), de.cpu().numpy(), dr.cpu().numpy()


def count_edges(n):
    """bool [n,512]: leaf i has COUNTS[i % 10] active voxels at random positions"""
    rng = np.random.default_rng(31)
    active = np.zeros((n, 512), bool)
    for i in range(n):
        active[i, rng.permutation(512)[:COUNTS[i % len(COUNTS)]]] = True
    return active


@pytest.fixture(scope="module")
def base(codec):
    """(x [145,512,3], x^ from one roundtrip_device call with the designed input's own x^ behind it, the mask variants, the
    tolerances), computed once and left unchanged"""
    leaves = np.ascontiguousarray(np.concatenate([synth_vec3.make_leaves(128, 4321), synth_vec3.edge_leaves()]))
    assert len(leaves) == N0
    _, uerr, rec = dev_roundtrip(codec, leaves)
    dx, dr, dact, _ = trm.designed(C)
    x, recon = np.ascontiguousarray(np.concatenate([leaves, dx])), np.ascontiguousarray(np.concatenate([rec, dr]))
    variants = mg.mask_variants(x, C, dact)
    variants["count_edges"] = count_edges(len(x))
    for a in (x, recon, *variants.values()):
        a.setflags(write=False)
    return x, recon, variants, mg.tolerances(uerr) + [trm.TOL_D]


class Resident:
    """leaves, x^, masks and masked errors on the device; the compact encode and sweep on slices of them"""

    def __init__(self, codec, x, recon, masks, err):
        self.codec, self.n = codec, len(x)
        self.x, self.r, self.m, self.e = mg.to_dev(x, F), mg.to_dev(recon, F), mg.to_dev(masks), mg.to_dev(err, F)

    def encode(self, tol, lo=0, n=None, capacity=None, stream=None):
        """-> (code [n], offsets [n+1], the whole payload buffer of n * 6144 bytes, filled with FILL before)"""
        n = self.n - lo if n is None else n
        dc = torch.full((n,), 77, dtype=torch.int16, device="cuda")
        do = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        dp = torch.full((n * 6144,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.codec.active_encode_device(self.x[lo:].data_ptr(), self.r[lo:].data_ptr(), self.m[lo:].data_ptr(), self.e[lo:].data_ptr(), n, tol,
                                        dc.data_ptr(), do.data_ptr(), dp.data_ptr(), n * 6144 if capacity is None else capacity, mg.stream_of(stream))
        torch.cuda.synchronize()
        return dc.cpu().numpy().view(np.uint16), do.cpu().numpy(), dp.cpu().numpy()

    def sweep(self, tols, lo=0, n=None, sums=None, stream=None, rows=None):
        """through the library's own entry point (the wrapper refuses the negative rungs that the C call takes)"""
        n = self.n - lo if n is None else n
        t = np.asarray(tols, F)
        if sums is None:
            sums = torch.zeros(len(t) if rows is None else rows, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = self.codec._lib.vqhip_vec3_active_sweep_device(self.codec._h, self.x[lo:].data_ptr(), self.r[lo:].data_ptr(), self.m[lo:].data_ptr(),
                                                            self.e[lo:].data_ptr(), n, t.ctypes.data, len(t), sums.data_ptr(),
                                                            mg.stream_of(stream) or None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return sums


def dev_apply(codec, recon, masks, tol, code, off, payload, background=None):
    dr, dm, dc, do = mg.to_dev(recon, F), mg.to_dev(masks), mg.to_dev(code), mg.to_dev(off, np.int64)
    dp = mg.to_dev(np.frombuffer(bytes(payload) + bytes(8), dtype=np.uint8).copy())
    torch.cuda.synchronize()
    codec.active_apply_device(dr.data_ptr(), dm.data_ptr(), len(recon), tol, dc.data_ptr(), do.data_ptr(), dp.data_ptr(), background)
    torch.cuda.synchronize()
    return dr.cpu().numpy()


def check_encode(codec, dev, x, recon, active, masks, err, tols):
    """-> {tol: (code, offsets, payload)}; codes == the masked encode's, offsets and payload == the restatement, nothing written
    beyond the total or beyond a short capacity, the same bits for slices from the front and (on a second stream) from the back"""
    n = len(x)
    second = torch.cuda.Stream()
    out = {}
    for tol in tols:
        code, off, buf = dev.encode(tol)
        mcode, moff, mbuf = mg.dev_encode(codec, C, x, recon, masks, err, tol)
        rcode, _ = trm.classify(x, recon, err, tol, active, C)
        assert np.array_equal(code, mcode) and np.array_equal(code, rcode), (tol, np.flatnonzero(code != mcode)[:8])
        roff = tra.offsets(rcode, active)
        assert np.array_equal(off, roff), tol
        assert (np.diff(off) <= np.diff(moff)).all() and (np.diff(off) % 8 == 0).all(), tol
        total = int(off[-1])
        want = np.frombuffer(tra.pack(x, recon, tol, rcode, active), dtype=np.uint8)
        assert len(want) == total, tol
        bad = np.flatnonzero(buf[:total] != want)
        assert len(bad) == 0, (tol, bad[:8], np.searchsorted(off, bad[:8], side="right") - 1)
        assert (buf[total:] == FILL).all(), "bytes written beyond the total"
        if active.all():
            assert np.array_equal(buf[:total], mbuf[:total]) and total == moff[-1]                 # all active: the masked bytes
        for m in mg.SIZES:
            for lo, stream in ((0, None), (n - m, second)):
                c2, o2, b2 = dev.encode(tol, lo, m, stream=stream)
                assert np.array_equal(c2, code[lo:lo + m]) and np.array_equal(o2, off[lo:lo + m + 1] - off[lo]), (tol, m, lo)
                assert np.array_equal(b2[:o2[-1]], buf[off[lo]:off[lo + m]]) and (b2[o2[-1]:] == FILL).all(), (tol, m, lo)
        sized = np.flatnonzero(np.diff(off) > 0)
        if len(sized):
            last = int(sized[-1])                                      # the last record that has bytes: one byte short of it
            c3, o3, b3 = dev.encode(tol, capacity=int(off[last + 1]) - 1)
            assert np.array_equal(c3, code) and np.array_equal(o3, off)
            assert np.array_equal(b3[:off[last]], buf[:off[last]]) and (b3[off[last]:] == FILL).all(), tol
        out[tol] = (code, off, buf[:total].copy(), moff, mbuf[:moff[-1]].copy())
    return out


def check_apply(codec, x, recon, active, masks, tol, code, off, payload, moff, mpayload):
    act3 = trm._active(active, C)
    planted = recon.copy()
    for i in range(len(x)):                                            # a NaN in x^ at the first inactive voxel of every leaf that has one
        gone = np.flatnonzero(~active[i])
        if len(gone):
            planted[i, gone[0], :] = np.nan
    out = dev_apply(codec, planted, masks, tol, code, off, payload)
    assert mg.same(out, tra.apply(planted, tol, code, payload.tobytes(), active)), tol
    assert out[~act3].tobytes() == planted[~act3].tobytes()            # inactive voxels keep their bits, the planted NaN included
    existing = mg.dev_apply(codec, C, recon, tol, code, moff, mpayload)               # the existing apply call on the masked records
    assert out[act3].tobytes() == existing[act3].tobytes(), tol
    filled = dev_apply(codec, planted, masks, tol, code, off, payload, BACKGROUND)
    assert mg.same(filled, tra.apply(planted, tol, code, payload.tobytes(), active, BACKGROUND)), tol
    assert filled[act3].tobytes() == out[act3].tobytes()
    assert filled[~active].tobytes() == np.tile(BACKGROUND, (int((~active).sum()), 1)).tobytes(), tol
    quant = (code != t3r.KEPT) & (code != t3r.RAW)
    with np.errstate(invalid="ignore"):
        assert (np.abs(x - out)[quant][act3[quant]] <= F(tol)).all(), tol                           # the bound, the decoder's own arithmetic
    raw = code == t3r.RAW
    assert out[raw][act3[raw]].tobytes() == x[raw][act3[raw]].tobytes()


def check_sweep(dev, x, recon, active, err, enc, tols):
    n = len(x)
    base = list(tols[:7])
    got = dev.sweep(base).cpu().numpy()
    assert np.array_equal(got, tra.sweep_bytes(x, recon, err, base, active)), got
    assert np.array_equal(got, [enc[t][1][-1] for t in base])
    one = dev.sweep(base[2:3], rows=64).cpu().numpy()
    assert one[0] == got[2] and not one[1:].any()
    extra = [-1.0, -0.0, float("-inf")]                                # negative rungs and -0 through the C call
    sixteen = (base + extra + [base[2] / 2, base[2] * 2, base[2] / 8, base[2] * 8, base[1] * 3, base[3] / 3])[:16]
    med = base[2] if base[2] > 0 else 1e-3
    many = [float(v) for v in np.geomspace(med / 64, med * 64, 64 - len(sixteen)).astype(F)] + sixteen
    assert len(sixteen) == 16 and len(many) == 64
    for rungs in (sixteen, many):
        got = dev.sweep(rungs).cpu().numpy()
        assert np.array_equal(got, tra.sweep_bytes(x, recon, err, rungs, active))
        assert np.array_equal(got, [dev.encode(float(F(t)))[1][-1] for t in rungs])               # offsets[n] of the encode at that rung
    both = dev.sweep(base, 0, n // 2)                                  # two calls on the two halves add up to the one call
    both = dev.sweep(base, n // 2, n - n // 2, sums=both, stream=torch.cuda.Stream()).cpu().numpy()
    assert np.array_equal(both, dev.sweep(base).cpu().numpy())


@pytest.mark.parametrize("name", VARIANTS)
def test_compact_encode_apply_and_sweep_equal_the_restatement(codec, base, name):
    x, recon, variants, tols = base
    active = variants[name]
    masks = trm.pack_masks(active)
    err = trm.leaf_err_fixed(x, recon, active, C)
    dev = Resident(codec, x, recon, masks, err)
    enc = check_encode(codec, dev, x, recon, active, masks, err, tols)
    for tol in (tols[2], trm.TOL_D):
        check_apply(codec, x, recon, active, masks, tol, *enc[tol])
    check_sweep(dev, x, recon, active, err, enc, tols)
    if name == "designed":
        code, off = enc[trm.TOL_D][:2]
        raw_off = enc[tols[6]][1]                                      # the NaN rung: every selected leaf with a voxel is raw
        for kind in ("single_0", "single_63", "single_64", "single_511"):
            i = N0 + trm.KINDS.index(kind)
            assert off[i + 1] - off[i] == 8 * t3r.widths(int(code[i])).sum() == 136 and raw_off[i + 1] - raw_off[i] == 16, kind
    if name == "count_edges":
        A = active.sum(axis=1)
        raw = enc[tols[6]][0] == t3r.RAW
        assert set(A[raw]) == set(COUNTS) - {0} and (np.diff(enc[tols[6]][1]) == 8 * ((3 * A + 1) // 2)).all()


def test_compact_sweep_of_4099_leaves(codec):
    """4 099 leaves with synthetic x^ (the designed input, tiled; the model is not run): the stride loop above 4 096 leaves runs"""
    x, recon, active, _ = trm.designed(C)
    n = 4099
    pick = np.arange(n) % len(x)
    err = trm.leaf_err_fixed(x, recon, active, C)
    tols = [trm.TOL_D, trm.TOL_D / 4, 0.0, float("nan"), float("inf"), 4 * trm.TOL_D, -1.0]
    weight = np.bincount(pick, minlength=len(x))
    A = active.sum(axis=1)
    want = np.array([(tra.record_size(trm.classify(x, recon, err, tol, active, C)[0], A) * weight).sum() for tol in tols], np.int64)
    dev = Resident(codec, x[pick], recon[pick], trm.pack_masks(active[pick]), err[pick])
    got = dev.sweep(tols).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    assert got[0] > 0 and got[3] > got[0]


@pytest.mark.parametrize("mode", ("fp32", "bf16"))
def test_host_pair_and_sweep_give_the_device_results_in_chunks_of_32(pack, base, mode):
    x, _, variants, tols = base
    codec = HipVec3Codec(pack, precision=mode)
    try:
        active = variants["designed"].copy()
        active[:N0] = variants["half"][:N0]
        masks = pack_masks(active)
        idx, _, rec = dev_roundtrip(codec, x)                          # the mode's x^ of all 145 leaves, designed ones included
        err = mg.dev_err(codec, x, rec, masks)
        tol = tols[2]
        dev = Resident(codec, x, rec, masks, err)
        code, off, buf = dev.encode(tol)
        codec.set_chunk_leaves(32)
        hi, hc, hp, he = codec.compress_active(x, masks, tol, return_leaf_err=True)
        assert np.array_equal(hi, idx) and mg.same(he, err) and np.array_equal(hc, code) and np.array_equal(hp, buf[:off[-1]])
        assert np.array_equal(hp, np.frombuffer(tra.pack(x, rec, tol, code, active), dtype=np.uint8))
        sums = codec.rate_sweep_active(x, masks, tols[:7])
        assert np.array_equal(sums, dev.sweep(tols[:7]).cpu().numpy()) and np.array_equal(sums, tra.sweep_bytes(x, rec, err, tols[:7], active))
        assert sums[2] == len(hp)
        out = codec.decompress_active(hi, masks, tol, hc, hp)
        assert mg.same(out, tra.apply(rec, tol, hc, hp.tobytes(), active))
        filled = codec.decompress_active(hi, masks, tol, hc, hp, background=BACKGROUND)
        assert mg.same(filled, tra.apply(rec, tol, hc, hp.tobytes(), active, BACKGROUND))
        quant = (hc != t3r.KEPT) & (hc != t3r.RAW)
        act3 = trm._active(active, C)
        with np.errstate(invalid="ignore"):
            assert (np.abs(x - out)[quant][act3[quant]] <= F(tol)).all()
        mi, mc, mp = codec.compress_residual_masked(x, masks, tol)
        assert np.array_equal(mi, hi) and np.array_equal(mc, hc) and len(hp) < len(mp)               # what the feature is for
    finally:
        codec.close()


def test_refusals(codec, base):
    x, recon, variants, tols = base
    lib, h, last = codec._lib, codec._h, codec._lib.vqhip_vec3_last_error
    active = variants["half"]
    n = len(x)
    masks = trm.pack_masks(active)
    err = trm.leaf_err_fixed(x, recon, active, C)
    dev = Resident(codec, x, recon, masks, err)
    dc, do = torch.zeros(n, dtype=torch.int16, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    dp = torch.zeros(n * 6144, dtype=torch.uint8, device="cuda")
    sums = torch.zeros(64, dtype=torch.int64, device="cuda")
    t1 = np.array([0.5], F)
    p = lambda t: t.data_ptr()                                         # noqa: E731
    assert lib.vqhip_vec3_active_encode_device(h, p(dev.x), p(dev.r), None, p(dev.e), n, 0.5, p(dc), p(do), p(dp), n * 6144, None) == -1
    assert "null pointer" in last(h).decode()
    assert lib.vqhip_vec3_active_apply_device(h, p(dev.r), None, n, 0.5, p(dc), p(do), p(dp), None, None) == -1 and "null pointer" in last(h).decode()
    assert lib.vqhip_vec3_active_sweep_device(h, p(dev.x), p(dev.r), None, p(dev.e), n, t1.ctypes.data, 1, p(sums), None) == -1
    assert "null pointer" in last(h).decode()
    for bad in (0, 65, -1):
        assert lib.vqhip_vec3_active_sweep_device(h, p(dev.x), p(dev.r), p(dev.m), p(dev.e), n, t1.ctypes.data, bad, p(sums), None) == -1
        assert "n_tols" in last(h).decode()
        assert lib.vqhip_vec3_active_sweep(h, x.ctypes.data, masks.ctypes.data, n, t1.ctypes.data, bad, np.zeros(64, np.int64).ctypes.data) == -1
    # n == 0 returns OK and touches nothing, whatever the pointers
    assert lib.vqhip_vec3_active_encode_device(h, None, None, None, None, 0, 0.5, None, None, None, 0, None) == 0
    assert lib.vqhip_vec3_active_apply_device(h, None, None, 0, 0.5, None, None, None, None, None) == 0
    assert lib.vqhip_vec3_active_sweep_device(h, None, None, None, None, 0, t1.ctypes.data, 1, None, None) == 0
    nbytes = ctypes.c_int64(-1)
    assert lib.vqhip_vec3_active_compress(h, None, None, 0, 0.5, None, None, None, None, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert lib.vqhip_vec3_active_decompress(h, None, None, 0, 0.5, None, None, 0, None, None) == 0
    hh = np.full(1, -1, np.int64)
    assert lib.vqhip_vec3_active_sweep(h, None, None, 0, t1.ctypes.data, 1, hh.ctypes.data) == 0 and hh[0] == 0
    assert lib.vqhip_vec3_active_compress(h, x.ctypes.data, None, n, 0.5, None, None, None, None, ctypes.byref(nbytes)) == -1
    assert lib.vqhip_vec3_active_sweep(h, x.ctypes.data, None, n, t1.ctypes.data, 1, hh.ctypes.data) == -1 and "null pointer" in last(h).decode()
    torch.cuda.synchronize()
    assert not sums.any().item() and not dc.any().item() and not do.any().item() and not dp.any().item()
    # decompress: a bad code or a payload size off by 8 is refused before any GPU work and leaves `leaves` untouched
    tol = tols[2]
    hi, hc, hp = codec.compress_active(x, masks, tol)
    assert len(hp) > 8
    out = np.full((n, 512, 3), 7.0, F)
    call = lambda lc, pl, nb: lib.vqhip_vec3_active_decompress(h, hi.ctypes.data, masks.ctypes.data, n, tol, lc.ctypes.data, pl.ctypes.data, nb, None,  # noqa: E731
                                                               out.ctypes.data)
    wrong = hc.copy()
    wrong[5] = t3r.make_code(17, 0, 0)
    assert call(wrong, hp, len(hp)) == -1 and "0x0011" in last(h).decode() and (out == 7.0).all()
    assert call(hc, hp, len(hp) - 8) == -1 and "payload bytes" in last(h).decode() and (out == 7.0).all()
    longer = np.concatenate([hp, np.zeros(8, np.uint8)])
    assert call(hc, longer, len(hp) + 8) == -1 and (out == 7.0).all()
    assert call(hc, hp, len(hp)) == 0 and mg.same(out, codec.decompress_active(hi, masks, tol, hc, hp))   # the handle is still usable
