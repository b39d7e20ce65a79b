"""Active-voxel masks of the Vec3 handle on the GPU (include/vqvdb_hip_vec3_mask.h): the masked error, encode and
sweep against tests/torch_ref_masked.py (C = 3) to the bit, the EXISTING apply and decompress calls on masked records, the host pair
and sweep on a batch cut into chunks in both precision modes, and the refusals.  The leaves are the 136 of
tests/test_gpu_vec3_residual.py and the designed input of tests/torch_ref_masked.py (whose x^ is its own: the device calls take x^
as an argument; the host calls run the model on all 145)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import masked_gpu_common as mg  # noqa: E402
import torch_ref_masked as trm  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import synth_vec3, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec, pack_masks  # noqa: E402

pytestmark = pytest.mark.gpu

C = 3
N0 = 136
F = np.float32
VARIANTS = ("ones", "zeros", "half", "sparse", "nonzero", "one_word", "designed")


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


@pytest.fixture(scope="module")
def base(codec):
    """(x [145,512,3], x^ for the device calls, roundtrip_device's own errors of the 136, the mask variants, the tolerances), computed
    once and left unchanged"""
    leaves = np.ascontiguousarray(np.concatenate([synth_vec3.make_leaves(128, 4321), synth_vec3.edge_leaves()]))
    assert len(leaves) == N0
    _, uerr, rec = dev_roundtrip(codec, leaves)
    dx, dr, dact, _ = trm.designed(C)
    x, recon = np.ascontiguousarray(np.concatenate([leaves, dx])), np.ascontiguousarray(np.concatenate([rec, dr]))
    variants = mg.mask_variants(x, C, dact)
    for a in (x, recon, uerr, *variants.values()):
        a.setflags(write=False)
    return x, recon, uerr, variants, mg.tolerances(uerr)


@pytest.mark.parametrize("name", VARIANTS)
def test_masked_error_equals_the_restatement_bit_for_bit(codec, base, name):
    x, recon, uerr, variants, _ = base
    got = mg.case_error(codec, C, x, recon, variants[name], None)
    if name == "ones":                                                 # an all-ones mask: roundtrip_device's own error bits
        assert mg.same(got[:N0], uerr)


@pytest.mark.parametrize("name", VARIANTS)
def test_masked_encode_apply_and_sweep_equal_the_restatement(codec, base, name):
    x, recon, uerr, variants, tols = base
    active = variants[name]
    err, enc = mg.case_encode(codec, C, x, recon, active, tols + [trm.TOL_D])
    for tol in (tols[2], trm.TOL_D):
        code, off, payload = enc[tol]
        mg.case_apply(codec, C, x, recon, active, err, tol, code, off, payload)
    mg.case_sweep(codec, C, x, recon, active, err, enc, tols)
    ucode = t3r.classify(x, recon, trm.leaf_err_fixed(x, recon, np.ones_like(active), C), trm.TOL_D)[0]
    code = enc[trm.TOL_D][0]
    assert (t3r.record_size(code) <= t3r.record_size(ucode)).all() and (code[ucode == t3r.KEPT] == t3r.KEPT).all()
    if name == "designed":
        k = {kind: N0 + i for i, kind in enumerate(trm.KINDS)}
        assert code[k["kept_by_mask"]] == t3r.KEPT != ucode[k["kept_by_mask"]]                  # what the feature is for
        assert ucode[k["raw_to_quantised"]] == t3r.RAW and code[k["raw_to_quantised"]] < 0x8000
        assert code[k["raw_either_way"]] == t3r.RAW and code[k["all_inactive"]] == t3r.KEPT
        assert enc[tols[6]][0][k["all_inactive"]] == 0                                            # NaN rung: selected, no active voxel


def test_masked_sweep_of_4099_leaves(codec):
    mg.case_sweep_4099(codec, C)


@pytest.mark.parametrize("mode", ("fp32", "bf16"))
def test_host_pair_and_sweep_give_the_device_results_in_chunks_of_32(pack, base, mode):
    x, _, _, variants, tols = base
    codec = HipVec3Codec(pack, precision=mode)
    try:
        active = variants["designed"].copy()
        active[:N0] = variants["half"][:N0]
        masks = pack_masks(active)
        assert np.array_equal(masks, trm.pack_masks(active))
        idx, _, rec = dev_roundtrip(codec, x)                          # the mode's x^ of all 145 leaves, designed ones included
        err = mg.dev_err(codec, x, rec, masks)
        assert mg.same(err, trm.leaf_err_fixed(x, rec, active, C))
        tol = tols[2]
        code, off, buf = mg.dev_encode(codec, C, x, rec, masks, err, tol)
        codec.set_chunk_leaves(32)
        hi, hc, hp, he = codec.compress_residual_masked(x, masks, tol, return_leaf_err=True)
        hist = codec.rate_sweep_masked(x, masks, tols)
        out = codec.decompress_residual(hi, tol, hc, hp)               # the existing decompress call reads the masked records
        assert np.array_equal(hi, idx) and mg.same(he, err) and np.array_equal(hc, code) and np.array_equal(hp, buf[:off[-1]])
        assert np.array_equal(hist, mg.Resident(codec, C, x, rec, masks, err).sweep(tols).cpu().numpy())
        assert np.array_equal(hist, trm.sweep(x, rec, err, tols, active, C))
        quant = (hc != t3r.KEPT) & (hc != t3r.RAW)
        act = trm._active(active, C)
        with np.errstate(invalid="ignore"):
            assert (np.abs(x - out)[quant][act[quant]] <= F(tol)).all() and mg.same(out[hc == t3r.RAW], x[hc == t3r.RAW])
        assert mg.same(out, trm.apply(rec, tol, hc, hp.tobytes(), C))
        usize = t3r.record_size(codec.compress_residual(x, tol)[1])
        assert (t3r.record_size(hc) <= usize).all() and t3r.record_size(hc).sum() < usize.sum()
    finally:
        codec.close()


def test_refusals(codec, base):
    x, recon, _, variants, _ = base
    mg.case_refusals(codec, C, x, recon, variants["half"])
