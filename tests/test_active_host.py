"""Compact residual records of the Vec3 handle without a GPU: the numpy restatement tests/torch_ref_active.py held
against the format's properties (all-ones mask == the masked records, sizes, single active voxels, active counts around the word
boundaries, padding, what apply leaves at active and inactive voxels), and the C ABI of include/vqvdb_hip_vec3_active.h
(declarations, exports, bindings, forbidden strings, NULL handle, the record-size function)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_active as tra  # noqa: E402
import torch_ref_masked as trm  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import codec  # noqa: E402

F = np.float32
NAMES = ["vqhip_vec3_active_record_bytes", "vqhip_vec3_active_encode_device", "vqhip_vec3_active_apply_device", "vqhip_vec3_active_sweep_device",
         "vqhip_vec3_active_compress", "vqhip_vec3_active_decompress", "vqhip_vec3_active_sweep"]
ARITY = dict(zip(NAMES, (2, 12, 10, 10, 10, 10, 7)))
FORBIDDEN = ("vqhip_vec3_mask_", "vqhip_mask_", "vqhip_rate_", "vqhip_vec3_rate_")
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 511, 512)


def count_masks(n, seed=3):
    """bool [n,512]: leaf i has COUNTS[i % 10] active voxels at random positions"""
    rng = np.random.default_rng(seed)
    active = np.zeros((n, 512), bool)
    for i in range(n):
        active[i, rng.permutation(512)[:COUNTS[i % len(COUNTS)]]] = True
    return active


def random_batch(n=30, seed=8):
    """finite x^ and x = x^ + noise whose scale differs from leaf to leaf; a NaN in two leaves' x (raw where it is active)"""
    rng = np.random.default_rng(seed)
    recon = rng.standard_normal((n, 512, 3)).astype(F)
    scale = (10.0 ** rng.uniform(-3, 0, n)).astype(F).reshape(n, 1, 1)
    x = (recon + rng.standard_normal((n, 512, 3)).astype(F) * scale).astype(F)
    x[3, 100, 1] = np.nan
    x[14, :, 0] = np.nan
    return x, recon


@pytest.fixture(scope="module")
def batch():
    """(x, x^) of the designed input and 30 random leaves, their tolerances"""
    dx, dr, dact, _ = trm.designed(3)
    rx, rr = random_batch()
    x, recon = np.concatenate([dx, rx]), np.concatenate([dr, rr])
    err = trm.leaf_err_fixed(rx, rr, np.ones((len(rx), 512), bool), 3)[:, 0]
    err = err[np.isfinite(err)]
    return x, recon, dact, [trm.TOL_D, float(np.median(err)), float(err.min()), float("nan")]


def masks_of(x, dact):
    n = len(x)
    rng = np.random.default_rng(12)
    own = rng.random((n, 512)) < 0.5
    own[:len(dact)] = dact
    return {"ones": np.ones((n, 512), bool), "designed_half": own, "sparse": rng.random((n, 512)) < 0.05, "counts": count_masks(n),
            "zeros": np.zeros((n, 512), bool)}


def test_all_ones_mask_gives_the_masked_records_byte_for_byte(batch):
    x, recon, _, tols = batch
    ones = np.ones((len(x), 512), bool)
    err = trm.leaf_err_fixed(x, recon, ones, 3)
    for tol in tols:
        code, off = trm.classify(x, recon, err, tol, ones, 3)
        assert tra.pack(x, recon, tol, code, ones) == trm.pack(x, recon, tol, code, ones, 3), tol
        assert np.array_equal(tra.offsets(code, ones), off), tol
    assert (trm.classify(x, recon, err, tols[0], ones, 3)[0] == t3r.RAW).any()


def test_sizes_follow_the_table_and_never_exceed_the_masked_size(batch):
    x, recon, dact, tols = batch
    for name, active in masks_of(x, dact).items():
        err = trm.leaf_err_fixed(x, recon, active, 3)
        A = active.sum(axis=1)
        for tol in tols:
            code, moff = trm.classify(x, recon, err, tol, active, 3)
            payload = tra.pack(x, recon, tol, code, active)
            recs = tra.records(code, payload, active)
            for i, c in enumerate(code):
                c, b = int(c), t3r.widths(int(c)).sum()
                want = 0 if c == t3r.KEPT else 8 * ((3 * A[i] + 1) // 2) if c == t3r.RAW else 8 * ((A[i] + 63) // 64) * b
                assert len(recs[i]) == want == tra.record_size(c, A[i]) and want % 8 == 0, (name, tol, i)
                assert want <= np.diff(moff)[i], (name, tol, i)
            assert tra.offsets(code, active)[-1] == len(payload) <= len(x) * 6144
            assert np.array_equal(tra.sweep_bytes(x, recon, err, [tol], active), [len(payload)])


def test_single_active_voxels_cost_eight_bytes_per_plane():
    x, recon, active, kinds = trm.designed(3)
    err = trm.leaf_err_fixed(x, recon, active, 3)
    code, moff = trm.classify(x, recon, err, trm.TOL_D, active, 3)
    recs = tra.records(code, tra.pack(x, recon, trm.TOL_D, code, active), active)
    for name in ("single_0", "single_63", "single_64", "single_511"):
        i = kinds.index(name)
        planes = int(t3r.widths(int(code[i])).sum())
        assert planes > 0 and len(recs[i]) == 8 * planes == 136 and np.diff(moff)[i] == 64 * planes == 1088, name
        words = np.frombuffer(recs[i], "<u8")
        assert not (words & ~np.uint64(1)).any(), name                 # rank 0 is bit 0 of the one word of every plane
    rcode = trm.classify(x, recon, err, float("nan"), active, 3)[0]    # a NaN tolerance: every selected leaf with a voxel is raw
    rrecs = tra.records(rcode, tra.pack(x, recon, float("nan"), rcode, active), active)
    for name, v in (("single_0", 0), ("single_63", 63), ("single_64", 64), ("single_511", 511)):
        i = kinds.index(name)
        assert rcode[i] == t3r.RAW and len(rrecs[i]) == 16
        assert rrecs[i][:12] == x[i, v].tobytes() and rrecs[i][12:] == bytes(4)
    assert rcode[kinds.index("all_inactive")] == 0 and rrecs[kinds.index("all_inactive")] == b""


def test_active_counts_around_the_word_boundaries_round_trip(batch):
    x, recon, _, tols = batch
    active = count_masks(len(x))
    A = active.sum(axis=1)
    assert set(A) == set(COUNTS)
    err = trm.leaf_err_fixed(x, recon, active, 3)
    rk = tra.ranks(active)
    assert all(np.array_equal(rk[i][active[i]], np.arange(A[i])) for i in range(len(x)))
    for tol in tols:
        code, _ = trm.classify(x, recon, err, tol, active, 3)
        payload = tra.pack(x, recon, tol, code, active)
        zz, _ = trm.quantise(x, recon, tol, active, 3)
        zz = zz.reshape(len(x), 512, 3)
        for i, rec in enumerate(tra.records(code, payload, active)):
            c = int(code[i])
            if c == t3r.RAW:
                assert rec[:12 * A[i]] == x[i][active[i]].tobytes()
                assert rec[12 * A[i]:] == bytes(4 * (A[i] % 2)), (tol, i)                     # odd A: four zero bytes of padding
            elif c != t3r.KEPT:
                assert np.array_equal(t3r.zigzag(tra.unpack_leaf(rec, c, A[i])), zz[i][active[i]]), (tol, i)
    assert (A[trm.classify(x, recon, err, float("nan"), active, 3)[0] == t3r.RAW] % 2 == 1).any()


def test_apply_corrects_active_values_and_leaves_or_fills_inactive_ones(batch):
    x, recon, dact, tols = batch
    background = np.array([-0.0, np.nan, 1e30], F)
    for name, active in masks_of(x, dact).items():
        err = trm.leaf_err_fixed(x, recon, active, 3)
        act3 = trm._active(active, 3)
        planted = recon.copy()
        planted[~act3] = np.nan                                        # whatever x^ holds at an inactive voxel
        for tol in tols[:3]:
            code, _ = trm.classify(x, recon, err, tol, active, 3)
            payload = tra.pack(x, recon, tol, code, active)
            out = tra.apply(planted, tol, code, payload, active)
            assert out.dtype == F and out[~act3].tobytes() == planted[~act3].tobytes(), (name, tol)      # bit-unchanged, NaN included
            masked = trm.apply(recon, tol, code, trm.pack(x, recon, tol, code, active, 3), 3)
            assert out[act3].tobytes() == masked[act3].tobytes(), (name, tol)
            quant = (code != t3r.KEPT) & (code != t3r.RAW)
            with np.errstate(invalid="ignore"):
                assert (np.abs(x - out)[quant][act3[quant]] <= F(tol)).all(), (name, tol)            # the decoder's own float32 arithmetic
            raw = code == t3r.RAW
            assert out[raw][act3[raw]].tobytes() == x[raw][act3[raw]].tobytes()
            filled = tra.apply(planted, tol, code, payload, active, background)
            assert filled[act3].tobytes() == out[act3].tobytes()
            assert filled[~active].tobytes() == np.tile(background, ((~active).sum(), 1)).tobytes(), (name, tol)


def test_header_library_and_bindings_hold_exactly_the_seven_names():
    assert codec.VEC3_ACTIVE_SYMBOLS == NAMES
    raw = open(os.path.join(ROOT, "include", "vqvdb_hip_vec3_active.h")).read()
    for s in FORBIDDEN:
        assert s not in raw, s                                         # comments included: older tests search every header
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(NAMES)
    assert all(n.startswith("vqhip_vec3_active_") and "precision" not in n for n in NAMES)
    assert re.search(r'#include\s+"vqvdb_hip_vec3_mask.h"', text)
    lib = codec.load_library()
    for name in NAMES:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert params.count(",") + 1 == ARITY[name], name
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == ARITY[name], name
        assert f.restype == (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int), name
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_\w+)\b", out))
    assert {n for n in exported if n.startswith("vqhip_vec3_active_")} == set(NAMES)
    assert not {n for n in exported if n.startswith("vqhip_mask_")}
    others = [v for k, v in vars(codec).items() if k.endswith("_SYMBOLS") and k != "VEC3_ACTIVE_SYMBOLS"]
    assert len(others) >= 10 and codec.VEC3_MASK_SYMBOLS in others
    for other in others:
        assert not set(NAMES) & set(other)
    assert "active" not in open(os.path.join(ROOT, "include", "vqvdb_hip.h")).read().lower()   # nothing new in the base header


def test_a_null_handle_is_refused_without_a_device():
    lib = codec.load_library()
    tols, sums, nbytes, bg = np.array([0.5], F), np.zeros(1, np.int64), ctypes.c_int64(0), np.zeros(3, F)
    assert lib.vqhip_vec3_active_encode_device(None, None, None, None, None, 1, 0.5, None, None, None, 0, None) == -1
    assert lib.vqhip_vec3_active_apply_device(None, None, None, 1, 0.5, None, None, None, bg.ctypes.data, None) == -1
    assert lib.vqhip_vec3_active_sweep_device(None, None, None, None, None, 1, tols.ctypes.data, 1, None, None) == -1
    assert lib.vqhip_vec3_active_compress(None, None, None, 1, 0.5, None, None, None, None, ctypes.byref(nbytes)) == -1
    assert lib.vqhip_vec3_active_decompress(None, None, None, 1, 0.5, None, None, 0, None, None) == -1
    assert lib.vqhip_vec3_active_sweep(None, None, None, 1, tols.ctypes.data, 1, sums.ctypes.data) == -1


def test_record_bytes_equals_the_restatement():
    lib = codec.load_library()
    codes = [t3r.KEPT, t3r.RAW, 0, t3r.make_code(16, 16, 16), t3r.make_code(1, 0, 0), t3r.make_code(0, 7, 0), t3r.make_code(3, 0, 16),
             t3r.make_code(5, 9, 2)]
    for c in codes:
        for A in (0, 1, 63, 64, 65, 511, 512):
            want = int(tra.record_size(c, A))
            assert lib.vqhip_vec3_active_record_bytes(c, A) == want == codec.vec3_active_record_bytes(c, A), (c, A)
        assert lib.vqhip_vec3_active_record_bytes(c, 512) == int(t3r.record_size(c))           # all active: the masked size
        assert lib.vqhip_vec3_active_record_bytes(c, 513) == -1 and lib.vqhip_vec3_active_record_bytes(c, -1) == -1
    for bad in (t3r.make_code(17, 0, 0), t3r.make_code(0, 0, 17), 0x8000, 0x10000, -1):
        assert lib.vqhip_vec3_active_record_bytes(bad, 64) == -1, bad
    with pytest.raises(ValueError, match="no record size"):
        codec.vec3_active_record_bytes(t3r.make_code(17, 0, 0), 64)
    with pytest.raises(ValueError, match="no record size"):
        codec.vec3_active_record_bytes(0, 513)
    with pytest.raises(TypeError, match="integer"):
        codec.vec3_active_record_bytes(0.0, 5)


def test_wrapper_checks_its_arguments_before_any_device():
    m = np.zeros((2, 8), np.uint64)
    leaves, idx = np.zeros((2, 512, 3), F), np.zeros((2, 64), np.uint16)
    fake = object.__new__(codec.HipVec3Codec)                          # no handle: every check below runs before the library is called
    with pytest.raises(TypeError, match="uint64"):
        fake.compress_active(leaves, m.astype(np.int64), 0.5)
    with pytest.raises(ValueError, match="2 leaves but 3 masks"):
        fake.compress_active(leaves, np.zeros((3, 8), np.uint64), 0.5)
    with pytest.raises(ValueError, match="shape"):
        fake.rate_sweep_active(leaves, np.zeros((2, 7), np.uint64), [0.5])
    with pytest.raises(ValueError, match="1..64 tolerances"):
        fake.rate_sweep_active(leaves, m, [])
    with pytest.raises(ValueError, match="NULL device pointer"):
        fake.active_encode_device(1, 1, 0, 1, 2, 0.5, 1, 1, 1, 10)
    with pytest.raises(ValueError, match="payload_capacity"):
        fake.active_encode_device(1, 1, 1, 1, 2, 0.5, 1, 1, 1, -1)
    with pytest.raises(ValueError, match="NULL device pointer"):
        fake.active_apply_device(1, 0, 2, 0.5, 1, 1, 1)
    with pytest.raises(ValueError, match="three numbers"):
        fake.active_apply_device(1, 1, 2, 0.5, 1, 1, 1, background=[0.0, 1.0])
    with pytest.raises(ValueError, match="NULL device pointer"):
        fake.active_sweep_device(1, 1, 0, 1, 2, [0.5], 1)
    with pytest.raises(ValueError, match="1..64 tolerances"):
        fake.active_sweep_device(1, 1, 1, 1, 2, [0.5] * 65, 1)
    full = np.full((2, 8), 0xFFFFFFFFFFFFFFFF, np.uint64)
    code = np.array([t3r.make_code(1, 1, 1), t3r.RAW], np.uint16)
    assert np.array_equal(codec.HipVec3Codec.active_counts(np.array([[1, 0, 0, 0, 0, 0, 0, 1 << 63], [0] * 8], np.uint64)), [2, 0])
    assert np.array_equal(codec.HipVec3Codec.active_record_sizes(code, full), [192, 6144])
    assert np.array_equal(codec.HipVec3Codec.active_record_sizes(code, m), [0, 0])
    with pytest.raises(ValueError, match="need 6336 payload bytes, got 8"):
        fake.decompress_active(idx, full, 0.5, code, bytes(8))
    with pytest.raises(ValueError, match="2 leaves but 1 codes"):
        fake.decompress_active(idx, full, 0.5, code[:1], bytes(8))
    with pytest.raises(ValueError, match="widths? in 0..16|every width"):
        fake.decompress_active(idx, full, 0.5, np.array([t3r.make_code(17, 0, 0), 0], np.uint16), b"")
