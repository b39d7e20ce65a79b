"""bf16 decode mode of the scalar handle without a GPU: the C ABI of include/vqvdb_hip_precision.h, the wrapper's
argument check, the bf16 rounding, tests/torch_ref_precision.py pinned to the oracle's fp32 contract, the flip cap of the
teacher-forced GPU test on the index rows it uses, and the constants the GPU closeness test compares against."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_precision as tp  # noqa: E402
from vqvdb_amd import codec  # noqa: E402

FLIP_SHARE, FLIP_BOUND = 1e-3, 1e-3      # as tests/test_gpu_precision.py


def stage_rows(golden):
    """The 33 index rows of the teacher-forced GPU test: 26 of the fixture's uniform leaves and 7 of its 8 edge leaves.  Edge
    leaf 4 is left out: one of its conv1 activations sits within a float32 ulp of a bf16 rounding boundary, where the
    restatement with float64 transforms already rounds it the other way, and one such activation moves up to 1 728 outputs
    (1 000 of that leaf's d_y4 elements by more than 1e-5), more than the cap's share of the whole tensor."""
    return np.ascontiguousarray(np.concatenate([golden["idx_rand"][:26], golden["idx_edge"][[0, 1, 2, 3, 5, 6, 7]]]))


def inside_cap(got, ref):
    """(inside the flip cap?, largest error / largest value, share over 1e-5) per leaf-independent tensor pair."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    top = float(np.abs(ref).max())
    share = float((err > 1e-5 * top).mean())
    return share <= FLIP_SHARE and float(err.max()) <= FLIP_BOUND * top, float(err.max()) / top, share


def test_header_library_and_bindings_hold_exactly_the_two_names():
    hdr = open(os.path.join(ROOT, "include", "vqvdb_hip_precision.h")).read()
    declared = sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == sorted(codec.PRECISION_SYMBOLS)
    assert not set(codec.PRECISION_SYMBOLS) & set(codec.ABI_SYMBOLS)
    base = open(os.path.join(ROOT, "include", "vqvdb_hip.h")).read()
    assert not [s for s in codec.PRECISION_SYMBOLS if s in base]
    assert "VQHIP_PRECISION_FP32 0" in hdr and "VQHIP_PRECISION_BF16 1" in hdr
    assert codec.PRECISIONS == {"fp32": 0, "bf16": 1}
    from vqvdb_amd.build import build
    out = subprocess.run(["nm", "-D", "--defined-only", build()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in codec.PRECISION_SYMBOLS if s not in exported]
    lib = codec.load_library()
    for s in codec.PRECISION_SYMBOLS:
        assert getattr(lib, s).argtypes is not None


def test_wrapper_checks_the_precision_name_before_any_device():
    assert codec.HipCodec.check_decode_precision("fp32") == 0 and codec.HipCodec.check_decode_precision("bf16") == 1
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ValueError, match="decode_precision must be one of"):
            codec.HipCodec.check_decode_precision(bad)
    with pytest.raises(ValueError, match="decode_precision must be one of"):
        codec.HipCodec(b"", decode_precision="half")   # refused before the library is loaded or a device is touched


def test_bf16_rounding_equals_torch_on_the_edge_values():
    u = np.array([
        0x00000000, 0x80000000,                          # both zeros
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even down, to even up, both signs
        0x3F807FFF, 0x3F808001, 0x3F80FFFF,              # just below / above a tie, carry into the next bf16
        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000,   # subnormals (ties among them) and the smallest normal
        0x7F7FFFFF, 0xFF7FFFFF,                          # the largest finite values round to infinity
        0x7F800000, 0xFF800000,                          # infinities
        0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF80FFFF, 0x7FFFFFFF,   # quiet and signalling NaNs
    ], dtype=np.uint32)
    rng = np.random.default_rng(5)
    u = np.concatenate([u, rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)])
    x = u.view(np.float32)
    got = tp.bf16_bits(x)
    ref = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], ref[~nan])
    # NaN stays a quiet NaN of the same sign (torch returns one canonical NaN; the payload is not part of the contract)
    assert np.all((got[nan] & 0x7FC0) == 0x7FC0) and np.array_equal(got[nan] >> 15, (u[nan] >> 31).astype(np.uint16))
    assert np.all(np.isnan(torch.from_numpy(ref[nan].view(np.int16).copy()).view(torch.bfloat16).float().numpy()))


def test_restatement_without_rounding_is_the_fp32_contract(oracle, weights, golden):
    """Operand rounding off: d_y4 and d_x6 of the oracle within 1e-6 of each tensor's largest value, teacher-forced and chained."""
    idx = stage_rows(golden)
    _, dbg = oracle.decode(idx, debug=("d_d2", "d_y4", "d_x6"))
    y4 = tp.conv1(dbg["d_d2"], weights, round_operands=False)
    x6 = tp.conv2(dbg["d_y4"], dbg["d_d2"], weights, round_operands=False)
    x6_chain = tp.conv2(y4, dbg["d_d2"], weights, round_operands=False)
    for name, got, ref in (("d_y4", y4, dbg["d_y4"]), ("d_x6", x6, dbg["d_x6"]), ("d_x6 chained", x6_chain, dbg["d_x6"])):
        rel = float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())
        print(f"{name}: {rel:.2e} of the largest value")
        assert rel < 1e-6, name
    # ... and with it on the restatement is a different function: the mode is visible at the scale of bf16's 2^-9
    assert float(np.abs(tp.conv1(dbg["d_d2"], weights) - dbg["d_y4"]).max() / np.abs(dbg["d_y4"]).max()) > 1e-4


def test_flip_cap_holds_between_fp32_and_fp64_transforms_on_the_stage_rows(oracle, weights, golden):
    """The GPU test's cap is a property of the chosen rows: the restatement with float32 transforms against the same with
    float64 transforms stays inside it for both convs teacher-forced, and end to end from the indices to d_x6."""
    idx = stage_rows(golden)
    _, dbg = oracle.decode(idx, debug=("d_d2", "d_y4"))
    d2 = dbg["d_d2"]
    y4_32, x6_32 = tp.res_block(d2, weights)
    y4_64, x6_64 = tp.res_block(d2, weights, transform_dtype=torch.float64)
    pairs = {
        "conv1": (y4_32, y4_64),
        "conv2 teacher-forced": (tp.conv2(y4_32, d2, weights), tp.conv2(y4_32, d2, weights, transform_dtype=torch.float64)),
        "indices to d_x6": (x6_32, x6_64),
    }
    bad = []
    for name, (a, b) in pairs.items():
        ok, worst, share = inside_cap(a, b)
        print(f"{name}: largest error {worst:.2e} of the largest value, share over 1e-5: {share:.2e}")
        if not ok:
            bad.append(name)
    assert not bad


def test_ref_pair_constants_are_what_the_restatement_measures(oracle, weights):
    from test_gpu_precision import REF_PAIR
    got = tp.ref_pair(oracle, weights)
    print(got)
    assert set(got) == {"rms", "max", "mse_ratio"}
    for k in got:
        assert abs(got[k] - REF_PAIR[k]) <= 1e-6 * abs(REF_PAIR[k]), (k, got[k], REF_PAIR[k])
