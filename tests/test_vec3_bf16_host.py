"""bf16-operand inference mode of the Vec3 handle without a GPU: the C ABI of
include/vqvdb_hip_vec3_precision.h (declarations, exports, bindings), the wrapper's argument check, the torch restatement
tests/torch_ref_vec3_bf16.py against tests/torch_ref_vec3.py, the flip cap of the teacher-forced GPU test on the leaves that
test uses, and the restatement-pair constants of the end-to-end closeness test."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch_ref_vec3 as tr  # noqa: E402
import torch_ref_vec3_bf16 as tb  # noqa: E402
from vqvdb_amd import codec, synth_vec3  # noqa: E402

HEADER = os.path.join(ROOT, "include", "vqvdb_hip_vec3_precision.h")
FLIP_SHARE, FLIP_BOUND = 1e-3, 1e-3      # as tests/test_gpu_vec3_bf16.py
# `python tools/vec3_bf16_pair.py`; the same constants as tests/test_gpu_vec3_bf16.py REF_PAIR
REF_PAIR = {"index_share": 0.008353365384615384, "rms": 0.026919963339083922, "max": 0.4132680405407192, "mse_ratio": 1.0000118428673792}


@pytest.fixture(scope="module")
def w64():
    return tr.weights_to_torch(synth_vec3.make_weights(0), torch.float64)


@pytest.fixture(scope="module")
def leaves():
    return np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])


def test_header_library_and_bindings_hold_exactly_the_two_names():
    assert codec.VEC3_PRECISION_SYMBOLS == ["vqhip_vec3_set_precision", "vqhip_vec3_get_precision"]
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(vqhip_vec3_\w+)\s*\(", text))) == sorted(codec.VEC3_PRECISION_SYMBOLS)
    assert re.search(r"#define\s+VQHIP_VEC3_PRECISION_FP32\s+0\b", text) and re.search(r"#define\s+VQHIP_VEC3_PRECISION_BF16\s+1\b", text)
    for other in (codec.ABI_SYMBOLS, codec.VEC3_TRAIN_SYMBOLS, codec.VEC3_FULLTRAIN_SYMBOLS):
        assert not set(codec.VEC3_PRECISION_SYMBOLS) & set(other)
    lib = codec.load_library()
    for name in codec.VEC3_PRECISION_SYMBOLS:
        assert getattr(lib, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(vqhip_vec3_\w*precision\w*)\b", out)) == set(codec.VEC3_PRECISION_SYMBOLS)
    assert lib.vqhip_vec3_set_precision(None, 1) == -1 and lib.vqhip_vec3_get_precision(None, None) == -1
    assert len(codec.VEC3_DEBUG_LAYERS) == 12 and list(tb.STAGES) == list(codec.VEC3_DEBUG_LAYERS)


def test_wrapper_checks_the_precision_name_before_any_device():
    assert codec.HipVec3Codec.check_precision("fp32") == 0 and codec.HipVec3Codec.check_precision("bf16") == 1
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ValueError, match="precision must be one of"):
            codec.HipVec3Codec.check_precision(bad)
    with pytest.raises(ValueError, match="precision must be one of"):
        codec.HipVec3Codec(b"", precision="half")


def test_one_conv_on_bf16_representable_operands_equals_the_fp32_restatement():
    g = torch.Generator().manual_seed(7)
    w = {"c.weight": tb.rb(torch.randn(32, 16, 3, 3, 3, generator=g, dtype=torch.float64)),
         "c.bias": torch.randn(32, generator=g, dtype=torch.float64)}
    x = tb.rb(torch.randn(2, 16, 4, 4, 4, generator=g, dtype=torch.float64))
    ref = F.conv3d(x, w["c.weight"], w["c.bias"], padding=1)
    got = tb.conv_bf16(x, w, "c")
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    x2 = x * (1 + 2.0 ** -12)   # no longer representable: the rounding shows
    assert float((tb.conv_bf16(x2, w, "c") - F.conv3d(x2, w["c.weight"], w["c.bias"], padding=1)).abs().max()) > 1e-6


def test_restatement_differs_from_fp32_on_the_fixture_leaves(w64, leaves):
    with torch.no_grad():
        a, b = {}, {}
        tb.encoder(leaves[:4], w64, a)
        tr.encoder(leaves[:4], w64, b)
    for k in a:
        d = float((a[k] - b[k]).abs().max() / b[k].abs().max())
        assert (1e-5 < d < 5e-2) if k != "encoder.pre.0" else (1e-6 < d < 5e-2), (k, d)


def test_flip_cap_holds_between_fp32_and_fp64_transforms_on_the_stage_leaves(w64, leaves):
    """The condition of the teacher-forced GPU test, on its leaves: the restatement with its transforms in float32 against
    the same restatement with its transforms in float64, each stage from the same input."""
    from test_gpu_vec3_bf16 import STAGE_IDS, STAGE_LEAVES
    assert STAGE_IDS[0] == 0 and len(set(STAGE_IDS)) >= 32
    x = leaves[STAGE_IDS]
    with torch.no_grad():
        acts = {}
        idx, _ = tb.encode(x, w64, acts)
        tb.decode(idx.numpy(), w64, acts)
        prev = {k: v.reshape(v.shape[0], v.shape[1], -1).numpy() for k, v in acts.items()}
        prev["leaves"] = x
        prev["codes"] = tb.codes(idx.numpy(), w64).reshape(STAGE_LEAVES, 64, 64).numpy()
    for name, (p, _fn) in tb.STAGES.items():
        a = tb.stage(name, prev[p], w64, torch.float32).numpy()
        b = tb.stage(name, prev[p], w64, torch.float64).numpy()
        err, top = np.abs(a - b), float(np.abs(b).max())
        share = float((err > 1e-5 * top).mean())
        print(f"{name}: share over 1e-5 {share:.2e}, max {err.max() / top:.2e}")
        assert share <= FLIP_SHARE and float(err.max()) <= FLIP_BOUND * top, name


def test_restatement_pair_constants_are_what_the_tool_measures(w64, leaves):
    import vec3_bf16_pair
    got = vec3_bf16_pair.pair(leaves, w64)
    print(got)
    for k, v in REF_PAIR.items():
        assert got[k] == pytest.approx(v, rel=1e-4), k
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_vec3_bf16.py")).read()
    assert repr(REF_PAIR["rms"]) in gpu_test and repr(REF_PAIR["index_share"]) in gpu_test
