"""bf16 encode mode of the scalar handle without a GPU: the C ABI of include/vqvdb_hip_encode_mode.h, the
wrapper's argument check, tests/torch_ref_encode_mode.py pinned to the oracle's fp32 contract, the flip cap of the teacher-forced
GPU test on the leaves it uses, the index criterion on the reference alone, the planted ties, and the constants the GPU
end-to-end test compares against."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import precision_regimes as pr  # noqa: E402
import torch_ref_encode_mode as te  # noqa: E402
from vqvdb_amd import codec, synth  # noqa: E402

FLIP_SHARE, FLIP_BOUND = 1e-3, 1e-3      # the project's cap (tests/test_gpu_precision.py)
GAP = 1e-5                               # §4's bar on the relative top-2 gap
GAP_SHARE = 0.01
REGIMES = ("seed0", "trained")
# torch_ref_encode_mode.ref_ratios on pair_leaves(): mean ||x - decode(encode(x))||^2 of the restated bf16 mode over the fp32
# mode, with float32 and with float64 transforms (test_ref_ratio_constants_are_what_the_restatement_measures recomputes them)
REF_RATIO = {"float32": 1.0000000496138401, "float64": 1.0000000496138401}


def stage_leaves():
    """The 35 leaves of the teacher-forced GPU tests (a full tile and 3 leaves of a second one), from the generators of the
    regimes fixture: 16 uniform leaves (synth.make_leaves(., seed=9001)), 11 of the first 12 sparse leaves
    (synth.sparse_leaves(., seed=9002)) and the 8 edge leaves.  Sparse leaf 3 is left out: under the seed0 weights its conv1
    activations sit so close to bf16 rounding boundaries that the restatement with float64 transforms already rounds some the
    other way, one such activation feeds up to 432 outputs, and 3.9 % of that leaf's e_y4 elements move by more than 1e-5 of
    the largest value: 1.07e-3 of the whole 36-leaf tensor, over the cap's share."""
    x = np.concatenate([synth.make_leaves(16, seed=9001), synth.sparse_leaves(12, seed=9002)[[0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]], synth.edge_leaves()])
    assert x.shape == (35, 512)
    return np.ascontiguousarray(x)


def inside_cap(got, ref):
    """(inside the flip cap?, largest error / largest value, share over 1e-5) of a tensor pair."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    top = float(np.abs(ref).max())
    share = float((err > 1e-5 * top).mean())
    return share <= FLIP_SHARE and float(err.max()) <= FLIP_BOUND * top, float(err.max()) / top, share


def test_header_library_and_bindings_hold_exactly_the_two_names():
    hdr = open(os.path.join(ROOT, "include", "vqvdb_hip_encode_mode.h")).read()
    declared = sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == sorted(codec.ENCODE_MODE_SYMBOLS) == ["vqhip_get_encode_mode", "vqhip_set_encode_mode"]
    others = [v for k, v in vars(codec).items() if k.endswith("_SYMBOLS") and k != "ENCODE_MODE_SYMBOLS"]
    assert len(others) >= 10 and codec.ABI_SYMBOLS in others and codec.PRECISION_SYMBOLS in others
    for names in others:
        assert not set(codec.ENCODE_MODE_SYMBOLS) & set(names)
    base = open(os.path.join(ROOT, "include", "vqvdb_hip.h")).read()
    assert not [s for s in codec.ENCODE_MODE_SYMBOLS if s in base]
    assert '#include "vqvdb_hip_precision.h"' in hdr and "#define" not in hdr.split("VQVDB_HIP_ENCODE_MODE_H", 2)[2]
    from vqvdb_amd.build import build
    out = subprocess.run(["nm", "-D", "--defined-only", build()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in codec.ENCODE_MODE_SYMBOLS if s not in exported]
    lib = codec.load_library()
    for s in codec.ENCODE_MODE_SYMBOLS:
        assert getattr(lib, s).argtypes is not None and len(getattr(lib, s).argtypes) == 2


def test_wrapper_checks_the_precision_name_before_any_device():
    assert codec.HipCodec.check_encode_precision("fp32") == 0 and codec.HipCodec.check_encode_precision("bf16") == 1
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ValueError, match="encode_precision must be one of"):
            codec.HipCodec.check_encode_precision(bad)
    with pytest.raises(ValueError, match="encode_precision must be one of"):
        codec.HipCodec(b"", encode_precision="half")   # refused before the library is loaded or a device is touched


@pytest.mark.parametrize("regime", REGIMES)
def test_restatement_without_rounding_is_the_fp32_contract(regime):
    """Operand rounding off: e_y4 and e_a6 of the oracle within 1e-6 of each tensor's largest value, teacher-forced and chained."""
    w = pr.weights_of(regime)
    _, dbg = pr.oracle_of(regime).encode(stage_leaves(), debug=("e_a1", "e_y4", "e_a6"))
    y4 = te.conv1(dbg["e_a1"], w, round_operands=False)
    a6 = te.conv2(dbg["e_y4"], dbg["e_a1"], w, round_operands=False)
    a6_chain = te.conv2(y4, dbg["e_a1"], w, round_operands=False)
    for name, got, ref in (("e_y4", y4, dbg["e_y4"]), ("e_a6", a6, dbg["e_a6"]), ("e_a6 chained", a6_chain, dbg["e_a6"])):
        rel = float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())
        print(f"{regime} {name}: {rel:.2e} of the largest value")
        assert rel < 1e-6, name
    # ... and with it on the restatement is a different function: the mode is visible at the scale of bf16's 2^-9
    assert float(np.abs(te.conv1(dbg["e_a1"], w) - dbg["e_y4"]).max() / np.abs(dbg["e_y4"]).max()) > 1e-4
    assert float(np.abs(te.conv2(dbg["e_y4"], dbg["e_a1"], w) - dbg["e_a6"]).max() / np.abs(dbg["e_a6"]).max()) > 1e-4


@pytest.mark.parametrize("regime", REGIMES)
def test_flip_cap_holds_between_fp32_and_fp64_transforms_on_the_stage_leaves(regime):
    """The GPU test's cap is a property of the chosen leaves: the restatement with float32 transforms against the same with
    float64 transforms stays inside it for both convs teacher-forced, and chained from e_a1 to e_a6."""
    w = pr.weights_of(regime)
    _, dbg = pr.oracle_of(regime).encode(stage_leaves(), debug=("e_a1",))
    a1 = dbg["e_a1"]
    y4_32, a6_32 = te.res_block(a1, w)
    y4_64, a6_64 = te.res_block(a1, w, transform_dtype=torch.float64)
    pairs = {
        "conv1": (y4_32, y4_64),
        "conv2 teacher-forced": (te.conv2(y4_32, a1, w), te.conv2(y4_32, a1, w, transform_dtype=torch.float64)),
        "e_a1 to e_a6": (a6_32, a6_64),
    }
    bad = []
    for name, (a, b) in pairs.items():
        ok, worst, share = inside_cap(a, b)
        print(f"{regime} {name}: largest error {worst:.2e} of the largest value, share over 1e-5: {share:.2e}")
        if not ok:
            bad.append(name)
    assert not bad


@pytest.mark.parametrize("regime", REGIMES)
def test_index_criterion_holds_for_the_reference_alone(regime):
    """From the oracle's fp32 e_a6 the float64 rest of the encoder: the oracle's index is the float64 argmin wherever the float64
    relative top-2 gap is at least 1e-5, its e_x7 / e_x11 lie within 1e-5 of the float64 tensors' largest value, and at most
    1 % of the positions of the stage leaves fall under the gap."""
    w = pr.weights_of(regime)
    idx, dbg = pr.oracle_of(regime).encode(stage_leaves(), debug=("e_a6", "e_x7", "e_x11"))
    am, gap, x7, x11 = te.rest(dbg["e_a6"], w)
    under = gap < GAP
    print(f"{regime}: {float(under.mean()):.2e} of the positions under the gap, {int((am != idx).sum())} indices off the float64 argmin")
    assert not ((am != idx) & ~under).any()
    assert float(under.mean()) <= GAP_SHARE
    for name, ref in (("e_x7", x7), ("e_x11", x11)):
        assert float(np.abs(dbg[name] - ref).max()) <= 1e-5 * float(np.abs(ref).max()), name


@pytest.mark.parametrize("r", range(te.LIVE_SETS))
def test_planted_ties_have_one_possible_result_and_other_roundings_change_it(r):
    w = te.planted_weights(r)
    for gn, conv in (("gn1", "conv1"), ("gn2", "conv2")):
        beta = w[te.P + gn + ".bias"].view(np.uint32)
        live = beta[r::te.LIVE_SETS]
        assert np.all((live >> 31) == 0) and set((live & 0xFFFF).tolist()) == {0x7FFF, 0x8000, 0x8001}      # ties and both neighbours
        assert {int(m) & 1 for m in (live[(live & 0xFFFF) == 0x8000] >> 16)} == {0, 1}                      # ties that round down, ties that round up
        wb = w[te.P + conv + ".weight"].view(np.uint32)
        assert set((wb & 0xFFFF).reshape(-1).tolist()) == {0x7FFF, 0x8000, 0x8001}
        v, budget = te.closed_form(w, gn, conv)
        assert isinstance(budget, int) and budget < 2 ** 24, (conv, budget)
        # the restatement (float64 sums) is the closed form: the planted case is inside the contract it states
        a1 = np.zeros((1, 16, 512), dtype=np.float32)
        got = te.conv1(a1, w) if conv == "conv1" else te.conv2(a1, a1, w)
        want = v[None] if conv == "conv1" else te.planted_a6(a1, v)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), conv
        for other in (te.round_half_up, te.round_half_away, te.round_trunc):
            v2, _ = te.closed_form(w, gn, conv, other)
            changed = int((v2 != v).sum())
            print(f"set {r} {conv} {other.__name__}: {changed} of {v.size} outputs change")
            assert changed > v.size // 2, (conv, other.__name__)
    # conv2's epilogue: one rounding (an fma) instead of two changes stored bits for a skip tensor of ordinary values
    v, _ = te.closed_form(w, "gn2", "conv2")
    a1 = synth.make_leaves(16, seed=31).reshape(1, 16, 512)
    two, one = te.planted_a6(a1, v), te.planted_a6(a1, v, fma=True)
    changed = int((two.view(np.uint32) != one.view(np.uint32)).sum())
    print(f"set {r}: an fma in conv2's epilogue changes {changed} of {two.size} elements")
    assert changed > 0


def test_ref_ratio_constants_are_what_the_restatement_measures(oracle, weights):
    got = te.ref_ratios(oracle, weights)
    print(got)
    assert set(got) == set(REF_RATIO)
    for k in got:
        assert abs(got[k] - REF_RATIO[k]) <= 1e-9, (k, got[k], REF_RATIO[k])
