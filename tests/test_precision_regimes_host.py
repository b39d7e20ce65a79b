"""bf16 decode mode of the scalar handle on six weight regimes, without a GPU: what
tests/test_gpu_precision_regimes.py relies on.  The per-element bound holds between the restatement's float32 and float64
transforms on the rows the GPU test decodes and rejects five defects a kernel could have; the planted weight sets give one
float32 result under any accumulation order, and another one under any other tie rule; the tail constants are what the fp32
path measures."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import precision_regimes as pr  # noqa: E402
import torch_ref_precision as tp  # noqa: E402

CONVS = (("conv1", "gn1"), ("conv2", "gn2"))
N_OUT = pr.N_ROWS * 64 * 64
# Outputs (of 151 552 per conv and regime) that a defect must push outside its bound: floors below the smallest count over the six
# regimes and both convs on the CPU (smallest: truncated weights 107 840, unrounded operands 79 445, kd / kw exchanged 151 310,
# wrapped padding tap 37 653 of the 37 888 outputs it touches).
MUTANT_MIN = {"trunc_w": 100000, "no_round": 75000, "swap_kd_kw": 151000, "wrap_pad": 37500}
# One weight zeroed: a corner tap reaches 27 positions of a leaf, 999 outputs over the 37 rows, fewer where its input channel is
# cut by the ReLU.  Floors at 0.9 of the CPU counts (conv1, conv2).
ZERO_W_MIN = {"seed0": (225, 673), "seed1": (500, 355), "seed2": (384, 520), "trained": (225, 217), "deadcodes": (228, 241),
              "default": (126, 418)}


@pytest.fixture(scope="module", params=pr.REGIMES)
def stage(request):
    """(regime, weights, {conv: (input, skip)}): the oracle's fp32 d_d2 and d_y4 on the regime's 37 rows, never written to."""
    regime = request.param
    _, dbg = pr.oracle_of(regime).decode(pr.rows(regime), debug=("d_d2", "d_y4"))
    for a in dbg.values():
        a.setflags(write=False)
    return regime, pr.weights_of(regime), {"conv1": (dbg["d_d2"], None), "conv2": (dbg["d_y4"], dbg["d_d2"])}


def test_rows_hold_every_code_and_fill_a_tile_and_a_ragged_half():
    for regime in pr.REGIMES:
        idx = pr.rows(regime)
        assert idx.shape == (37, 64) and idx.dtype == np.uint8
        assert len(np.unique(idx)) == 256
    assert not np.array_equal(pr.rows("trained"), pr.rows("deadcodes"))


def test_float32_transform_inside_the_bound_of_the_float64_transform(stage):
    """(a) of the issue, and that pr.restate without a defect is tests/torch_ref_precision.py bit for bit."""
    regime, w, inputs = stage
    for conv, gn in CONVS:
        x, skip = inputs[conv]
        bound, parts = pr.conv_bound(x, w, gn, conv, skip=skip, parts=True)
        r32 = pr.restate(x, w, gn, conv, skip=skip)
        r64 = pr.restate(x, w, gn, conv, skip=skip, transform_dtype=torch.float64)
        ref = tp.conv1(x, w) if skip is None else tp.conv2(x, skip, w)
        assert np.array_equal(r32.view(np.uint32), ref.view(np.uint32))
        worst, const, over = pr.ratios(r32, r64, bound, parts["mass"])
        print(f"{regime} {conv}: err / bound {worst:.3f}, {over} of {N_OUT} over; near inputs {parts['near_share']:.1e}; "
              f"mean terms acc {parts['acc'].mean():.2e} flip {parts['flip'].mean():.2e} rounding {parts['rnd'].mean():.2e}")
        assert bound.shape == (pr.N_ROWS, 64, 64) and np.all(bound > 0)
        assert over == 0 and worst <= 1.0
        assert parts["near_share"] < 2e-3      # the flip term is the exception, not a blanket


def test_the_bound_rejects_defects(stage):
    """(b) of the issue: each defect leaves the bound at no fewer outputs than the CPU run's floor."""
    regime, w, inputs = stage
    short = []
    for k, (conv, gn) in enumerate(CONVS):
        x, skip = inputs[conv]
        bound = pr.conv_bound(x, w, gn, conv, skip=skip)
        ref = pr.restate(x, w, gn, conv, skip=skip).astype(np.float64)
        for mutant in ("trunc_w", "no_round", "zero_w", "swap_kd_kw", "wrap_pad"):
            got = pr.restate(x, w, gn, conv, skip=skip, mutant=mutant)
            outside = int((np.abs(got - ref) > bound).sum())
            floor = ZERO_W_MIN[regime][k] if mutant == "zero_w" else MUTANT_MIN[mutant]
            print(f"{regime} {conv} {mutant}: {outside} outputs outside their bound (floor {floor})")
            if outside < floor:
                short.append((conv, mutant, outside, floor))
    assert not short, short


@pytest.mark.parametrize("r", range(pr.LIVE_SETS))
def test_planted_case_is_exact_in_any_order_and_feels_the_tie_rule(r):
    w = pr.planted_weights(r)
    live = [c for c in range(64) if c % pr.LIVE_SETS == r]
    for conv, gn in CONVS:
        beta, W = w[pr.P + gn + ".bias"], w[pr.P + conv + ".weight"]
        assert not w[pr.P + gn + ".weight"].any()
        # what is planted: ties to even both ways, their neighbours, negatives, both zeros; normal numbers only
        low = beta.view(np.uint32) & 0xFFFF
        odd = (beta.view(np.uint32) >> 16) & 1
        pos = beta > 0
        assert sorted(np.nonzero(pos)[0].tolist()) == live
        for lo_bits in (0x8000, 0x7FFF, 0x8001):
            for parity in (0, 1):
                assert np.any(pos & (low == lo_bits) & (odd == parity)), (gn, hex(lo_bits), parity)
        assert np.any(beta < 0) and np.any(beta.view(np.uint32) == 0x80000000) and np.any(beta.view(np.uint32) == 0)
        wl = W.view(np.uint32) & 0xFFFF
        assert set(np.unique(wl).tolist()) == {0x7FFF, 0x8000, 0x8001} and np.any(W < 0) and np.any(W > 0)
        assert len(np.unique(np.frexp(W)[1])) == 1 and len(np.unique(np.frexp(beta[beta != 0])[1])) == 1      # one binade each
        # integer arithmetic: every output's sum of magnitudes, in quanta, is a float32 integer
        val, budget = pr.closed_form(w, gn, conv)
        print(f"planted set {r} {conv}: largest sum of magnitudes {budget} quanta = {budget / 2 ** 24:.3f} of 2^24")
        assert budget < 2 ** 24
        # ... so the restatement's float64 sums, and a float32 chain in another order, give these very bits
        changed = {}
        for f in (pr.round_half_away, pr.round_half_up, pr.round_trunc):
            other, _ = pr.closed_form(w, gn, conv, f)
            changed[f.__name__] = int((other.view(np.uint32) != val.view(np.uint32)).sum())
        print(f"planted set {r} {conv}: outputs of 4096 whose bits another tie rule changes: {changed}")
        assert all(c >= 4000 for c in changed.values()), changed
    half_away, _ = pr.closed_form(w, "gn1", "conv1", pr.round_half_away)
    half_up, _ = pr.closed_form(w, "gn1", "conv1", pr.round_half_up)
    assert not np.array_equal(half_away, half_up)
    d2 = np.random.default_rng(40 + r).standard_normal((3, 64, 64)).astype(np.float32)
    v1, _ = pr.closed_form(w, "gn1", "conv1")
    v2, _ = pr.closed_form(w, "gn2", "conv2")
    y4 = tp.conv1(d2, w)
    assert np.array_equal(y4.view(np.uint32), np.broadcast_to(v1, y4.shape).view(np.uint32))
    x6 = tp.conv2(y4, d2, w)
    want = pr.planted_x6(d2, v2)
    assert np.array_equal(x6.view(np.uint32), want.view(np.uint32))
    # a float32 chain in reverse tap and channel order: the same bits
    kt = tp.rb(torch.from_numpy(np.maximum(w[pr.P + "gn1.bias"], np.float32(0)))).numpy()
    Wb = tp.rb(torch.from_numpy(w[pr.P + "conv1.weight"])).numpy().reshape(64, 64, 27)
    acc = np.zeros((64, 64), dtype=np.float32)
    for t in reversed(range(27)):
        for c in reversed(range(64)):
            acc = (acc + (Wb[:, c, t] * kt[c])[:, None] * pr.TAP_VALID[t][None, :].astype(np.float32)).astype(np.float32)
    acc = (acc + w[pr.P + "conv1.bias"][:, None]).astype(np.float32)
    assert np.array_equal(acc.view(np.uint32), v1.view(np.uint32))
    # the epilogue contracted into one fma would be seen
    fused = (d2.astype(np.float64) + float(np.float32(0.1)) * v2.astype(np.float64)[None]).astype(np.float32)
    assert int((fused.view(np.uint32) != want.view(np.uint32)).sum()) >= 500


def test_ref_tail_constants_are_what_the_fp32_path_measures():
    from test_gpu_precision_regimes import REF_TAIL
    assert sorted(REF_TAIL) == sorted(pr.REGIMES)
    for regime in pr.REGIMES:
        got = pr.ref_tail(regime)
        print(regime, got)
        for name in ("d_x7", "voxels"):
            for k in ("rms", "max"):
                assert abs(got[name][k] - REF_TAIL[regime][name][k]) <= 1e-5 * REF_TAIL[regime][name][k], (regime, name, k, got[name][k])
