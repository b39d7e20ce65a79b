"""bf16 decode mode of the scalar handle on six weight regimes, on the GPU: both convs teacher-forced inside a
per-element bound (tests/precision_regimes.conv_bound: no share cap, every element), the planted tie case bit for bit, and the
fp32 tail behind the bf16 kernel against the float64 tail of the GPU's own d_x6.  tests/test_precision_regimes_host.py holds the
CPU half: the bound between float32 and float64 transforms, the defects it rejects, the planted sets' integer proof, REF_TAIL."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import precision_regimes as pr  # noqa: E402
import torch_ref_precision as tp  # noqa: E402
from vqvdb_amd import weightpack  # noqa: E402
from vqvdb_amd.codec import HipCodec  # noqa: E402

pytestmark = pytest.mark.gpu

# The fp32 path's own distance from the float64 tail per regime: the oracle's d_x7 and voxels on precision_regimes.rows(regime)
# against tail_parts(the oracle's d_x6); tests/test_precision_regimes_host.py recomputes them.
REF_TAIL = {
    "seed0": {"d_x7": {"rms": 2.0852361181877118e-08, "max": 4.287938288882742e-07},
              "voxels": {"rms": 2.6816490653388716e-08, "max": 1.543003623760697e-07}},
    "seed1": {"d_x7": {"rms": 2.0120189839148776e-08, "max": 3.438399356348043e-07},
              "voxels": {"rms": 2.6959642874840142e-08, "max": 1.3534539222703756e-07}},
    "seed2": {"d_x7": {"rms": 1.968222649492235e-08, "max": 3.6533182434794753e-07},
              "voxels": {"rms": 2.7089398876650437e-08, "max": 1.4506327172814082e-07}},
    "trained": {"d_x7": {"rms": 2.8507277806849986e-08, "max": 4.797597998873471e-07},
                "voxels": {"rms": 3.15013464924328e-08, "max": 2.227395659026854e-07}},
    "deadcodes": {"d_x7": {"rms": 2.4986498570644978e-08, "max": 3.4922419489546996e-07},
                  "voxels": {"rms": 3.0718524453009306e-08, "max": 2.5450843998964245e-07}},
    "default": {"d_x7": {"rms": 1.766749206314179e-08, "max": 3.1039115722109045e-07},
                "voxels": {"rms": 2.4236602034907693e-08, "max": 1.0434182146079607e-07}},
}
TAIL_FACTOR = 2.0      # the fp32 tail's own accumulation orders, and other d_x6 values than the constants were measured on


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def staged_decode(w, idx):
    """A bf16-mode decode with debug on by a handle of its own -> (voxels, {d_d2, d_y4, d_x6})."""
    c = HipCodec(weightpack.dumps(w), decode_precision="bf16")
    try:
        c.debug_enable(True)
        rec = c.decode(idx)
        got = {k: c.debug_fetch(k, len(idx), 64, 64) for k in ("d_d2", "d_y4", "d_x6")}
    finally:
        c.close()
    return rec, got


@pytest.fixture(scope="module", params=pr.REGIMES)
def staged(request):
    regime = request.param
    w = pr.weights_of(regime)
    rec, got = staged_decode(w, np.array(pr.rows(regime)))
    for a in (rec, *got.values()):
        a.setflags(write=False)
    return regime, w, rec, got


def test_both_convs_inside_their_per_element_bound(staged):
    """d_y4 from the GPU's own d_d2, d_x6 from the GPU's own d_y4 and d_d2, on 37 rows per regime (a full tile and a half tile
    of 5 leaves; every code; edge leaf 4 included): EVERY element within conv_bound of the restatement.  Printed per tensor: the
    largest err / bound, and the largest err / (2^-24 sum |products|), the accumulation constant the hardware needs where the
    bound allows 1729.  Measured on the MI355X: DESIGN §23."""
    regime, w, _, got = staged
    over = []
    for name, conv, gn, x, skip in (("d_y4", "conv1", "gn1", got["d_d2"], None), ("d_x6", "conv2", "gn2", got["d_y4"], got["d_d2"])):
        ref = tp.conv1(x, w) if skip is None else tp.conv2(x, skip, w)
        bound, parts = pr.conv_bound(x, w, gn, conv, skip=skip, parts=True)
        worst, const, n_over = pr.ratios(got[name], ref, bound, parts["mass"])
        print(f"{regime} {name}: largest err / bound {worst:.4f}, largest err / (2^-24 sum |products|) {const:.2f}, "
              f"{n_over} of {bound.size} elements over their bound")
        if n_over:
            over.append((name, n_over, worst))
    assert not over, f"{regime}: elements outside their bound (tensor, count, largest err / bound): {over}"


def test_tail_behind_the_bf16_kernel(staged):
    """The gate, the folded tail and the sigmoid are the fp32 kernels, fed by csum_combine_k<64> from the bf16 kernel's channel-sum
    partials: the voxels against the float64 tail of the GPU's own d_x6, no farther than TAIL_FACTOR times the fp32 path's own
    distance (REF_TAIL).  d_x7 is never stored by the GPU (the gate is applied inside the tail kernel), so it is held through
    the voxels only; REF_TAIL keeps its fp32 figure for reference."""
    regime, w, rec, got = staged
    _, vox = pr.tail_parts(got["d_x6"], w)
    d = pr.distance(rec, vox)
    ref = REF_TAIL[regime]["voxels"]
    print(f"{regime} voxels vs the float64 tail of the GPU's d_x6: {d}; the fp32 path on the CPU: {ref}")
    assert d["rms"] <= TAIL_FACTOR * ref["rms"] and d["max"] <= TAIL_FACTOR * ref["max"]


@pytest.mark.parametrize("r", range(pr.LIVE_SETS))
def test_planted_ties_bit_for_bit(r):
    """Planted weights (precision_regimes.planted_weights): every operand of both convs is a bf16 tie, a tie's float32 neighbour,
    a negative or a zero, and every output's sum of magnitudes is below 2^24 quanta, so a correct kernel has ONE possible
    result whatever its accumulation order.  No tolerance: d_y4 is the closed form, d_x6 is fl(d_d2 + fl(0.1f v))."""
    w = pr.planted_weights(r)
    idx = np.array(pr.rows("seed0")[:33])
    _, got = staged_decode(w, idx)
    v1, b1 = pr.closed_form(w, "gn1", "conv1")
    v2, b2 = pr.closed_form(w, "gn2", "conv2")
    assert b1 < 2 ** 24 and b2 < 2 ** 24
    for name, have, want in (("d_y4", got["d_y4"], np.broadcast_to(v1, (33, 64, 64))), ("d_x6", got["d_x6"], pr.planted_x6(got["d_d2"], v2))):
        bad = bits(have) != bits(want)
        diff = np.abs(have.astype(np.float64) - want)
        print(f"planted set {r} {name}: {int(bad.sum())} of {bad.size} elements differ; largest difference {diff.max() / pr.QUANTUM:.1f} quanta"
              f" (a bf16 ulp of an operand times the other operand is 128 to 144 quanta)")
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
