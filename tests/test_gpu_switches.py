"""The kernel switches through the real library (run with -m gpu on an MI355X): a value the table of vqvdb_amd/csrc/vq_switches.h
does not list refuses vqhip_create and names its switch; a refused create leaves nothing behind; every switch set to the NAME of its
default gives the handle that no variable gives, bit for bit, on both launch policies and in a training step; and
VQHIP_STEM_SMALL=split — the one spelling that changed, presence alone selected it before — still selects a decoder front that
computes the default's bits.  The parser itself is checked on the host (tests/test_switches_host.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fulltrain_common import fwdbwd, new_codec  # noqa: E402  (imports torch: before the library, as in the other training tests)
from vqvdb_amd import synth, weightpack  # noqa: E402
from vqvdb_amd.codec import HipCodec  # noqa: E402

pytestmark = pytest.mark.gpu

N = 40   # two tiles, the second ragged
# every switch with the name of its default (VQHIP_CUS: the device's count, filled in by the test; VQHIP_COPY_THREADS is process-wide
# and cached at the first host call, so a test does not set it)
DEFAULT_NAMES = {
    "VQHIP_CONV8": "w16", "VQHIP_CONV4": "lds", "VQHIP_DOWN": "lds", "VQHIP_FIRST": "once", "VQHIP_FIRST_SRC": "packed", "VQHIP_STEM": "taps",
    "VQHIP_STEM_SMALL": "fused", "VQHIP_TAIL": "rows16", "VQHIP_TAIL16_TILES": "48", "VQHIP_R64S": "resident", "VQHIP_VQ_SPLIT": "2",
    "VQHIP_HOST_SPLIT": "8,8192", "VQHIP_TRAIN_STEM": "lut", "VQHIP_TRAIN_WGRAD": "rows", "VQHIP_TRAIN_STREAMS": "2", "VQHIP_TRAIN_GNBWD": "fused",
    "VQHIP_TRAIN_BIAS": "deferred", "VQHIP_TRAIN_R64": "quarters", "VQHIP_TRAIN_DGRAD": "streamed", "VQHIP_TRAIN_WGRAD_CU_PCT": "100",
    "VQHIP_TRAIN_RED_OWN_LEAVES": "2048", "VQHIP_TRAIN_EMA_AT": "forward", "VQHIP_TRAIN_EMA": "lists", "VQHIP_TRAIN_TAIL": "folded",
    "VQHIP_TRAIN_SIDE_PRIO": "plain", "VQHIP_TRAIN_RED_QUEUE": "mask", "VQHIP_TRAIN_RED_PRIO": "auto",
}
ALL = tuple(DEFAULT_NAMES) + ("VQHIP_CUS",)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _clean(monkeypatch):
    for k in ALL:
        monkeypatch.delenv(k, raising=False)


def _roundtrip(c, leaves):
    """(indices, voxel bits) with the automatic small-batch policy and with it off (the kernels of full chunks)"""
    out = []
    for tiles in (-1, 0):
        c.set_small_batch_tiles(tiles)
        idx = c.encode(leaves)
        out += [idx, _bits(c.decode(idx))]
    return out


@pytest.fixture(scope="module")
def pack(weights):
    return weightpack.dumps(weights)


@pytest.fixture(scope="module")
def leaves():
    a = np.ascontiguousarray(synth.make_leaves(N, seed=4040))
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def reference(pack, weights, leaves):
    """What handles created with no switch set give: indices and voxel bits on both launch policies, the gradient and the auxiliary
    sums of one training pass, the device's compute units.  Computed once, read-only."""
    with pytest.MonkeyPatch.context() as mp:
        _clean(mp)
        c = HipCodec(pack)
        try:
            device_cus = c.compute_units()[0]
            trip = _roundtrip(c, np.array(leaves))
        finally:
            c.close()
        t = new_codec(weights)
        try:
            g, aux = fwdbwd(t, np.array(leaves))
        finally:
            t.close()
    assert np.isfinite(g).all() and np.abs(g).max() > 0.0
    for a in (*trip, g, aux):
        a.setflags(write=False)
    return trip, g, aux, device_cus


def _same_roundtrip(got, want, label):
    for name, a, b in zip(("indices, small-batch policy", "voxels, small-batch policy", "indices, full-chunk kernels", "voxels, full-chunk kernels"), got, want):
        assert np.array_equal(a, b), f"{label}: {name} differ"


@pytest.mark.parametrize("name,value", [("VQHIP_CONV8", "row"), ("VQHIP_VQ_SPLIT", "two"), ("VQHIP_HOST_SPLIT", "4,31")])
def test_unknown_values_refuse_the_create_and_leave_nothing_behind(pack, leaves, reference, monkeypatch, name, value):
    _clean(monkeypatch)
    monkeypatch.setenv(name, value)
    with pytest.raises(RuntimeError, match=name):
        HipCodec(pack)
    monkeypatch.delenv(name)
    c = HipCodec(pack)
    try:
        _same_roundtrip(_roundtrip(c, np.array(leaves)), reference[0], f"after the refused {name}={value}")
    finally:
        c.close()


def test_every_default_by_name_is_the_default(pack, weights, leaves, reference, monkeypatch):
    trip, g, aux, device_cus = reference
    _clean(monkeypatch)
    for k, v in DEFAULT_NAMES.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VQHIP_CUS", str(device_cus))
    c = HipCodec(pack)
    try:
        assert c.compute_units() == (device_cus, device_cus)
        _same_roundtrip(_roundtrip(c, np.array(leaves)), trip, "every default by name")
    finally:
        c.close()
    t = new_codec(weights)
    try:
        g2, aux2 = fwdbwd(t, np.array(leaves))
    finally:
        t.close()
    print(f"worst gradient difference {float(np.abs(g - g2).max()):.3e} of a largest gradient {float(np.abs(g).max()):.3e}")
    assert np.array_equal(g.view(np.uint32), g2.view(np.uint32))
    assert np.array_equal(aux.view(np.uint32), aux2.view(np.uint32))


def test_stem_small_split_decodes_the_default_bits(pack, leaves, reference, monkeypatch):
    _clean(monkeypatch)
    monkeypatch.setenv("VQHIP_STEM_SMALL", "split")
    c = HipCodec(pack)
    monkeypatch.delenv("VQHIP_STEM_SMALL")
    try:
        c.set_small_batch_tiles(-1)
        assert np.array_equal(_bits(c.decode(np.array(reference[0][0]))), reference[0][1])
    finally:
        c.close()
