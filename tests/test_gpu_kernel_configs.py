"""The two generic conv kernels at the batch sizes where the launch code changes configuration (vq_kernels.h: RowsCfg / Mfma32Cfg;
vq_runtime.hip: launch_rows / launch_mfma32 derive block, grid and dynamic LDS from the configuration).

The sizes come from the selection conditions of the split path in enc_down / enc_res32 / dec_res64 (gh = ceil(2 nt / 8) workgroups of 8 half tiles,
psr = 16 ranges of output rows at these sizes):
  encode  1024 leaves: gh psr 2 = 256, the last size of the cout-split x2 kernels     1056: 288, the position-split kernels
  decode  2048 leaves: gh psr 4 = 1024, the last size of the x4 kernels (LDS-resident quarters, or streamed with VQHIP_R64S=stream)
          2080: 1088, the per-block-partials kernels
  65 leaves with the small-batch policy off and VQHIP_CONV4=rows VQHIP_DOWN=rows: the full-chunk row kernels with a ragged second tile
Every case gives the bits of a default handle with the small-batch policy off on the whole batch, and the oracle's on the first 64 leaves.
The full training step at 64 and 1056 leaves (cout quarters / halves, streamed data gradients) gives the gradient bits of
VQHIP_TRAIN_R64=whole VQHIP_TRAIN_DGRAD=resident (whole layers, LDS-resident data gradients): the K order of every output is the same."""
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

SWITCHES = ("VQHIP_R64S", "VQHIP_CONV4", "VQHIP_DOWN", "VQHIP_TRAIN_R64", "VQHIP_TRAIN_DGRAD")
N_MAX = 2080


def _bits(a):
    return np.where(a == 0, 0.0, a).astype(np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pack(weights):
    return weightpack.dumps(weights)


@pytest.fixture(scope="module")
def reference(pack, oracle):
    """(leaves, indices, voxels) of the 2080-leaf batch from a default handle with the small-batch policy off — per-leaf results, so a
    prefix of them is the result of the prefix — and the oracle's indices and voxels of the first 64 leaves.  Computed once, read-only."""
    leaves = np.ascontiguousarray(np.concatenate([synth.make_leaves(N_MAX - 300 - len(synth.edge_leaves()), seed=77), synth.sparse_leaves(300, seed=78),
                                                  synth.edge_leaves()]))
    assert len(leaves) == N_MAX
    leaves = leaves[np.random.default_rng(79).permutation(N_MAX)]   # every prefix mixes the three kinds
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        c = HipCodec(pack)
        c.set_small_batch_tiles(0)
        idx = c.encode(leaves)
        rec = c.decode(idx)
        c.close()
    oidx = oracle.encode(leaves[:64], threads=16)
    orec = oracle.decode(oidx, threads=16)
    assert np.array_equal(idx[:64], oidx) and np.array_equal(_bits(rec[:64]), _bits(orec))
    for a in (leaves, idx, rec, oidx, orec):
        a.setflags(write=False)
    return leaves, idx, rec, oidx, orec


CASES = [  # (what, leaves, small-batch policy, environment)
    ("encode", 1024, -1, {}), ("encode", 1056, -1, {}),
    ("decode", 2048, -1, {}), ("decode", 2080, -1, {}), ("decode", 2048, -1, {"VQHIP_R64S": "stream"}),
    ("both", 65, 0, {"VQHIP_CONV4": "rows", "VQHIP_DOWN": "rows"}),
]


@pytest.mark.parametrize("what,n,tiles,env", CASES, ids=[f"{w}-{n}" + "".join(f"-{v}" for v in e.values()) for w, n, _, e in CASES])
def test_conv_configurations_at_the_selection_edges(pack, reference, monkeypatch, what, n, tiles, env):
    leaves, ref_idx, ref_rec, oidx, orec = reference
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = HipCodec(pack)
    try:
        c.set_small_batch_tiles(tiles)
        if what in ("encode", "both"):
            idx = c.encode(np.array(leaves[:n]))
            assert np.array_equal(idx, ref_idx[:n])
            assert np.array_equal(idx[:64], oidx)
        if what in ("decode", "both"):
            rec = c.decode(np.array(ref_idx[:n]))
            assert np.array_equal(_bits(rec), _bits(ref_rec[:n]))
            assert np.array_equal(_bits(rec[:64]), _bits(orec))
    finally:
        c.close()


@pytest.mark.parametrize("n", (64, 1056))
def test_training_conv_configurations_give_the_same_gradient_bits(weights, reference, monkeypatch, n):
    leaves = np.array(reference[0][:n])
    out = []
    for env in ({}, {"VQHIP_TRAIN_R64": "whole", "VQHIP_TRAIN_DGRAD": "resident"}):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = new_codec(weights)
        try:
            out.append(fwdbwd(c, leaves))
        finally:
            c.close()
    (g, aux), (g2, aux2) = out
    assert np.isfinite(g).all() and np.abs(g).max() > 0.0
    print(f"{n} leaves: worst gradient difference {float(np.abs(g - g2).max()):.3e} of a largest gradient {float(np.abs(g).max()):.3e}")
    assert np.array_equal(g.view(np.uint32), g2.view(np.uint32))
    assert np.array_equal(aux.view(np.uint32), aux2.view(np.uint32))
