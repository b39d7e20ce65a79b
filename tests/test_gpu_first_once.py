"""The encoder's first layer issued once (conv_first_once_k, vq_first_once.h): an 8-leaf group's conv output stays in the accumulators
of one workgroup, which normalises it, stores a1 and emits both GroupNorm statistics.  It must compute the bits of the two-pass
sequence (VQHIP_FIRST=twopass) and of the oracle.

All handles run with set_small_batch_tiles(0): the kernels of full chunks at any batch size.

The statistics pairs (mean, rstd of y1 and of a1) live in two small buffers that the later layers reuse, so no fetch sees them after
a pass; they are pinned through their readers: a1 = relu(gn(y1)) is bit-exact only with y1's pair, and the residual block's first
conv output e_y4 normalises a1 with a1's pair on load."""
import numpy as np
import pytest

from oracle.oracle import DEBUG_SHAPES, ENC_DEBUG
from vqvdb_amd import synth, weightpack
from vqvdb_amd.codec import HipCodec

pytestmark = pytest.mark.gpu

LAYERS = [n for n in ENC_DEBUG if n not in ("e_x12", "e_z")]   # (gated activations and the 128-channel latent are never formed on the GPU)
FIRST_ENV = ("VQHIP_FIRST", "VQHIP_FIRST_SRC")


def _bits(a):
    return np.where(a == 0, 0.0, a).astype(np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pack(weights):
    return weightpack.dumps(weights)


@pytest.fixture(scope="module")
def codec(pack):
    import os
    assert not any(k in os.environ for k in FIRST_ENV), "these tests are about the default first layer"
    c = HipCodec(pack)
    c.set_small_batch_tiles(0)
    yield c
    c.close()


def _batch(n):
    """n = 0: the edge leaves."""
    return synth.edge_leaves() if n == 0 else synth.make_leaves(n, seed=1000 + n)


_ORACLE = {}


def _oracle_of(oracle, n):
    if n not in _ORACLE:
        _ORACLE[n] = oracle.encode(_batch(n), threads=8, debug=ENC_DEBUG)
    return _ORACLE[n]


# 1, 7: a partial 8-leaf group; 8, 9: a group boundary; 31, 32, 33: a partial tile, a tile boundary; 72: more than one tile; 0: edge leaves
@pytest.mark.parametrize("n", [1, 7, 8, 9, 31, 32, 33, 72, 0])
@pytest.mark.parametrize("debug", [False, True])
def test_against_the_oracle_every_intermediate(codec, oracle, n, debug):
    leaves = _batch(n)
    oidx, dbg = _oracle_of(oracle, n)
    codec.debug_enable(debug)
    try:
        idx = codec.encode(leaves)
        if debug:
            for name in LAYERS:
                c, p = DEBUG_SHAPES[name]
                assert np.array_equal(_bits(codec.debug_fetch(name, len(leaves), c, p)), _bits(dbg[name])), name
    finally:
        codec.debug_enable(False)
    assert np.array_equal(idx, oidx)


def test_against_the_two_pass_path(pack, monkeypatch):
    leaves = np.concatenate([synth.make_leaves(300, seed=41), synth.sparse_leaves(100, seed=42), synth.edge_leaves()])
    ref = None
    for first in (None, "twopass", "steps"):
        for k in FIRST_ENV:
            monkeypatch.delenv(k, raising=False)
        if first:
            monkeypatch.setenv("VQHIP_FIRST", first)
        c = HipCodec(pack)
        c.set_small_batch_tiles(0)
        idx = c.encode(leaves)
        c.debug_enable(True)
        idx_dbg = c.encode(leaves)
        got = {name: _bits(c.debug_fetch(name, len(leaves), *DEBUG_SHAPES[name])) for name in LAYERS}
        c.close()
        assert np.array_equal(idx, idx_dbg), first
        if ref is None:
            ref = (idx, got)
            continue
        assert np.array_equal(idx, ref[0]), first
        for name in LAYERS:
            assert np.array_equal(got[name], ref[1][name]), (first, name)


def test_same_call_twice_and_on_a_second_handle_identical_bytes(pack, oracle):
    """More groups than compute units (264 > 256), so some workgroups walk two groups and carry the prefetched rows across."""
    leaves = np.concatenate([synth.make_leaves(2092, seed=77), synth.edge_leaves()])   # 2100 leaves: 66 tiles, the last one partial

    def run(c):
        c.debug_enable(True)
        idx = c.encode(leaves)
        out = [idx] + [c.debug_fetch(name, len(leaves), *DEBUG_SHAPES[name]) for name in ("e_y1", "e_a1")]
        c.debug_enable(False)
        return out + [c.encode(leaves)]

    a = HipCodec(pack)
    a.set_small_batch_tiles(0)
    first, second = run(a), run(a)
    b = HipCodec(pack)
    b.set_small_batch_tiles(0)
    third = run(b)
    a.close()
    b.close()
    for other in (second, third):
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()
    assert np.array_equal(first[0], first[3])   # the same indices without the debug stores
    assert np.array_equal(first[0], oracle.encode(leaves, threads=16))
