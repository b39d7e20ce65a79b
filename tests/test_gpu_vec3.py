"""Vec3 model (VQVAE(3, 64, K)) on the GPU: parity with the reference's fixture and with the fp64 restatement,
determinism across batch, chunk and entry point, buffer bounds, malformed input."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
from torch_ref_vec3 import check_indices_vs_fixture  # noqa: E402
from vqvdb_amd import synth_vec3, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_v1.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def W():
    return synth_vec3.make_weights(0)


@pytest.fixture(scope="module")
def codec(W):
    c = HipVec3Codec(weightpack.dumps(W))
    yield c
    c.close()


@pytest.fixture(scope="module")
def w64(W):
    return tr.weights_to_torch(W, torch.float64)


def fixture_leaves():
    return np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])


def check_vs_fp64(idx, leaves, w64):
    """Chosen code's fp64 distance within 1e-5 * max(|d_min|, |z|^2) of the fp64 minimum."""
    with torch.no_grad():
        z = tr.encoder(leaves, w64)
        dist = tr.distances(z, w64).numpy()
        zz = (z.permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1]) ** 2).sum(1).numpy()
    dmin = dist.min(axis=1)
    got = dist[np.arange(dist.shape[0]), idx.reshape(-1).astype(np.int64)]
    bound = 1e-5 * np.maximum(np.abs(dmin), zz)
    assert (got - dmin <= bound).all(), f"worst excess {float(((got - dmin) / np.maximum(bound, 1e-300)).max()):.2f} x bound"


def test_vec3_model_info(codec):
    assert codec.model_info() == {"num_codes": 4096, "embedding_dim": 64, "latent_shape": [4, 4, 4]}


def test_vec3_fixture_parity_indices_voxels_layers(codec, golden):
    leaves = fixture_leaves()
    idx = codec.encode(leaves)
    n_off, gap = check_indices_vs_fixture(idx, golden)
    print(f"vec3 vs reference: {n_off} of {idx.size} positions off top-1, largest gap at a flip {gap:.2e}")
    rec = codec.decode(np.ascontiguousarray(np.concatenate([golden["idx"][:64], golden["idx"][512:]])))
    assert float(np.abs(rec - golden["rec"]).max()) < 1e-5
    codec.debug_enable(True)
    try:
        codec.encode(leaves[:1])
        codec.decode(np.ascontiguousarray(golden["idx"][:1]))
        for k in golden.files:
            if k.startswith("act_"):
                a = codec.debug_fetch(k[4:], 1)[0]
                ref = golden[k]
                assert float(np.abs(a - ref).max()) <= 1e-5 * float(np.abs(ref).max()), k
    finally:
        codec.debug_enable(False)


def test_vec3_fresh_leaves_against_fp64(codec, w64):
    leaves = np.concatenate([synth_vec3.make_leaves(96, seed=777), synth_vec3.edge_leaves()])
    idx = codec.encode(leaves)
    check_vs_fp64(idx, leaves, w64)
    rng = np.random.default_rng(5)
    fresh = rng.integers(0, 4096, size=(24, 64)).astype(np.uint16)
    rec = codec.decode(fresh)
    with torch.no_grad():
        ref = tr.decode(fresh, w64).numpy()
    assert float(np.abs(rec - ref).max()) < 1e-5
    assert np.abs(rec).max() <= 1.0


def test_vec3_k1000_codebook_pads(W):
    w = dict(W)
    w["quantizer.embedding"] = np.ascontiguousarray(W["quantizer.embedding"][:1000])
    c = HipVec3Codec(weightpack.dumps(w))
    try:
        assert c.model_info()["num_codes"] == 1000
        leaves = np.concatenate([synth_vec3.make_leaves(64, seed=31), synth_vec3.edge_leaves()])
        idx = c.encode(leaves)
        assert idx.max() < 1000
        check_vs_fp64(idx, leaves, tr.weights_to_torch(w, torch.float64))
        rec = c.decode(idx[:8])
        with torch.no_grad():
            ref = tr.decode(idx[:8], tr.weights_to_torch(w, torch.float64)).numpy()
        assert float(np.abs(rec - ref).max()) < 1e-5
        with pytest.raises(RuntimeError, match="out of range"):
            c.decode(np.full((2, 64), 1000, np.uint16))
    finally:
        c.close()


def duplicate_pairs(used):
    """Four (lower, higher) code pairs, each made of a code the encoder chose (`src`) and the row it is copied into:
    inside one 32-code tile on opposite half-waves of vq_k (c and c+4: lanes 0-31 hold rows 0-3, 8-11, ... of a tile,
    lanes 32-63 rows 4-7, ...) with the used code first the lower and then the higher of the two, and across 128-code
    LDS blocks (c and c+128) both ways.  Returns [(src, dst, lower, higher)], all eight codes distinct."""
    used = sorted(set(int(c) for c in used))
    taken, out = set(), []
    rules = [lambda c: c + 4 if c % 8 < 4 else None,            # src in the lanes-0-31 half, dst 4 rows up (other half)
             lambda c: c - 4 if c % 8 >= 4 else None,           # src in the lanes-32-63 half, dst 4 rows down
             lambda c: c + 128 if c + 128 < 4096 else None,     # src lower, dst in the next LDS block
             lambda c: c - 128 if c >= 128 else None]           # src higher, dst in the previous LDS block
    for rule in rules:
        for c in used:
            d = rule(c)
            if d is None or d in used or c in taken or d in taken:
                continue
            taken |= {c, d}
            out.append((c, d, min(c, d), max(c, d)))
            break
    assert len(out) == 4, "not enough codes in use to build the duplicate pairs"
    return out


def test_vec3_duplicate_codes_lower_index_wins(codec, W):
    leaves = synth_vec3.make_leaves(256, seed=3)
    first = codec.encode(leaves)
    pairs = duplicate_pairs(first.reshape(-1))
    w = dict(W)
    e = W["quantizer.embedding"].copy()
    for src, dst, _lo, _hi in pairs:
        e[dst] = e[src]
    w["quantizer.embedding"] = e
    c = HipVec3Codec(weightpack.dumps(w))
    try:
        idx = c.encode(leaves)
    finally:
        c.close()
    for src, dst, lo, hi in pairs:
        # the distances to both rows are bit-identical, and no other row moved closer: every position that chose src now
        # chooses the lower index of the pair, and the higher never occurs
        assert (first == src).any()
        assert (idx[first == src] == lo).all(), (src, dst)
        assert not (idx == hi).any(), (src, dst)


def test_vec3_determinism_batch_chunk_entry_point(codec, W):
    leaves = synth_vec3.make_leaves(4097, seed=99)
    idx = codec.encode(leaves)
    assert np.array_equal(codec.encode(leaves), idx)
    rec = codec.decode(idx)
    assert np.array_equal(codec.decode(idx).view(np.uint32), rec.view(np.uint32))
    for b in (1, 31, 32, 33):
        for off in (0, 7, 4097 - b):
            assert np.array_equal(codec.encode(np.ascontiguousarray(leaves[off:off + b])), idx[off:off + b]), (b, off)
            assert np.array_equal(codec.decode(np.ascontiguousarray(idx[off:off + b])).view(np.uint32), rec[off:off + b].view(np.uint32)), (b, off)
    small = HipVec3Codec(weightpack.dumps(W))
    try:
        for bad in (0, 131073):
            with pytest.raises(RuntimeError, match=r"chunk_leaves must be in \[1, 131072\]"):
                small.set_chunk_leaves(bad)
        small.set_chunk_leaves(131072)
        assert small.chunk_leaves() == 131072
        small.set_chunk_leaves(100)
        assert small.chunk_leaves() == 100
        assert np.array_equal(small.encode(leaves), idx)
        assert np.array_equal(small.decode(idx).view(np.uint32), rec.view(np.uint32))
    finally:
        small.close()
    dl = torch.from_numpy(leaves).cuda()
    di = torch.zeros((4097, 64), dtype=torch.int16, device="cuda")
    do = torch.zeros((4097, 512, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the codec's own stream does not wait for torch's
    codec.encode_device(dl.data_ptr(), 4097, di.data_ptr())
    codec.decode_device(di.data_ptr(), 4097, do.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy().view(np.uint16), idx)
    assert np.array_equal(do.cpu().numpy().view(np.uint32), rec.view(np.uint32))


def test_vec3_canary_tail_untouched_and_zero_leaves(codec):
    n = 37
    leaves = torch.from_numpy(synth_vec3.make_leaves(n, seed=5)).cuda()
    idx = torch.full((n + 64, 64), 0x5A5A, dtype=torch.int16, device="cuda")
    out = torch.full((n + 64, 512, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    codec.encode_device(leaves.data_ptr(), n, idx.data_ptr())
    codec.decode_device(idx.data_ptr(), n, out.data_ptr())
    torch.cuda.synchronize()
    assert (idx[n:] == 0x5A5A).all() and (out[n:] == 7.0).all()
    assert codec.encode(np.zeros((0, 512, 3), np.float32)).shape == (0, 64)
    assert codec.decode(np.zeros((0, 64), np.uint16)).shape == (0, 512, 3)


def test_vec3_malformed_packs_and_indices(codec, W):
    from vqvdb_amd import synth
    with pytest.raises(RuntimeError, match="not a Vec3 model pack"):
        HipVec3Codec(weightpack.dumps(synth.make_weights(0)))
    for emb, msg in ((np.zeros((16, 32), np.float32), "embedding_dim is 32"), (np.zeros((65537, 64), np.float32), "num_codes is 65537")):
        bad = dict(W)
        bad["quantizer.embedding"] = emb
        with pytest.raises(RuntimeError, match=msg):
            HipVec3Codec(weightpack.dumps(bad))
    bad = dict(W)
    bad["decoder.up_conv.weight"] = np.zeros((256, 128, 3, 3, 2), np.float32)
    with pytest.raises(RuntimeError, match="'decoder.up_conv.weight' has unexpected shape"):
        HipVec3Codec(weightpack.dumps(bad))
    idx = np.zeros((3, 64), np.uint16)
    idx[2, 17] = 4096
    with pytest.raises(RuntimeError, match="out of range"):
        codec.decode(idx)


def test_vec3_65536_leaf_round_trip_spans_chunks(W):
    c = HipVec3Codec(weightpack.dumps(W))
    try:
        c.set_chunk_leaves(16384)
        leaves = synth_vec3.make_leaves(256, seed=2024)
        big = np.ascontiguousarray(np.tile(leaves, (256, 1, 1)))
        idx = c.encode(big)
        ref = c.encode(leaves)
        assert np.array_equal(idx, np.tile(ref, (256, 1)))
        rec = c.decode(idx)
        assert np.array_equal(rec[-256:].view(np.uint32), c.decode(ref).view(np.uint32))
    finally:
        c.close()
