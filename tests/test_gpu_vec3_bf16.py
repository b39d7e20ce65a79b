"""bf16-operand inference mode of the Vec3 handle on the GPU: the default path unchanged, error handling,
every debug-fetch layer teacher-forced against tests/torch_ref_vec3_bf16.py, the codebook search criterion on the new latent,
bit invariance, closeness to fp32 mode end to end, and the interplay with full training."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
import torch_ref_vec3_bf16 as tb  # noqa: E402
from torch_ref_vec3 import check_indices_vs_fixture  # noqa: E402
from vqvdb_amd import synth_vec3, vec3_full_training, weightpack  # noqa: E402
from vqvdb_amd.codec import VEC3_DEBUG_LAYERS, HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_v1.npz")
# leaf 0 and 31 further fixture leaves; tests/test_vec3_bf16_host.py checks the flip cap on them (fixture leaves 8 and 14 are
# left out: there the restatement with float64 transforms already leaves the cap)
STAGE_IDS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33]
STAGE_LEAVES = len(STAGE_IDS)
FLIP_SHARE, FLIP_BOUND = 1e-3, 1e-3
# torch_ref_vec3_bf16 against torch_ref_vec3 (float64 weights) on the 520 fixture leaves: `python tools/vec3_bf16_pair.py`
REF_PAIR = {"index_share": 0.008353365384615384, "rms": 0.026919963339083922, "max": 0.4132680405407192, "mse_ratio": 1.0000118428673792}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def W():
    return synth_vec3.make_weights(0)


@pytest.fixture(scope="module")
def w64(W):
    return tr.weights_to_torch(W, torch.float64)


@pytest.fixture(scope="module")
def leaves():
    return np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])


@pytest.fixture()
def codec(W):
    c = HipVec3Codec(weightpack.dumps(W))
    yield c
    c.close()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_default_is_fp32_and_unchanged_by_a_round_trip_of_the_mode(codec, W, golden, leaves):
    assert codec.precision == "fp32"
    idx = codec.encode(leaves)
    dec_in = np.ascontiguousarray(np.concatenate([golden["idx"][:64], golden["idx"][512:]]))
    rec = codec.decode(dec_in)
    check_indices_vs_fixture(idx, golden)
    assert float(np.abs(rec - golden["rec"]).max()) < 1e-5
    codec.precision = "bf16"
    assert codec.precision == "bf16"
    codec.encode(leaves[:8])
    codec.precision = "fp32"
    assert codec.precision == "fp32"
    assert np.array_equal(codec.encode(leaves), idx)
    assert np.array_equal(bits(codec.decode(dec_in)), bits(rec))
    kw = HipVec3Codec(weightpack.dumps(W), precision="bf16")
    try:
        assert kw.precision == "bf16"
    finally:
        kw.close()


def test_invalid_modes_are_refused_and_leave_the_mode(codec):
    for start in ("fp32", "bf16"):
        codec.precision = start
        for bad in (2, -1):
            rc = codec._lib.vqhip_vec3_set_precision(codec._h, bad)
            assert rc == -1   # VQHIP_ERR_INVALID
            assert f"mode {bad}" in codec._lib.vqhip_vec3_last_error(codec._h).decode()
            assert codec.precision == start
    assert codec._lib.vqhip_vec3_get_precision(codec._h, None) == -1
    assert codec._lib.vqhip_vec3_set_precision(None, 0) == -1
    with pytest.raises(ValueError, match="precision must be one of"):
        codec.precision = "fp16"


def test_every_layer_teacher_forced_against_the_bf16_restatement(codec, w64, leaves):
    """Each debug-fetch layer from the GPU's own previous fetch point.  Bar: 1e-5 of the tensor's largest value; at most
    FLIP_SHARE of a tensor's elements may exceed it (an activation within an ulp of a bf16 rounding boundary), and those stay
    within FLIP_BOUND of the largest value.

    Measured on the MI355X (STAGE_IDS): no element of any of the twelve layers is over 1e-5; the largest error is between 0
    (encoder.pre.2 and decoder.stem, bit-identical) and 9.3e-6 (encoder.pre) of the tensor's largest value.  The restatement must give
    the GroupNorm statistics and gates of the kernels to the last bit for that (torch_ref_vec3_bf16.gn_stats, gates): with an
    rstd one float32 ulp off, whole groups of activations round the other way and two layers leave the cap; DESIGN §14."""
    x = np.ascontiguousarray(leaves[STAGE_IDS])
    codec.precision = "bf16"
    codec.debug_enable(True)
    try:
        idx = codec.encode(x)
        codec.decode(idx)
        got = {k: codec.debug_fetch(k, STAGE_LEAVES) for k in VEC3_DEBUG_LAYERS}
    finally:
        codec.debug_enable(False)
    assert list(tb.STAGES) == list(VEC3_DEBUG_LAYERS)
    with torch.no_grad():
        got["leaves"] = x
        got["codes"] = tb.codes(idx, w64).reshape(STAGE_LEAVES, 64, 64).numpy()
    worst_share, over = 0.0, []
    for name, (prev, _fn) in tb.STAGES.items():
        ref = tb.stage(name, got[prev], w64).numpy()
        err = np.abs(got[name].astype(np.float64) - ref)
        top = float(np.abs(ref).max())
        share = float((err > 1e-5 * top).mean())
        worst_share = max(worst_share, share)
        print(f"{name}: max err {err.max() / top:.2e} of the largest value, share over 1e-5: {share:.2e}")
        if share > FLIP_SHARE or float(err.max()) > FLIP_BOUND * top:
            over.append((name, share, float(err.max()) / top))
    print(f"largest share of elements over 1e-5: {worst_share:.2e}")
    assert not over, f"layers outside the flip cap (name, share over 1e-5, largest error / largest value): {over}"


def test_search_criterion_on_the_bf16_latent(codec, w64, leaves):
    x = np.ascontiguousarray(np.concatenate([leaves[:96], leaves[512:]]))
    codec.precision = "bf16"
    codec.debug_enable(True)
    try:
        idx = codec.encode(x)
        z = torch.from_numpy(codec.debug_fetch("encoder.proj", len(x))).double().reshape(-1, 64, 4, 4, 4)
    finally:
        codec.debug_enable(False)
    with torch.no_grad():
        dist = tr.distances(z, w64).numpy()
        zz = (z.permute(0, 2, 3, 4, 1).reshape(-1, 64) ** 2).sum(1).numpy()
    dmin = dist.min(axis=1)
    got = dist[np.arange(dist.shape[0]), idx.reshape(-1).astype(np.int64)]
    assert (got - dmin <= 1e-5 * np.maximum(np.abs(dmin), zz)).all()


def test_duplicate_codebook_rows_go_to_the_lower_index_in_bf16_mode(codec, W, leaves):
    x = np.ascontiguousarray(leaves[:128])
    codec.precision = "bf16"
    first = codec.encode(x)
    src = int(np.bincount(first.reshape(-1)).argmax())
    dst = src + 128 if src + 128 < 4096 else src - 128
    w = dict(W)
    e = W["quantizer.embedding"].copy()
    e[dst] = e[src]
    w["quantizer.embedding"] = e
    c = HipVec3Codec(weightpack.dumps(w), precision="bf16")
    try:
        idx = c.encode(x)
    finally:
        c.close()
    assert (idx[first == src] == min(src, dst)).all() and not (idx == max(src, dst)).any()


def test_bits_do_not_depend_on_batch_place_chunk_entry_point_or_stream(codec, W, leaves):
    codec.precision = "bf16"
    idx = codec.encode(leaves)
    rec = codec.decode(idx)
    assert np.array_equal(codec.encode(leaves), idx) and np.array_equal(bits(codec.decode(idx)), bits(rec))
    for n in (1, 33):
        assert np.array_equal(codec.encode(np.ascontiguousarray(leaves[:n])), idx[:n]), n
        assert np.array_equal(bits(codec.decode(np.ascontiguousarray(idx[:n]))), bits(rec[:n])), n
    moved = np.ascontiguousarray(np.concatenate([leaves[100:], leaves[:100]]))       # every leaf at another place in the batch
    assert np.array_equal(codec.encode(moved), np.concatenate([idx[100:], idx[:100]]))
    assert np.array_equal(bits(codec.decode(np.ascontiguousarray(np.concatenate([idx[100:], idx[:100]])))), bits(np.concatenate([rec[100:], rec[:100]])))
    small = HipVec3Codec(weightpack.dumps(W), precision="bf16")
    try:
        small.set_chunk_leaves(7)
        assert np.array_equal(small.encode(leaves), idx)
        assert np.array_equal(bits(small.decode(idx)), bits(rec))
    finally:
        small.close()
    n = len(leaves)
    dl = torch.from_numpy(leaves).cuda()
    for stream in (None, torch.cuda.Stream()):
        di = torch.zeros((n, 64), dtype=torch.int16, device="cuda")
        do = torch.zeros((n, 512, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        h = stream.cuda_stream if stream is not None else 0
        codec.encode_device(dl.data_ptr(), n, di.data_ptr(), h)
        codec.decode_device(di.data_ptr(), n, do.data_ptr(), h)
        torch.cuda.synchronize()
        assert np.array_equal(di.cpu().numpy().view(np.uint16), idx)
        assert np.array_equal(bits(do.cpu().numpy()), bits(rec))


def test_closeness_to_fp32_mode_end_to_end(codec, W, leaves):
    """The GPU's bf16 mode against its fp32 mode on the 520 fixture leaves, next to the same four quantities of the two
    torch restatements (REF_PAIR).  The fixture model is untrained: many codes are near-ties, so a large share of indices
    moves; the reconstruction error is what a user sees."""
    fp = HipVec3Codec(weightpack.dumps(W))
    try:
        codec.precision = "bf16"
        g = tb.closeness(leaves, None, codec.encode, codec.decode, fp.encode, fp.decode)
    finally:
        fp.close()
    print(f"GPU bf16 vs fp32: {g}")
    print(f"restatements:     {REF_PAIR}")
    for k in ("index_share", "rms", "max"):
        assert g[k] <= 1.5 * REF_PAIR[k], k
    assert g["mse_ratio"] <= REF_PAIR["mse_ratio"] + 0.02


def test_training_ignores_the_mode_and_rebuilds_the_bf16_tables(W, leaves):
    x = torch.from_numpy(np.ascontiguousarray(leaves[:64])).cuda()
    torch.cuda.synchronize()
    params, state = {}, {}
    handles = {}
    try:
        for mode in ("fp32", "bf16"):
            c = handles[mode] = HipVec3Codec(weightpack.dumps(W), precision=mode)
            t = vec3_full_training.Vec3FullTrainer(c, lr=1e-3)
            for _ in range(3):
                t.step(x, n_global=64)
            torch.cuda.synchronize()
            assert c.precision == mode
            params[mode] = c.fulltrain_get_params()
            state[mode] = t.state_dict()
        assert np.array_equal(bits(params["fp32"]), bits(params["bf16"]))
        live = handles["bf16"]
        idx = live.encode(leaves[:64])
        rec = live.decode(idx)
        pack = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in state["bf16"].items() if k in W}
        fresh = HipVec3Codec(weightpack.dumps({k: pack[k] for k in W}), precision="bf16")
        try:
            assert np.array_equal(fresh.encode(leaves[:64]), idx)
            assert np.array_equal(bits(fresh.decode(idx)), bits(rec))
        finally:
            fresh.close()
        # and the live tables did move: the untrained handle decodes these indices differently
        base = HipVec3Codec(weightpack.dumps(W), precision="bf16")
        try:
            assert not np.array_equal(bits(base.decode(idx)), bits(rec))
        finally:
            base.close()
    finally:
        for c in handles.values():
            c.close()
