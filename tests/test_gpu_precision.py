"""bf16 decode mode of the scalar handle on the GPU: the default path unchanged, error handling, the two convs
teacher-forced against tests/torch_ref_precision.py, bit invariance over batch size / place / chunk / launch path / stream /
entry point, one handle alternating modes and sizes, closeness to fp32 mode end to end, the fragments after training, and the file call."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_precision as tp  # noqa: E402
from vqvdb_amd import synth, vqvdbfile, weightpack  # noqa: E402
from vqvdb_amd.codec import HipCodec  # noqa: E402

pytestmark = pytest.mark.gpu

FLIP_SHARE, FLIP_BOUND = 1e-3, 1e-3
# tests/torch_ref_precision.py (bf16 operands, float64 tail) against the oracle's fp32 decode on the 97 leaves of
# torch_ref_precision.pair_leaves(); tests/test_precision_host.py recomputes them
REF_PAIR = {"rms": 1.8940351446129792e-05, "max": 0.00010723078037733202, "mse_ratio": 0.9999998689462706}


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def pack(weights):
    return weightpack.dumps(weights)


@pytest.fixture()
def codec(pack):
    c = HipCodec(pack)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pair(oracle):
    """(the 97 leaves, their index rows, the oracle's fp32 decode of those rows): computed once, never written to."""
    x = tp.pair_leaves()
    idx = oracle.encode(x, threads=8)
    rec = oracle.decode(idx, threads=8)
    for a in (x, idx, rec):
        a.setflags(write=False)
    return x, idx, rec


@pytest.fixture(scope="module")
def bf16_97(pack, pair):
    """The bf16-mode decode of the 97 rows by a handle of its own, the reference of the invariance tests."""
    c = HipCodec(pack, decode_precision="bf16")
    try:
        out = c.decode(pair[1])
    finally:
        c.close()
    out.setflags(write=False)
    return out


def test_default_is_fp32_and_the_mode_touches_only_the_plain_decode(codec, pack, pair):
    x, idx, orec = pair
    assert codec.decode_precision == "fp32"
    rec = codec.decode(idx)
    assert np.array_equal(bits(rec), bits(orec))
    xh = np.array(x)   # (a writable copy: torch wraps no read-only arrays)
    xd = torch.from_numpy(xh).cuda()
    host32 = codec.roundtrip(xh, return_recon=True)
    dev32 = [t.cpu().numpy() for t in codec.roundtrip(xd, return_recon=True)]
    assert np.array_equal(bits(host32[2]), bits(rec))
    codec.decode_precision = "bf16"
    assert codec.decode_precision == "bf16"
    assert not np.array_equal(bits(codec.decode(idx)), bits(rec))       # the mode is real
    # the round trip states its error against the fp32 reconstruction: indices, errors and reconstruction have the same bits in
    # either mode, host form and device form
    for a, b in zip(host32, codec.roundtrip(xh, return_recon=True)):
        assert np.array_equal(bits(a), bits(b))
    for a, b in zip(dev32, [t.cpu().numpy() for t in codec.roundtrip(xd, return_recon=True)]):
        assert np.array_equal(bits(a), bits(b))
    codec.decode_precision = "fp32"
    assert codec.decode_precision == "fp32"
    assert np.array_equal(bits(codec.decode(idx)), bits(rec))
    kw = HipCodec(pack, decode_precision="bf16")
    try:
        assert kw.decode_precision == "bf16"
    finally:
        kw.close()


def test_train_eval_ignores_the_mode(codec, pair):
    from vqvdb_amd.codebook_training import STATS_FLOATS
    x = torch.from_numpy(np.array(pair[0][:64])).cuda()
    codec.train_begin()
    got = []
    for mode in ("fp32", "bf16"):
        codec.decode_precision = mode
        stats = torch.zeros(STATS_FLOATS + 3, dtype=torch.float32, device="cuda")
        recon = torch.zeros((64, 512), dtype=torch.float32, device="cuda")
        codec.train_eval_device(x.data_ptr(), 64, stats.data_ptr(), stats[STATS_FLOATS:].data_ptr(), recon.data_ptr())
        torch.cuda.synchronize()
        got.append((stats.cpu().numpy(), recon.cpu().numpy()))
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(bits(got[0][1]), bits(got[1][1]))


def test_invalid_modes_are_refused_and_leave_the_mode(codec):
    for start in ("fp32", "bf16"):
        codec.decode_precision = start
        for bad in (2, -1):
            assert codec._lib.vqhip_set_decode_mode(codec._h, bad) == -1   # VQHIP_ERR_INVALID
            assert f"mode {bad}" in codec._lib.vqhip_last_error(codec._h).decode()
            assert codec.decode_precision == start
    assert codec._lib.vqhip_get_decode_mode(codec._h, None) == -1
    assert codec._lib.vqhip_set_decode_mode(None, 0) == -1
    with pytest.raises(ValueError, match="decode_precision must be one of"):
        codec.decode_precision = "fp16"


def test_both_convs_teacher_forced_against_the_bf16_restatement(codec, weights, golden):
    """d_y4 from the GPU's own d_d2, d_x6 from the GPU's own d_y4 and d_d2.  Bar: 1e-5 of the tensor's largest value; at most
    FLIP_SHARE of the elements may exceed it (an activation within an ulp of a bf16 rounding boundary), and those stay within
    FLIP_BOUND of the largest value.  Measured on the MI355X: d_y4 3.75e-7, d_x6 4.27e-8 of the largest value, no element
    over 1e-5."""
    from test_precision_host import stage_rows
    idx = stage_rows(golden)
    n = len(idx)
    assert n == 33
    codec.decode_precision = "bf16"
    codec.debug_enable(True)
    try:
        codec.decode(idx)
        got = {k: codec.debug_fetch(k, n, 64, 64) for k in ("d_d2", "d_y4", "d_x6")}
    finally:
        codec.debug_enable(False)
    ref = {"d_y4": tp.conv1(got["d_d2"], weights), "d_x6": tp.conv2(got["d_y4"], got["d_d2"], weights)}
    over = []
    for name in ("d_y4", "d_x6"):
        err = np.abs(got[name].astype(np.float64) - ref[name])
        top = float(np.abs(ref[name]).max())
        share = float((err > 1e-5 * top).mean())
        print(f"{name}: max err {err.max() / top:.2e} of the largest value, share over 1e-5: {share:.2e}")
        if share > FLIP_SHARE or float(err.max()) > FLIP_BOUND * top:
            over.append((name, share, float(err.max()) / top))
    assert not over, f"tensors outside the flip cap (name, share over 1e-5, largest error / largest value): {over}"


@pytest.mark.parametrize("n", [1, 17, 33, 15, 16, 31, 32, 48, 49, 64, 65])
def test_a_prefix_decoded_alone_has_the_same_bits(pack, pair, bf16_97, n):
    """A workgroup serves a half tile of 16 leaves (grid = 2 * n_tiles): either side of every half-tile and tile edge up to 65."""
    c = HipCodec(pack, decode_precision="bf16")
    try:
        assert np.array_equal(bits(c.decode(pair[1][:n])), bits(bf16_97[:n]))
    finally:
        c.close()


def test_one_handle_alternating_modes_and_sizes(pack, pair):
    """fp32 with 33 leaves, bf16 with 97, fp32 with 1, bf16 with 17, bf16 with 65 on ONE handle (the workspace, the statistics
    partials and the fragments are shared between the modes): each result has the bits of a fresh handle in the same mode."""
    idx = pair[1]
    c = HipCodec(pack)
    try:
        for mode, n in (("fp32", 33), ("bf16", 97), ("fp32", 1), ("bf16", 17), ("bf16", 65)):
            c.decode_precision = mode
            got = c.decode(idx[:n])
            fresh = HipCodec(pack, decode_precision=mode)
            try:
                want = fresh.decode(idx[:n])
            finally:
                fresh.close()
            assert np.array_equal(bits(got), bits(want)), (mode, n)
    finally:
        c.close()


def test_same_bits_for_place_chunk_launch_path_stream_and_entry_point(pack, pair, bf16_97, tmp_path):
    idx = np.array(pair[1])
    want = bits(np.asarray(bf16_97))
    c = HipCodec(pack, decode_precision="bf16")
    try:
        rot = np.ascontiguousarray(np.roll(idx, 40, axis=0))
        assert np.array_equal(bits(c.decode(rot)), np.roll(want, 40, axis=0)), "rotated by 40"
        # decode_device on the null stream and on a second stream
        d_idx = torch.from_numpy(idx).cuda()
        for stream in (None, torch.cuda.Stream()):
            out = torch.zeros((97, 512), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            c.decode_device(d_idx.data_ptr(), 97, out.data_ptr(), stream.cuda_stream if stream else 0)
            torch.cuda.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), want), f"decode_device, stream {stream}"
        # decode_leaves: one buffer per leaf
        pool = np.zeros((97, 512), dtype=np.float32)
        c.decode_leaves(idx, [pool[i] for i in range(97)])
        assert np.array_equal(bits(pool), want), "decode_leaves"
        # pieces of 7 leaves: the chunk setter's floor is 32, the file call's batch_leaves goes below it
        path = tmp_path / "rows97.vqvdb"
        org = np.arange(97 * 3, dtype=np.int32).reshape(97, 3)
        vqvdbfile.save(path, [vqvdbfile.Grid("g", org, idx)])
        grids, st = c.decompress_file(path, batch_leaves=7)
        assert st["leaves"] == 97 and np.array_equal(bits(grids[0][3]), want), "pieces of 7 leaves"
        # chunks of 32 leaves
        c.set_chunk_leaves(32)
        assert np.array_equal(bits(c.decode(idx)), want), "chunk of 32 leaves"
    finally:
        c.close()
    # the full-chunk launch sequence instead of the position-split one (the default at this size)
    big = HipCodec(pack, decode_precision="bf16")
    try:
        big.set_small_batch_tiles(0)
        assert np.array_equal(bits(big.decode(idx)), want), "full-chunk launch sequence"
    finally:
        big.close()


def test_close_to_fp32_mode_end_to_end(codec, pair, bf16_97):
    x, idx, _ = pair
    got = tp.closeness(bf16_97, codec.decode(idx), x)
    print(f"GPU bf16 vs GPU fp32: {got}; restatement pair: {REF_PAIR}")
    assert got["rms"] <= 1.5 * REF_PAIR["rms"] and got["max"] <= 1.5 * REF_PAIR["max"]
    assert got["mse_ratio"] <= REF_PAIR["mse_ratio"] + 0.02


def test_after_a_training_step_the_fragments_follow_the_live_weights(pack, weights, pair):
    """bf16 fragments built BEFORE the step; after it a bf16 decode on the live handle has the bits of a fresh bf16 handle built
    from the exported weights."""
    from vqvdb_amd.full_training import FullTrainer
    idx = pair[1]
    c = HipCodec(pack, decode_precision="bf16")
    fresh = None
    try:
        before = c.decode(idx)
        tr = FullTrainer(c, lr=1e-3)
        tr.step(torch.from_numpy(synth.make_leaves(64, seed=77)).cuda())
        tr.finish()
        sd = tr.state_dict()
        w2 = {k: np.ascontiguousarray(v) for k, v in sd.items() if k in weights}
        assert not np.array_equal(w2["decoder.res_stack.0.conv1.weight"], weights["decoder.res_stack.0.conv1.weight"])
        live = c.decode(idx)
        fresh = HipCodec(weightpack.dumps(w2), decode_precision="bf16")
        assert c.decode_precision == "bf16"
        assert np.array_equal(bits(live), bits(fresh.decode(idx)))
        assert not np.array_equal(bits(live), bits(before))
    finally:
        c.close()
        if fresh is not None:
            fresh.close()


def test_decompress_file_follows_the_mode(codec):
    path = os.path.join(ROOT, "tests", "golden", "ref_writer_v3.vqvdb")
    want = vqvdbfile.load(path)
    fp32 = [codec.decode(g.indices) for g in want]
    codec.decode_precision = "bf16"
    grids, st = codec.decompress_file(path, batch_leaves=97)
    assert st["leaves"] == 1000 and st["grids"] == 2
    for (name, _tr, org, leaves), g, f in zip(grids, want, fp32):
        assert name == g.name and np.array_equal(org, g.origins)
        assert np.array_equal(bits(leaves), bits(codec.decode(g.indices)))
        assert not np.array_equal(bits(leaves), bits(f))
