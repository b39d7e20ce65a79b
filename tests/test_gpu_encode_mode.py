"""bf16 encode mode of the scalar handle on the GPU: the default path unchanged, error handling, the two convs
teacher-forced against tests/torch_ref_encode_mode.py on two weight regimes, the fp32 layers behind them against float64, the
planted ties bit for bit, bit invariance over batch size / place / chunk / launch sequence / stream / entry point / compute-unit
count, one handle alternating modes and sizes, the file call, the calls that ignore the mode, the fragments after training, and
the reconstruction error against fp32 mode end to end."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import precision_regimes as pr  # noqa: E402
import torch_ref_encode_mode as te  # noqa: E402
from test_encode_mode_host import GAP, GAP_SHARE, REF_RATIO, REGIMES, inside_cap, stage_leaves  # noqa: E402
from vqvdb_amd import synth, vqvdbfile, weightpack  # noqa: E402
from vqvdb_amd.codec import HipCodec  # noqa: E402

pytestmark = pytest.mark.gpu

ENC = {"e_a1": (16, 512), "e_y4": (16, 512), "e_a6": (16, 512), "e_x7": (32, 64), "e_x11": (32, 64)}


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def encode_debug(c, x, names):
    """(index rows, {name: tensor}) of one encode with the debug layout."""
    c.debug_enable(True)
    try:
        idx = c.encode(x)
        return idx, {k: c.debug_fetch(k, len(x), *ENC[k]) for k in names}
    finally:
        c.debug_enable(False)


@pytest.fixture(scope="module")
def pack(weights):
    return weightpack.dumps(weights)


@pytest.fixture()
def codec(pack):
    c = HipCodec(pack)
    yield c
    c.close()


@pytest.fixture(scope="module")
def leaves97():
    x = te.pair_leaves()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def bf16_97(pack, leaves97):
    """(index rows, e_a6) of the 97 leaves in bf16 mode by a handle of its own: the reference of the invariance tests."""
    c = HipCodec(pack, encode_precision="bf16")
    try:
        idx, dbg = encode_debug(c, leaves97, ("e_a6",))
    finally:
        c.close()
    idx.setflags(write=False), dbg["e_a6"].setflags(write=False)
    return idx, dbg["e_a6"]


def test_default_is_fp32_bit_for_bit_also_after_a_visit_to_bf16(codec, pack, oracle, leaves97):
    names = ("e_y1", "e_a1", "e_y4", "e_a6", "e_x7", "e_y9", "e_x11")
    shapes = dict(ENC, e_y1=(16, 512), e_y9=(32, 64))
    oidx, odbg = oracle.encode(leaves97, threads=8, debug=names)

    def check(c, what):
        c.debug_enable(True)
        try:
            assert np.array_equal(c.encode(leaves97), oidx), what
            for k in names:
                assert np.array_equal(bits(c.debug_fetch(k, 97, *shapes[k])), bits(odbg[k])), (what, k)
        finally:
            c.debug_enable(False)

    assert codec.encode_precision == "fp32" and codec.decode_precision == "fp32"
    check(codec, "fresh handle")
    codec.encode_precision = "bf16"
    assert codec.encode_precision == "bf16" and codec.decode_precision == "fp32"      # the two modes are independent
    _, dbg = encode_debug(codec, leaves97, ("e_y4",))
    assert not np.array_equal(bits(dbg["e_y4"]), bits(odbg["e_y4"]))                  # the mode is real
    codec.decode_precision = "bf16"
    assert codec.encode_precision == "bf16"
    codec.decode_precision = "fp32"
    codec.encode_precision = "fp32"
    assert codec.encode_precision == "fp32"
    check(codec, "after fp32 -> bf16 -> fp32")
    kw = HipCodec(pack, encode_precision="bf16")
    try:
        assert kw.encode_precision == "bf16" and kw.decode_precision == "fp32"
    finally:
        kw.close()


def test_invalid_modes_are_refused_and_leave_the_mode(codec):
    for start in ("fp32", "bf16"):
        codec.encode_precision = start
        for bad in (2, -1):
            assert codec._lib.vqhip_set_encode_mode(codec._h, bad) == -1   # VQHIP_ERR_INVALID
            assert f"mode {bad}" in codec._lib.vqhip_last_error(codec._h).decode()
            assert codec.encode_precision == start
    assert codec._lib.vqhip_get_encode_mode(codec._h, None) == -1
    assert codec._lib.vqhip_get_encode_mode(None, None) == -1
    assert codec._lib.vqhip_set_encode_mode(None, 0) == -1
    with pytest.raises(ValueError, match="encode_precision must be one of"):
        codec.encode_precision = "fp16"


@pytest.mark.parametrize("regime", REGIMES)
def test_both_convs_teacher_forced_and_the_fp32_layers_behind_them(regime):
    """e_y4 from the GPU's own e_a1, e_a6 from the GPU's own e_y4 and e_a1, both inside the flip cap of
    tests/test_encode_mode_host.py on its stage leaves (1e-5 of the tensor's largest value; at most 1e-3 of the elements over it,
    those within 1e-3).  Then from the GPU's e_a6 the float64 rest of the encoder: e_x7 and e_x11 within 1e-5 of their largest
    value, every index the float64 argmin wherever the float64 gap is at least 1e-5, at most 1 % of the positions under it."""
    w = pr.weights_of(regime)
    x = stage_leaves()
    c = HipCodec(weightpack.dumps(w), encode_precision="bf16")
    try:
        idx, got = encode_debug(c, x, tuple(ENC))
    finally:
        c.close()
    ref = {"e_y4": te.conv1(got["e_a1"], w), "e_a6": te.conv2(got["e_y4"], got["e_a1"], w)}
    over = []
    for name in ("e_y4", "e_a6"):
        ok, worst, share = inside_cap(got[name], ref[name])
        print(f"{regime} {name}: max err {worst:.2e} of the largest value, share over 1e-5: {share:.2e}")
        if not ok:
            over.append((name, share, worst))
    assert not over, f"tensors outside the flip cap (name, share over 1e-5, largest error / largest value): {over}"
    am, gap, x7, x11 = te.rest(got["e_a6"], w)
    for name, r in (("e_x7", x7), ("e_x11", x11)):
        rel = float(np.abs(got[name] - r).max() / np.abs(r).max())
        print(f"{regime} {name}: {rel:.2e} of the largest value from the float64 rest")
        assert rel <= 1e-5, name
    under = gap < GAP
    print(f"{regime}: {float(under.mean()):.2e} of the positions under the gap; {int((am != idx).sum())} indices off the float64 argmin")
    assert not ((am != idx) & ~under).any()
    assert float(under.mean()) <= GAP_SHARE


@pytest.mark.parametrize("r", range(te.LIVE_SETS))
def test_planted_ties_bit_for_bit(r):
    """Every sum stays below 2^24 quanta, so a kernel that rounds both operands to nearest even, skips (or zeroes) the padding
    taps and keeps the epilogue's two roundings has one possible result."""
    w = te.planted_weights(r)
    x = np.concatenate([synth.make_leaves(25, seed=400 + r), synth.edge_leaves()])      # 33 leaves: a tile and one more
    c = HipCodec(weightpack.dumps(w), encode_precision="bf16")
    try:
        _, got = encode_debug(c, x, ("e_a1", "e_y4", "e_a6"))
    finally:
        c.close()
    v1, b1 = te.closed_form(w, "gn1", "conv1")
    v2, b2 = te.closed_form(w, "gn2", "conv2")
    assert b1 < 2 ** 24 and b2 < 2 ** 24
    assert np.array_equal(bits(got["e_y4"]), bits(np.broadcast_to(v1[None], got["e_y4"].shape).copy()))
    assert np.array_equal(bits(got["e_a6"]), bits(te.planted_a6(got["e_a1"], v2)))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65])
def test_a_prefix_encoded_alone_has_the_same_bits(pack, leaves97, bf16_97, n):
    """A workgroup serves groups of 8 leaves: either side of every group, half-tile and tile edge up to 65."""
    c = HipCodec(pack, encode_precision="bf16")
    try:
        idx, dbg = encode_debug(c, leaves97[:n], ("e_a6",))
    finally:
        c.close()
    assert np.array_equal(idx, bf16_97[0][:n]) and np.array_equal(bits(dbg["e_a6"]), bits(bf16_97[1][:n]))


def test_same_bits_for_place_chunk_launch_sequence_stream_and_entry_point(pack, leaves97, bf16_97):
    x = np.array(leaves97)
    want_idx, want_a6 = np.asarray(bf16_97[0]), bits(np.asarray(bf16_97[1]))
    c = HipCodec(pack, encode_precision="bf16")
    try:
        idx, dbg = encode_debug(c, np.ascontiguousarray(np.roll(x, 40, axis=0)), ("e_a6",))
        assert np.array_equal(idx, np.roll(want_idx, 40, axis=0)) and np.array_equal(bits(dbg["e_a6"]), np.roll(want_a6, 40, axis=0)), "rotated by 40"
        # encode_device on the null stream and on a second stream
        d_x = torch.from_numpy(x).cuda()
        for stream in (None, torch.cuda.Stream()):
            out = torch.zeros((97, 64), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c.debug_enable(True)
            try:
                c.encode_device(d_x.data_ptr(), 97, out.data_ptr(), stream.cuda_stream if stream else 0)
                torch.cuda.synchronize()
                a6 = c.debug_fetch("e_a6", 97, 16, 512)
            finally:
                c.debug_enable(False)
            assert np.array_equal(out.cpu().numpy(), want_idx) and np.array_equal(bits(a6), want_a6), f"encode_device, stream {stream}"
        # encode_leaves: one buffer per leaf
        assert np.array_equal(c.encode_leaves([x[i] for i in range(97)]), want_idx), "encode_leaves"
        # chunks of 32 leaves
        c.set_chunk_leaves(32)
        assert np.array_equal(c.encode(x), want_idx), "chunk of 32 leaves"
        _, dbg = encode_debug(c, x[64:96], ("e_a6",))
        assert np.array_equal(bits(dbg["e_a6"]), want_a6[64:96]), "a chunk of 32 leaves alone"
    finally:
        c.close()
    # the full-chunk launch sequence instead of the position-split one (the default at this size)
    big = HipCodec(pack, encode_precision="bf16")
    try:
        big.set_small_batch_tiles(0)
        idx, dbg = encode_debug(big, x, ("e_a6",))
        assert np.array_equal(idx, want_idx) and np.array_equal(bits(dbg["e_a6"]), want_a6), "full-chunk launch sequence"
    finally:
        big.close()


@pytest.mark.parametrize("cus", [1, 3])
def test_same_bits_at_other_compute_unit_counts(pack, leaves97, bf16_97, monkeypatch, cus):
    """The bf16 kernel is persistent and takes its grid from the handle's compute-unit count: with 1 and 3 workgroups the 16
    groups of 97 leaves are walked several per workgroup."""
    monkeypatch.setenv("VQHIP_CUS", str(cus))
    c = HipCodec(pack, encode_precision="bf16")
    monkeypatch.delenv("VQHIP_CUS")
    try:
        assert c.compute_units()[1] == cus
        for tiles in (None, 0):      # position-split and full-chunk sequence
            if tiles is not None:
                c.set_small_batch_tiles(tiles)
            idx, dbg = encode_debug(c, leaves97, ("e_a6",))
            assert np.array_equal(idx, bf16_97[0]) and np.array_equal(bits(dbg["e_a6"]), bits(bf16_97[1])), tiles
    finally:
        c.close()


def test_one_handle_alternating_modes_and_sizes(pack, leaves97):
    """fp32 with 33 leaves, bf16 with 97, fp32 with 1, bf16 with 17, bf16 with 65 on ONE handle (the workspace, the statistics
    partials and the fragments are shared between the modes): each result has the bits of a fresh handle in the same mode."""
    c = HipCodec(pack)
    try:
        for mode, n in (("fp32", 33), ("bf16", 97), ("fp32", 1), ("bf16", 17), ("bf16", 65)):
            c.encode_precision = mode
            idx, dbg = encode_debug(c, leaves97[:n], ("e_a6",))
            fresh = HipCodec(pack, encode_precision=mode)
            try:
                widx, wdbg = encode_debug(fresh, leaves97[:n], ("e_a6",))
            finally:
                fresh.close()
            assert np.array_equal(idx, widx) and np.array_equal(bits(dbg["e_a6"]), bits(wdbg["e_a6"])), (mode, n)
    finally:
        c.close()


def test_compress_file_follows_the_mode(codec, leaves97, bf16_97, tmp_path):
    x = np.array(leaves97)
    org = np.arange(97 * 3, dtype=np.int32).reshape(97, 3)
    tr = np.arange(16, dtype=np.float32)
    fp32_idx = codec.encode(x)
    codec.encode_precision = "bf16"
    idx = codec.encode(x)
    assert np.array_equal(idx, bf16_97[0])
    path = tmp_path / "bf16.vqvdb"
    st = codec.compress_file(path, [("a", org[:60], x[:60], None), ("b", org[60:], x[60:], tr)], batch_leaves=7)
    assert st["leaves"] == 97 and st["grids"] == 2
    want = vqvdbfile.dumps([vqvdbfile.Grid("a", org[:60], idx[:60]), vqvdbfile.Grid("b", org[60:], idx[60:], tr)])
    assert path.read_bytes() == want
    if not np.array_equal(idx, fp32_idx):
        assert want != vqvdbfile.dumps([vqvdbfile.Grid("a", org[:60], fp32_idx[:60]), vqvdbfile.Grid("b", org[60:], fp32_idx[60:], tr)])
    grids, dst = codec.decompress_file(path, batch_leaves=32)
    assert dst["leaves"] == 97 and np.array_equal(bits(np.concatenate([g[3] for g in grids])), bits(codec.decode(idx)))


def test_round_trip_and_train_eval_ignore_the_mode(codec, leaves97):
    from vqvdb_amd.codebook_training import STATS_FLOATS
    xd = torch.from_numpy(np.array(leaves97)).cuda()
    rt32 = [t.cpu().numpy() for t in codec.roundtrip(xd, return_recon=True)]
    fp32_idx = codec.encode(np.array(leaves97))
    assert np.array_equal(rt32[0], fp32_idx)
    codec.encode_precision = "bf16"
    for a, b in zip(rt32, [t.cpu().numpy() for t in codec.roundtrip(xd, return_recon=True)]):
        assert np.array_equal(bits(a), bits(b))
    codec.encode_precision = "fp32"
    codec.train_begin()
    got = []
    for mode in ("fp32", "bf16"):
        codec.encode_precision = mode
        stats = torch.zeros(STATS_FLOATS + 3, dtype=torch.float32, device="cuda")
        recon = torch.zeros((64, 512), dtype=torch.float32, device="cuda")
        codec.train_eval_device(xd.data_ptr(), 64, stats.data_ptr(), stats[STATS_FLOATS:].data_ptr(), recon.data_ptr())
        torch.cuda.synchronize()
        got.append((stats.cpu().numpy(), recon.cpu().numpy()))
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(bits(got[0][1]), bits(got[1][1]))


def test_after_a_training_step_the_fragments_follow_the_live_weights(pack, weights, leaves97):
    """bf16 fragments built BEFORE the step; after it a bf16 encode on the live handle has the bits of a fresh bf16 handle built
    from the exported weights."""
    from vqvdb_amd.full_training import FullTrainer
    c = HipCodec(pack, encode_precision="bf16")
    fresh = None
    try:
        before = encode_debug(c, leaves97, ("e_a6",))[1]["e_a6"]
        tr = FullTrainer(c, lr=1e-3)
        tr.step(torch.from_numpy(synth.make_leaves(64, seed=77)).cuda())
        tr.finish()
        sd = tr.state_dict()
        w2 = {k: np.ascontiguousarray(v) for k, v in sd.items() if k in weights}
        assert not np.array_equal(w2["encoder.pre.3.conv1.weight"], weights["encoder.pre.3.conv1.weight"])
        assert c.encode_precision == "bf16"
        idx, live = encode_debug(c, leaves97, ("e_a6",))
        fresh = HipCodec(weightpack.dumps(w2), encode_precision="bf16")
        widx, want = encode_debug(fresh, leaves97, ("e_a6",))
        assert np.array_equal(idx, widx) and np.array_equal(bits(live["e_a6"]), bits(want["e_a6"]))
        assert not np.array_equal(bits(live["e_a6"]), bits(before))
    finally:
        c.close()
        if fresh is not None:
            fresh.close()


def test_reconstruction_error_against_fp32_mode_end_to_end(codec, leaves97, bf16_97):
    """mean ||x - decode(encode(x))||^2 of bf16 mode over fp32 mode, both decoded in fp32, against the same ratio of the CPU
    restatement pair (REF_RATIO of tests/test_encode_mode_host.py).  Allowed distance: four times the spread between the
    restatement's ratios with float32 and float64 transforms, at least 1e-4."""
    x = np.array(leaves97)
    idx32 = codec.encode(x)
    print(f"share of indices equal to fp32 mode: {float((idx32 == bf16_97[0]).mean()):.6f}")
    ratio = te.mse(x, codec.decode(np.asarray(bf16_97[0]))) / te.mse(x, codec.decode(idx32))
    allowed = max(4.0 * abs(REF_RATIO["float32"] - REF_RATIO["float64"]), 1e-4)
    print(f"mse ratio bf16 / fp32: GPU {ratio:.10f}, restatement {REF_RATIO['float32']:.10f}, allowed distance {allowed:.1e}")
    assert abs(ratio - REF_RATIO["float32"]) <= allowed
