"""Vec3 model on the GPU off the seed-0 weight draw (tests/vec3_regimes.py): six weight regimes regenerated from numpy and one
trained on the GPU by the project's own trainer, and codebook sizes from 1 to 65 536 with codes planted on the borders of
vq_k's 128-code LDS blocks.  Every bar is tied to what the float32 torch restatement itself achieves against float64
(tests/test_vec3_regimes_host.py shows each bar met by that restatement and violated by three wrong ones), so a failure
here is the kernels'.  fp32 mode against the reference's fixture and float64; bf16 mode against its own restatement, teacher
forced; the fused round trip and both bounded pairs in the two regimes that stretch the value range."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
import torch_ref_vec3_bf16 as tb  # noqa: E402
import vec3_regimes as vr  # noqa: E402
from test_gpu_vec3 import check_vs_fp64, duplicate_pairs  # noqa: E402
from test_gpu_vec3_bf16 import FLIP_BOUND, FLIP_SHARE  # noqa: E402
from torch_ref_vec3 import check_indices_vs_fixture  # noqa: E402
from vqvdb_amd import synth_vec3, vec3_full_training, weightpack  # noqa: E402
from vqvdb_amd.codec import VEC3_DEBUG_LAYERS, HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_REGIMES = ("trained",) + vr.REGIMES
MODES = ("fp32", "bf16")
# the `trained` regime: TRAIN_STEPS AdamW + EMA steps at a constant learning rate from seed 0, 64 fresh leaves per step
TRAIN_STEPS, TRAIN_LR, TRAIN_BATCH, TRAIN_SEED = 40, 5e-4, 64, 8800
STAGE_LEAVES = 8   # leaves of the teacher-forced bf16 check


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def train_on_the_gpu(W, tmp):
    """-> (weights of the exported pack, path of the pack, {tensor: largest move / largest initial value})."""
    c = HipVec3Codec(weightpack.dumps(W))
    try:
        c.fulltrain_begin()
        g = torch.zeros(c.fulltrain_param_count(), dtype=torch.float32, device="cuda")
        a = torch.zeros(c.fulltrain_aux_floats(), dtype=torch.float32, device="cuda")
        for s in range(TRAIN_STEPS):
            x = torch.from_numpy(synth_vec3.make_leaves(TRAIN_BATCH, seed=TRAIN_SEED + s)).cuda()
            torch.cuda.synchronize()
            c.fulltrain_fwdbwd_device(x.data_ptr(), TRAIN_BATCH, TRAIN_BATCH, g.data_ptr(), a.data_ptr())
            c.fulltrain_apply_device(g.data_ptr(), a.data_ptr(), TRAIN_LR, s + 1)
            torch.cuda.synchronize()
        params, state = c.fulltrain_get_params(), c.train_get_state()
    finally:
        c.close()
    base, out = str(tmp / "seed0.vqw"), str(tmp / "trained.vqw")
    weightpack.save(base, W)
    vec3_full_training.export_pack(base, {**vec3_full_training.vec_to_state(params), **{f"quantizer.{k}": v for k, v in state.items()}}, out)
    trained = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weightpack.load(out).items() if k in W}
    moves = {k: float(np.abs(trained[k] - W[k]).max() / np.abs(W[k]).max()) for k in W}
    return trained, out, moves


@pytest.fixture(scope="module")
def seed0():
    return synth_vec3.make_weights(0)


@pytest.fixture(scope="module")
def file_free():
    return vr.regimes()


@pytest.fixture(scope="module")
def fixture():
    return vr.load_fixture()


@pytest.fixture(scope="module")
def leaves():
    return vr.fresh_leaves()


@pytest.fixture(scope="module")
def seed0_indices(seed0, leaves):
    c = HipVec3Codec(weightpack.dumps(seed0))
    try:
        return c.encode(leaves)
    finally:
        c.close()


@pytest.fixture(scope="module", params=ALL_REGIMES)
def regime(request, seed0, file_free, fixture, leaves, tmp_path_factory):
    """One fp32 and one bf16 handle per regime, its weights as float32 / float64 torch tensors and the fp32 handle's indices."""
    name = request.param
    r = {"name": name, "fixture": fixture.get(name)}
    if name == "trained":
        r["w"], pack, r["moves"] = train_on_the_gpu(seed0, tmp_path_factory.mktemp("trained"))
        r["codec"], r["bf16"] = HipVec3Codec(pack), HipVec3Codec(pack, precision="bf16")   # fresh handles on the exported pack
    else:
        r["w"] = file_free[name]
        pack = weightpack.dumps(r["w"])
        r["codec"], r["bf16"] = HipVec3Codec(pack), HipVec3Codec(pack, precision="bf16")
    r["w32"], r["w64"] = tr.weights_to_torch(r["w"], torch.float32), tr.weights_to_torch(r["w"], torch.float64)
    r["idx"] = r["codec"].encode(leaves)
    yield r
    r["codec"].close()
    r["bf16"].close()


def fixture_part(a):
    """Rows of the fixture's 32 leaves in an array over fresh_leaves()."""
    return np.ascontiguousarray(np.concatenate([a[:vr.FIXTURE_LEAVES], a[vr.FRESH_LEAVES:]]))


# ---- fp32 mode --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["trained"], indirect=True)
def test_trained_regime_moved_and_stayed_finite(regime):
    """TRAIN_LR = 5e-4 (the trainer's default), constant over 40 steps of 64 leaves.  Measured on the MI355X: every tensor
    finite; 15 of the 16 conv tensors moved by >= 10 % of their largest initial value, the largest encoder.res_stack.0.conv1.weight
    by 61 %, the smallest by 8.8 %; the codebook moved by 2.5 x its largest value and 260 codes stay in use."""
    w, moves = regime["w"], regime["moves"]
    assert all(np.isfinite(v).all() for v in w.values())
    conv = {k: m for k, m in moves.items() if k.endswith(".weight") and w[k].ndim == 5}
    top = max(conv, key=conv.get)
    print(f"trained: lr {TRAIN_LR}, {TRAIN_STEPS} steps of {TRAIN_BATCH} leaves; largest conv move {top} {conv[top]:.3f} of its largest value, "
          f"smallest conv move {min(conv.values()):.3f}, codebook {moves['quantizer.embedding']:.3f}; "
          f"{sum(m >= 0.1 for m in conv.values())} of {len(conv)} conv tensors moved by >= 10 %")
    assert conv[top] >= 0.1


def test_fp32_indices_against_the_fixture_and_fp64(regime, leaves, seed0_indices):
    idx = regime["idx"]
    assert idx.dtype == np.uint16 and idx.shape == (len(leaves), 64)
    if regime["fixture"] is not None:
        n_off, gap = check_indices_vs_fixture(fixture_part(idx), regime["fixture"])
        print(f"{regime['name']}: {n_off} of {32 * 64} positions off the fixture's top-1, largest gap at a flip {gap:.2e}")
    check_vs_fp64(idx, leaves, regime["w64"])
    print(f"{regime['name']}: {len(np.unique(idx))} codes in use")
    if regime["name"] == "wide":      # proj and codebook x 8, a power of two: every distance is exactly 64 x seed 0's
        assert np.array_equal(idx, seed0_indices)


def test_fp32_decode_against_fp64_at_the_restatement_s_own_distance(regime):
    first = regime["fixture"]["idx"] if regime["fixture"] is not None else fixture_part(regime["idx"])
    dec = vr.decode_indices(first, 4096)
    rec = regime["codec"].decode(dec)
    rec32, rec64 = vr.decode_refs(dec, regime["w32"], regime["w64"])
    d, d_ref = vr.check_voxels(rec, rec32, rec64)
    print(f"{regime['name']}: voxels {d:.2e} from fp64, fp32 restatement d_ref {d_ref:.2e}, largest |rec| {float(np.abs(rec).max()):.8f}")
    if regime["fixture"] is not None:
        assert float(np.abs(rec[:32] - regime["fixture"]["rec"]).max()) <= max(1e-5, 2.0 * d_ref)
    if regime["name"] == "saturated":
        assert float(np.abs(rec).max()) == 1.0


def test_fp32_all_twelve_layers_against_fp64(regime, leaves):
    c = regime["codec"]
    x = np.ascontiguousarray(leaves[list(vr.LAYER_LEAVES)])
    c.debug_enable(True)
    try:
        idx = c.encode(x)
        c.decode(idx)
        got = {k: c.debug_fetch(k, len(x)) for k in VEC3_DEBUG_LAYERS}
    finally:
        c.debug_enable(False)
    assert np.array_equal(idx, regime["idx"][list(vr.LAYER_LEAVES)])
    worst = vr.check_layers(got, vr.layer_acts(x, idx, regime["w32"]), vr.layer_acts(x, idx, regime["w64"]))
    print(f"{regime['name']}: worst layer {worst[0]} {worst[1]:.2e} of its largest value (fp32 restatement {worst[2]:.2e})")


def test_fp32_one_batch_inside_a_larger_array_bit_for_bit(regime):
    c = regime["codec"]
    big = synth_vec3.make_leaves(97, seed=4242)
    idx = c.encode(big)
    rec = c.decode(idx)
    part = np.ascontiguousarray(big[7:40])
    assert len(part) == 33
    assert np.array_equal(c.encode(part), idx[7:40])
    assert same(c.decode(np.ascontiguousarray(idx[7:40])), rec[7:40])


def test_fp32_duplicates_with_equal_norms_go_to_the_lower_index(file_free, leaves):
    """default_like: every |e|^2 agrees to an ulp, so the search is decided by z.e alone and a tie is a tie of the MFMA sums."""
    w = file_free["default_like"]
    c = HipVec3Codec(weightpack.dumps(w))
    try:
        first = c.encode(leaves)
    finally:
        c.close()
    pairs = duplicate_pairs(first.reshape(-1))
    e = w["quantizer.embedding"].copy()
    for src, dst, _lo, _hi in pairs:
        e[dst] = e[src]
    c = HipVec3Codec(weightpack.dumps({**w, "quantizer.embedding": e}))
    try:
        vr.check_duplicates(first, c.encode(leaves), pairs)
    finally:
        c.close()


# ---- bf16 mode --------------------------------------------------------------------------------------------------------
def test_bf16_search_criterion_on_the_mode_s_own_latent(regime, leaves):
    c = regime["bf16"]
    c.debug_enable(True)
    try:
        idx = c.encode(leaves)
        z = torch.from_numpy(c.debug_fetch("encoder.proj", len(leaves))).double()
    finally:
        c.debug_enable(False)
    worst = vr.check_latent_vs_fp64(idx, vr.flat(z), regime["w64"]["quantizer.embedding"])
    print(f"{regime['name']} bf16: worst excess {worst:.3f} of the bound, {float((idx != regime['idx']).mean()):.4f} of the indices differ from fp32 mode")


def test_bf16_every_layer_teacher_forced(regime, leaves):
    """As test_gpu_vec3_bf16.test_every_layer_teacher_forced_against_the_bf16_restatement, FLIP_SHARE and FLIP_BOUND unchanged,
    on the first 8 leaves."""
    c, w64 = regime["bf16"], regime["w64"]
    x = np.ascontiguousarray(leaves[:STAGE_LEAVES])
    c.debug_enable(True)
    try:
        idx = c.encode(x)
        c.decode(idx)
        got = {k: c.debug_fetch(k, STAGE_LEAVES) for k in VEC3_DEBUG_LAYERS}
    finally:
        c.debug_enable(False)
    with torch.no_grad():
        got["leaves"] = x
        got["codes"] = tb.codes(idx, w64).reshape(STAGE_LEAVES, 64, 64).numpy()
    worst_share, worst_err, over = 0.0, 0.0, []
    for name, (prev, _fn) in tb.STAGES.items():
        ref = tb.stage(name, got[prev], w64).numpy()
        err = np.abs(got[name].astype(np.float64) - ref)
        top = float(np.abs(ref).max())
        share = float((err > 1e-5 * top).mean())
        worst_share, worst_err = max(worst_share, share), max(worst_err, float(err.max()) / top)
        if share > FLIP_SHARE or float(err.max()) > FLIP_BOUND * top:
            over.append((name, share, float(err.max()) / top))
    print(f"{regime['name']} bf16: largest share of elements over 1e-5 {worst_share:.2e}, largest error {worst_err:.2e} of the largest value")
    assert not over, f"layers outside the flip cap (name, share over 1e-5, largest error / largest value): {over}"


def test_bf16_duplicate_rows_go_to_the_lower_index(regime, leaves):
    first = regime["bf16"].encode(leaves)
    src = int(np.bincount(first.reshape(-1)).argmax())
    dst = src + 128 if src + 128 < 4096 else src - 128
    e = regime["w"]["quantizer.embedding"].copy()
    e[dst] = e[src]
    c = HipVec3Codec(weightpack.dumps({**regime["w"], "quantizer.embedding": e}), precision="bf16")
    try:
        idx = c.encode(leaves)
    finally:
        c.close()
    assert (idx[first == src] == min(src, dst)).all() and not (idx == max(src, dst)).any()


# ---- fused paths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fused_round_trip_and_bounded_pairs(regime, leaves, mode):
    """In every regime, `wide` and `saturated` among them: the two that stretch the value range."""
    c = regime["codec"] if mode == "fp32" else regime["bf16"]
    assert c.precision == mode
    idx, err, rec = c.roundtrip(leaves, return_recon=True)
    assert np.array_equal(idx, c.encode(leaves)) and same(rec, c.decode(idx))
    assert same(err[:, 0], np.abs(leaves - rec).reshape(len(leaves), -1).max(axis=1))
    tol = float(np.median(err[:, 0]))
    bad = np.ascontiguousarray(np.concatenate([leaves, leaves[3:5]]))
    n = len(leaves)
    bad.view(np.uint32)[n, 300, 1] = 0x7FC12345
    bad[n + 1, 17, 2] = -np.inf
    ok = np.arange(n)
    bidx, ids, raw = c.compress_bounded(bad, tol)
    out = c.decompress_bounded(bidx, ids, raw)
    assert 0 < len(ids) < n + 2 and n in ids and n + 1 in ids
    assert (np.abs(bad[ok] - out[ok]) <= np.float32(tol)).all()
    assert same(out[n:], bad[n:])
    ridx, code, payload = c.compress_residual(bad, tol)
    out = c.decompress_residual(ridx, tol, code, payload)
    assert (np.abs(bad[ok] - out[ok]) <= np.float32(tol)).all()
    assert same(out[n:], bad[n:])
    assert np.array_equal(bidx[ok], idx) and np.array_equal(ridx[ok], idx)
    print(f"{regime['name']} {mode}: tol {tol:.4f}, {len(ids)} of {n + 2} leaves raw in the bounded pair, {len(payload)} residual bytes")


# ---- codebook-size edges ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kedge():
    """The 65 536-code model, the leaves of the size edges (with one non-finite leaf appended) and their float32 / float64
    latents: the encoder does not depend on K."""
    big = synth_vec3.make_weights(0, k_codes=65536)
    x = vr.k_leaves()
    enc = {k: v for k, v in big.items() if k != "quantizer.embedding"}
    bad = x[2:3].copy()
    bad[0, 100, 0] = np.nan
    bad[0, 200, 1] = np.inf
    return {"big": big, "leaves": x, "with_bad": np.ascontiguousarray(np.concatenate([x, bad])),
            "z64": vr.latents(x, tr.weights_to_torch(enc, torch.float64))}


@pytest.mark.parametrize("k", vr.K_EDGES)
def test_codebook_size_edges_with_planted_codes(k, kedge):
    x, n = kedge["leaves"], len(kedge["leaves"])
    w, pos, rows = vr.planted_codes(vr.k_edge_weights(kedge["big"], k), x, z64=kedge["z64"])
    gap = vr.planted_precondition(w, x, pos, rows, z64=kedge["z64"])
    w32, w64 = tr.weights_to_torch(w, torch.float32), tr.weights_to_torch(w, torch.float64)
    pack = weightpack.dumps(w)
    for mode in MODES:
        c = HipVec3Codec(pack, precision=mode)
        try:
            assert c.model_info()["num_codes"] == k
            c.debug_enable(True)
            try:
                idx = c.encode(kedge["with_bad"])
                z = torch.from_numpy(c.debug_fetch("encoder.proj", n)).double()
            finally:
                c.debug_enable(False)
            assert idx.shape == (n + 1, 64) and int(idx.max()) < k       # the non-finite leaf included
            idx = np.ascontiguousarray(idx[:n])
            assert np.array_equal(idx.reshape(-1)[pos], rows), (mode, idx.reshape(-1)[pos], rows)
            # fp32 mode against the float64 latents of the restatement, bf16 mode on its own latent
            worst = vr.check_latent_vs_fp64(idx, kedge["z64"] if mode == "fp32" else vr.flat(z), w64["quantizer.embedding"])
            dec = vr.decode_indices(idx, k, n_random=8)
            rec = c.decode(dec)
            if mode == "fp32":
                rec32, rec64 = vr.decode_refs(dec, w32, w64)
            else:                                   # the voxel bar with the mode's own restatement in the float32 one's place
                with torch.no_grad():
                    rec32, rec64 = tb.decode(dec, w64).numpy(), tr.decode(dec, w64).numpy()
            d, d_ref = vr.check_voxels(rec, rec32, rec64)
            print(f"K = {k} {mode}: smallest planted gap {gap:.2e}, worst excess {worst:.3f}, voxels {d:.2e} from fp64 (d_ref {d_ref:.2e})")
            if k == 65536:
                assert (dec >= 32768).any()
                di = torch.zeros((n, 64), dtype=torch.int16, device="cuda")
                dx = torch.from_numpy(x).cuda()
                dd = torch.from_numpy(dec.view(np.int16)).cuda()
                do = torch.zeros((len(dec), 512, 3), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                c.encode_device(dx.data_ptr(), n, di.data_ptr())
                c.decode_device(dd.data_ptr(), len(dec), do.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(di.cpu().numpy().view(np.uint16), idx) and same(do.cpu().numpy(), rec)
            else:
                with pytest.raises(RuntimeError, match="out of range"):
                    c.decode(np.full((2, 64), k, np.uint16))
                assert np.array_equal(c.encode(x), idx) and same(c.decode(dec), rec)   # the handle still works
        finally:
            c.close()
