"""The persistent kernels at other compute-unit counts (VQHIP_CUS=k, run with -m gpu on an MI355X).

conv_first_once_k, conv8_lds_k (16 and 8 waves), conv_down_lds_k, conv4_lds_k, stem_taps_k and wgrad_rows4_k size their grid
from the handle's compute-unit count and carry pipeline state from one item (8-leaf group, half tile, tile, slice) into the
next.  With 256 compute units a workgroup reaches a second item only above 4 096 leaves, where the suite fetches hardly any
intermediate layer.  With the count lowered to 1 ... 7 a 97-leaf batch (4 tiles, 8 half tiles, 16 groups) makes every one of
them walk several items, with uneven trip counts (half tiles 8 / 3,3,2 / 2,2,2,1,1 / 2,1,1,1,1,1,1 at k = 1, 3, 5, 7), and the
CPU oracle returns every layer of such a batch at once.  Unless a case says otherwise the handles run the kernels of full
chunks (set_small_batch_tiles(0)), and every handle asserts through vqhip_compute_units that the switch was honoured.

Everything but the gradients is compared bit for bit (+0 / -0 identified).  The gradients: 5e-6 of each tensor's largest fp64
gradient, widened only by check_gradients' rule (keyed to torch's own fp32 error), the loss 2e-5 relative — the helpers and
bars of tests/test_gpu_fulltrain_edges.py; another count is another order of the weight gradients' partial sums, so no two
counts are compared with each other there.

Measured on the MI355X (worst GPU gradient error / torch fp32's worst; no bar widened; loss error 1.1e-8 .. 3.1e-8):
  33 leaves k=1 (both policies)  1.48e-6 / 1.61e-6      33 leaves k=3          1.44e-6 / 1.61e-6
  65 leaves k=3                  2.21e-6 / 1.82e-6      65 leaves k=32, 50 %   1.36e-6 / 1.82e-6
  33 leaves k=3, 10 %            1.48e-6 / 1.61e-6
The largest sit on the layers of wgrad_rows4_k (decoder.stem.0.weight): a handful of slices add hundreds of macro steps each in
fp32 where 256 slices add one or two (4.90e-7 / 5.29e-7 at 256 compute units).  Every bit-exact case holds; no kernel bug found.
With write_plane of the 8-wave conv8_lds_k recomputing its GroupNorm scale / shift only at P == 0 (scratch build),
test_large_path_kernel_variants_agree still passes and the k3-conv8-w8 case here fails at e_y4 of the 97-leaf batch, leaves 48 .. 96."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fulltrain_common import fwdbwd, handle_idx, pick, pool, screen  # noqa: E402
from oracle.oracle import DEBUG_SHAPES, DEC_DEBUG, ENC_DEBUG, VQ_STATS_FLOATS  # noqa: E402
from test_gpu_fulltrain_edges import check_gradients, check_loss, references  # noqa: E402
from vqvdb_amd import synth, weightpack  # noqa: E402
from vqvdb_amd.codebook_training import K  # noqa: E402
from vqvdb_amd.codec import HipCodec  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("VQHIP_CUS", "VQHIP_CONV8", "VQHIP_FIRST", "VQHIP_CONV4", "VQHIP_DOWN", "VQHIP_TRAIN_WGRAD_CU_PCT")
ENC_LAYERS = [name for name in ENC_DEBUG if name not in ("e_x12", "e_z")]   # gated activations and the 128-channel latent are never formed on the GPU
DEC_LAYERS = ["d_ystem", "d_d2", "d_y4", "d_x6"]


def _bits(a):
    return np.where(a == 0, 0.0, a).astype(np.float32).view(np.uint32)


def make(pack, monkeypatch, k=None, tiles=0, **env):
    """A handle created under VQHIP_CUS=k (None: without the variable) and the kernel switches of `env`; the environment is
    clean again when this returns."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if k is not None:
        monkeypatch.setenv("VQHIP_CUS", str(k))
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    c = HipCodec(pack)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    device, in_use = c.compute_units()
    assert device >= 1 and in_use == (device if k is None else k), (k, device, in_use)
    c.set_small_batch_tiles(tiles)
    return c


@pytest.fixture(scope="module")
def pack(weights):
    return weightpack.dumps(weights)


@pytest.fixture(scope="module")
def device_cus(pack):
    assert "VQHIP_CUS" not in os.environ
    c = HipCodec(pack)
    device, in_use = c.compute_units()
    c.close()
    assert in_use == device
    return device


# ---- a: the encoder, every stored layer ----
@pytest.fixture(scope="module")
def enc_batches(oracle):
    """(leaves, the oracle's indices, the oracle's layers) of the 33-leaf batch, the 97-leaf batch and the edge leaves."""
    out = {}
    for label, leaves in (("n33", synth.make_leaves(33, seed=4101)), ("n97", synth.make_leaves(97, seed=4102)), ("edge", synth.edge_leaves())):
        oidx, dbg = oracle.encode(leaves, threads=8, debug=ENC_DEBUG)
        out[label] = (leaves, oidx, dbg)
    return out


ENC_CASES = [(1, {}), (3, {}), (5, {}), (7, {}), (3, {"VQHIP_CONV8": "w8"}), (3, {"VQHIP_FIRST": "twopass"}), (3, {"VQHIP_CONV4": "rows"}),
             (3, {"VQHIP_DOWN": "rows"})]


@pytest.mark.parametrize("k,env", ENC_CASES, ids=[f"k{k}" + "".join(f"-{name[6:].lower()}-{v}" for name, v in env.items()) for k, env in ENC_CASES])
def test_encoder_every_layer_equals_the_oracle(pack, enc_batches, monkeypatch, k, env):
    c = make(pack, monkeypatch, k, **env)
    try:
        for label, (leaves, oidx, dbg) in enc_batches.items():
            n = len(leaves)
            c.debug_enable(True)
            idx = c.encode(leaves)
            for name in ENC_LAYERS:
                ch, p = DEBUG_SHAPES[name]
                got = _bits(c.debug_fetch(name, n, ch, p))
                bad = np.flatnonzero((got != _bits(dbg[name])).reshape(n, -1).any(axis=1))
                assert len(bad) == 0, f"k={k} {env} {label}: layer {name} differs from the oracle in leaves {bad[:16]}"
            assert np.array_equal(idx, oidx), (k, env, label, "indices, debug mode")
            c.debug_enable(False)
            assert np.array_equal(c.encode(leaves), oidx), (k, env, label, "indices")
    finally:
        c.close()


# ---- b: the decoder ----
@pytest.fixture(scope="module")
def dec_batch(oracle, golden, enc_batches):
    idx = np.ascontiguousarray(np.concatenate([enc_batches["n97"][1], golden["idx_edge"]]))
    assert len(idx) == 105      # four tiles, nine leaves in the last
    orec, dbg = oracle.decode(idx, threads=8, debug=DEC_DEBUG)
    return idx, orec, dbg


@pytest.mark.parametrize("k,tiles", [(1, 0), (3, 0), (3, -1)], ids=["k1", "k3", "k3-default-policy"])
def test_decoder_layers_and_voxels_equal_the_oracle(pack, dec_batch, monkeypatch, k, tiles):
    """tiles = -1: four tiles on three compute units is `nt >= n_cus`, the position-split path's call of stem_taps_k."""
    idx, orec, dbg = dec_batch
    n = len(idx)
    c = make(pack, monkeypatch, k, tiles=tiles)
    try:
        c.debug_enable(True)
        rec = c.decode(idx)
        for name in DEC_LAYERS:
            ch, p = DEBUG_SHAPES[name]
            got = _bits(c.debug_fetch(name, n, ch, p))
            bad = np.flatnonzero((got != _bits(dbg[name])).reshape(n, -1).any(axis=1))
            assert len(bad) == 0, f"k={k} tiles={tiles}: layer {name} differs from the oracle in leaves {bad[:16]}"
        c.debug_enable(False)
        assert np.array_equal(_bits(rec), _bits(orec)), (k, tiles, "voxels, debug mode")
        assert np.array_equal(_bits(c.decode(idx)), _bits(orec)), (k, tiles, "voxels")
    finally:
        c.close()


# ---- c: one result whatever the count ----
def test_results_do_not_depend_on_the_count(pack, oracle, device_cus, monkeypatch):
    leaves = np.concatenate([synth.make_leaves(200, seed=4103), synth.sparse_leaves(92, seed=4104), synth.edge_leaves()])
    assert len(leaves) == 300
    c = make(pack, monkeypatch)
    ref_idx = c.encode(leaves)
    ref_rec = c.decode(ref_idx)
    c.close()
    assert np.array_equal(ref_idx[:64], oracle.encode(leaves[:64], threads=8))
    assert np.array_equal(_bits(ref_rec[:64]), _bits(oracle.decode(ref_idx[:64], threads=8)))
    for k in sorted({1, 2, 3, 5, 7, 8, 32, 64, device_cus}):
        c = make(pack, monkeypatch, k)
        try:
            idx = c.encode(leaves)
            rec = c.decode(idx)
        finally:
            c.close()
        assert np.array_equal(idx, ref_idx), k
        assert np.array_equal(_bits(rec), _bits(ref_rec)), k


# ---- d: poison across an item boundary ----
@pytest.mark.parametrize("k", [1, 3])
def test_nan_inf_poison_does_not_cross_an_item_boundary(pack, monkeypatch, k):
    """The batch and the poisons of test_nan_inf_poison_stays_inside_its_own_leaf, but here a workgroup that held a poisoned
    group, half tile or tile in its registers and LDS goes on to a clean one (k = 1: one workgroup walks them all)."""
    leaves = synth.make_leaves(65, seed=21)
    poisons = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf), "3e38": np.float32(3e38)}
    bad = [5, 37, 64]
    keep = np.array([i for i in range(65) if i not in bad])
    c = make(pack, monkeypatch, k)
    try:
        clean_idx = c.encode(leaves)
        clean_rec = c.decode(clean_idx)
        for name, val in poisons.items():
            x = leaves.copy()
            x[5, 100] = val                      # one voxel
            x[37, :] = val                       # a whole leaf
            x[64, 0] = val
            x[64, 511] = -val if name != "nan" else val
            idx = c.encode(x)
            assert np.array_equal(idx[keep], clean_idx[keep]), (k, name)
            rec = c.decode(idx)
            assert np.isfinite(rec).all(), (k, name)
            assert np.array_equal(_bits(rec[keep]), _bits(clean_rec[keep])), (k, name)
            print(f"k={k} poison {name:4s}: leaf 5 -> {np.unique(idx[5]).size} distinct codes, leaf 37 -> codes {np.unique(idx[37])[:4]}, "
                  f"leaf 64 -> {np.unique(idx[64]).size} distinct codes")
    finally:
        c.close()


# ---- e: codebook-training statistics ----
def test_codebook_statistics_and_update_equal_the_oracle(pack, oracle, weights, monkeypatch):
    from test_gpu_training import _gpu_stats
    leaves = synth.make_leaves(65, seed=4105)
    c = make(pack, monkeypatch, 3)
    try:
        c.train_begin()
        state = {"embedding": weights["quantizer.embedding"].copy(), "cluster_size": np.ones(K, np.float32),
                 "embed_avg": weights["quantizer.embedding"].copy()}
        stats, idx, z = _gpu_stats(c, leaves)
        oz = oracle.latent(leaves, threads=8)
        assert np.array_equal(_bits(z), _bits(oz))
        oidx = oracle.vq_assign(oz, state["embedding"], threads=8)
        assert np.array_equal(idx, oidx)
        ostats = oracle.vq_stats(oz, oidx, state["embedding"])
        assert len(ostats) == VQ_STATS_FLOATS and np.array_equal(_bits(stats.cpu().numpy()), _bits(ostats))
        c.train_vq_update_device(stats.data_ptr(), 0.95, 1e-4, torch.cuda.current_stream().cuda_stream)
        state = oracle.vq_update(ostats, state, 0.95, 1e-4)
        got = c.train_get_state()
        for name in state:
            assert np.array_equal(_bits(got[name]), _bits(state[name])), name
    finally:
        c.close()


# ---- f: full-training gradients against fp64 ----
@pytest.fixture(scope="module")
def screened():
    """The 65 screened leaves of tests/test_gpu_fulltrain_edges.py with their fp64 assignment; the references by batch size."""
    W0 = synth.make_weights(0)
    cand = pool()
    keep, idx64 = screen(cand, W0)
    chosen = pick(keep, 65)
    return {"W": W0, "pack": weightpack.dumps(W0), "leaves": np.ascontiguousarray(cand[chosen]), "idx": idx64[chosen], "ref": {}}


def ref_of(screened, n):
    if n not in screened["ref"]:
        screened["ref"][n] = references(screened["leaves"][:n], np.ones(n), screened["W"], screened["idx"][:n])
    return screened["ref"][n]


GRAD_CASES = [(33, 1, None, 0), (33, 1, None, -1), (33, 3, None, 0), (65, 3, None, 0), (65, 32, "50", 0), (33, 3, "10", 0)]


@pytest.mark.parametrize("n,k,pct,tiles", GRAD_CASES,
                         ids=[f"n{n}-k{k}" + (f"-pct{pct}" if pct else "") + ("-default-policy" if tiles else "") for n, k, pct, tiles in GRAD_CASES])
def test_gradients_against_fp64(screened, monkeypatch, n, k, pct, tiles):
    """wgrad_rows4_k cuts 100 macro steps per tile into Q slices, Q from the count (and VQHIP_TRAIN_WGRAD_CU_PCT) times 1, 2 or
    4 by layer: k = 1 is Q = 1, 2, 4 (a slice spans several classes), k = 3 with 10 % would be no slice at all and must be one."""
    env = {"VQHIP_TRAIN_WGRAD_CU_PCT": pct} if pct else {}
    label = f"k={k} n={n}" + (f" pct={pct}" if pct else "") + (" default policy" if tiles else "")
    leaves = np.ascontiguousarray(screened["leaves"][:n])
    c = make(screened["pack"], monkeypatch, k, tiles=tiles, **env)
    try:
        c.fulltrain_begin()
        assert np.array_equal(handle_idx(c, leaves), screened["idx"][:n]), f"{label}: the handle's assignment is not the fp64 argmin"
        g, aux = fwdbwd(c, leaves)
    finally:
        c.close()
    vals, g64, g32 = ref_of(screened, n)
    check_gradients(label, g, g64, g32)
    check_loss(label, aux, vals)


# ---- g: refusals ----
def test_values_outside_the_range_are_refused_at_create(pack, device_cus, monkeypatch):
    leaves = synth.make_leaves(40, seed=4106)
    c = make(pack, monkeypatch, tiles=-1)
    want = c.encode(leaves)
    c.close()
    for value in ("0", "-1", "abc", str(device_cus + 1)):
        monkeypatch.setenv("VQHIP_CUS", value)
        with pytest.raises(RuntimeError, match="VQHIP_CUS"):
            HipCodec(pack)
    monkeypatch.delenv("VQHIP_CUS")
    c = HipCodec(pack)
    try:
        assert c.compute_units() == (device_cus, device_cus)
        assert np.array_equal(c.encode(leaves), want)
    finally:
        c.close()
