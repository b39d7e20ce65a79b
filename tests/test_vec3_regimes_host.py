"""Weight regimes and codebook-size edges of the Vec3 model, host side (tests/vec3_regimes.py; the GPU side is
tests/test_gpu_vec3_regimes.py): the regimes regenerate to the same bytes, the float32 torch restatement reproduces the
reference's fixture in every regime, every bar the GPU tests apply is met by that restatement alone (a GPU failure is the
kernel's), and three deliberately wrong restatements each fail an assertion the GPU tests make (the bars bite).
Runs without a GPU; the `trained` regime exists on the GPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
import vec3_regimes as vr  # noqa: E402
from test_gpu_vec3 import check_vs_fp64, duplicate_pairs  # noqa: E402
from torch_ref_vec3 import check_indices_vs_fixture  # noqa: E402
from vqvdb_amd import synth_vec3  # noqa: E402


@pytest.fixture(scope="module")
def R():
    return vr.regimes()


@pytest.fixture(scope="module")
def fixture():
    return vr.load_fixture()


@pytest.fixture(scope="module")
def leaves():
    return vr.fresh_leaves()


@pytest.fixture(scope="module")
def encoded(R, leaves):
    """regime -> float32 restatement's indices [48,64] of fresh_leaves(), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            w32 = tr.weights_to_torch(R[name], torch.float32)
            cache[name] = vr.top2(vr.latents(leaves, w32), w32["quantizer.embedding"])[0].reshape(-1, 64).astype(np.uint16)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def kedge():
    """The 65 536-code model, the leaves of the size edges and their latents (the encoder does not depend on K)."""
    big = synth_vec3.make_weights(0, k_codes=65536)
    x = vr.k_leaves()
    enc = {k: v for k, v in big.items() if k != "quantizer.embedding"}
    return {"big": big, "leaves": x, "z64": vr.latents(x, tr.weights_to_torch(enc, torch.float64)),
            "z32": vr.latents(x, tr.weights_to_torch(enc, torch.float32))}


def test_regimes_regenerate_to_the_same_bytes_and_are_what_they_say(R):
    again = vr.regimes()
    base = synth_vec3.make_weights(0)
    assert tuple(R) == vr.REGIMES
    for name in R:
        assert list(R[name]) == list(base)
        for k, v in R[name].items():
            assert v.dtype == np.float32 and v.shape == base[k].shape and v.tobytes() == again[name][k].tobytes(), (name, k)
    changed = {name: sorted(k for k in base if R[name][k].tobytes() != base[k].tobytes()) for name in vr.REGIMES[2:]}
    gn = sorted(k for k in base if vr.is_groupnorm(k))
    assert len(gn) == 24
    assert changed["default_like"] == sorted(gn + [k for k in base if k.endswith(".conv2.weight")] + ["quantizer.embedding"])
    assert changed["deadcodes"] == ["quantizer.embedding"] and changed["saturated"] == ["decoder.final.weight"]
    assert changed["wide"] == ["encoder.proj.bias", "encoder.proj.weight", "quantizer.embedding"]
    for k in changed["wide"]:                                    # an exact power of two: the scaling loses no bit
        assert np.array_equal(R["wide"][k] / np.float32(8.0), base[k]) and np.array_equal(base[k] * np.float32(8.0) / np.float32(8.0), base[k])
    d = R["default_like"]
    assert all((d[k] == (1.0 if k.endswith(".weight") else 0.0)).all() for k in gn)
    norms = np.sqrt((d["quantizer.embedding"].astype(np.float64) ** 2).sum(1))
    assert np.abs(norms - 1.0).max() <= 2.0 ** -21                 # all |e| agree to a few float32 ulp
    dead = R["deadcodes"]["quantizer.embedding"]
    rows = np.arange(4096)[5::29]
    assert len(rows) == 142 and np.array_equal(dead[rows], base["quantizer.embedding"][rows] * np.float32(0.02))
    assert np.array_equal(np.delete(dead, rows, 0), np.delete(base["quantizer.embedding"], rows, 0))
    assert np.array_equal(R["saturated"]["decoder.final.weight"], base["decoder.final.weight"] * np.float32(6.0))


@pytest.mark.parametrize("name", vr.REGIMES)
def test_torch_ref_vec3_reproduces_the_reference_fixture_in_every_regime(name, R, fixture, encoded):
    g = fixture[name]
    idx = encoded(name)[:vr.FIXTURE_LEAVES]                        # the fixture's leaves are fresh_leaves()[:24] + the edge leaves
    idx = np.concatenate([idx, encoded(name)[vr.FRESH_LEAVES:]])
    n_off, gap = check_indices_vs_fixture(idx, g)
    with torch.no_grad():
        rec = tr.decode(g["idx"], tr.weights_to_torch(R[name], torch.float32)).numpy()
    d = float(np.abs(rec - g["rec"]).max())
    print(f"{name}: torch_ref_vec3 fp32 {n_off} positions off top-1, largest gap {gap:.2e}, voxels {d:.2e} from the reference")
    assert d < 1e-5


@pytest.mark.parametrize("name", vr.REGIMES)
def test_the_bars_are_met_by_the_fp32_restatement_alone(name, R, fixture, leaves, encoded):
    w32, w64 = tr.weights_to_torch(R[name], torch.float32), tr.weights_to_torch(R[name], torch.float64)
    idx = encoded(name)
    check_vs_fp64(idx, leaves, w64)
    z64 = vr.latents(leaves, w64)
    assert vr.check_latent_vs_fp64(idx, z64, w64["quantizer.embedding"]) <= 1.0     # the chunked form of the same criterion
    idx64, _second, gap = vr.top2(z64, w64["quantizer.embedding"])
    used = len(np.unique(idx))
    assert used >= 400, "regime too collapsed to test the search"
    if name == "wide":                                               # every distance is exactly 64 x seed 0's
        assert np.array_equal(idx, _seed0_indices(leaves))
        assert float((z64 ** 2).sum(1).max()) > 1500.0
    dec = vr.decode_indices(fixture[name]["idx"], 4096)
    rec32, rec64 = vr.decode_refs(dec, w32, w64)
    d, d_ref = vr.check_voxels(rec32, rec32, rec64)
    if name == "saturated":
        assert float(np.abs(rec32).max()) == 1.0
        assert 1.0 - float(np.abs(rec64[-2:]).max()) < 1e-9         # float32 rounds to 1.0 below 3e-8: any tanhf saturates here
        assert d_ref > 5e-6                                          # why the voxel bar cannot be a flat 1e-5
    x = leaves[list(vr.LAYER_LEAVES)]
    a32, a64 = vr.layer_acts(x, idx[list(vr.LAYER_LEAVES)], w32), vr.layer_acts(x, idx[list(vr.LAYER_LEAVES)], w64)
    worst = vr.check_layers(a32, a32, a64)
    print(f"{name}: {used} codes in use, {int((idx.reshape(-1) != idx64).sum())} positions off the fp64 minimum, smallest fp64 gap "
          f"{gap.min():.2e}, d_ref {d_ref:.2e}, worst layer {worst[0]} {worst[2]:.2e}")


def _seed0_indices(leaves):
    w32 = tr.weights_to_torch(synth_vec3.make_weights(0), torch.float32)
    return vr.top2(vr.latents(leaves, w32), w32["quantizer.embedding"])[0].reshape(-1, 64).astype(np.uint16)


@pytest.mark.parametrize("k", vr.K_EDGES)
def test_the_size_edge_bars_are_met_by_the_fp32_restatement_alone(k, kedge):
    w, pos, rows = vr.planted_codes(vr.k_edge_weights(kedge["big"], k), kedge["leaves"], z64=kedge["z64"])
    assert rows.tolist() == vr.planted_rows(k) and len(set(pos.tolist())) == len(rows)
    assert np.array_equal(np.delete(w["quantizer.embedding"], rows, 0), np.delete(kedge["big"]["quantizer.embedding"][:k], rows, 0))
    gap = vr.planted_precondition(w, kedge["leaves"], pos, rows, z64=kedge["z64"])
    e32 = torch.from_numpy(w["quantizer.embedding"])
    idx = vr.top2(kedge["z32"], e32)[0]
    assert idx.max() < k
    assert np.array_equal(idx[pos], rows)
    vr.check_latent_vs_fp64(idx, kedge["z64"], e32.double())
    if k <= 4097:                                                    # the one-matrix form of the criterion, where it fits
        check_vs_fp64(idx.reshape(-1, 64), kedge["leaves"], tr.weights_to_torch(w, torch.float64))
    dec = vr.decode_indices(idx.reshape(-1, 64), k, n_random=8)
    assert k < 32768 or (dec >= 32768).any()
    rec32, rec64 = vr.decode_refs(dec, tr.weights_to_torch(w, torch.float32), tr.weights_to_torch(w, torch.float64))
    vr.check_voxels(rec32, rec32, rec64)
    print(f"K = {k}: planted rows {rows.tolist()} at positions {pos.tolist()}, smallest planted gap {gap:.2e}")


def test_planted_rows_sit_on_the_block_and_tile_borders():
    assert vr.planted_rows(1) == [0] and vr.planted_rows(2) == [0, 1] and vr.planted_rows(128) == [0, 127]
    assert vr.planted_rows(129) == [0, 127, 128] and vr.planted_rows(255) == [0, 127, 128, 254]
    assert vr.planted_rows(4097) == [0, 4095, 4096] and vr.planted_rows(65536) == [0, 65407, 65408, 65535]


# ---- the bars bite: three wrong restatements, each failing an assertion the GPU tests make -----------------------------------
def test_a_search_that_gives_a_duplicate_pair_to_the_higher_index_fails(R, leaves, encoded):
    w = R["default_like"]
    first = encoded("default_like")
    pairs = duplicate_pairs(first.reshape(-1))
    e = w["quantizer.embedding"].copy()
    for src, dst, _lo, _hi in pairs:
        e[dst] = e[src]
    w32 = tr.weights_to_torch({**w, "quantizer.embedding": e}, torch.float32)
    with torch.no_grad():
        dist = tr.distances(tr.encoder(leaves, w32), w32)
    vr.check_duplicates(first, torch.argmin(dist, dim=1).reshape(-1, 64).numpy().astype(np.uint16), pairs)   # first minimum: passes
    wrong = (e.shape[0] - 1 - torch.argmin(dist.flip(1), dim=1)).reshape(-1, 64).numpy().astype(np.uint16)    # last minimum
    with pytest.raises(AssertionError):
        vr.check_duplicates(first, wrong, pairs)


@pytest.mark.parametrize("k", (2, 129, 4097, 65536))
def test_a_search_that_leaves_out_code_k_minus_1_fails(k, kedge):
    w, pos, rows = vr.planted_codes(vr.k_edge_weights(kedge["big"], k), kedge["leaves"], z64=kedge["z64"])
    e32 = torch.from_numpy(w["quantizer.embedding"])
    good = vr.top2(kedge["z32"], e32)[0]
    wrong = vr.top2(kedge["z32"], e32[:k - 1])[0]
    # what natural leaves show of it: nothing
    natural = vr.top2(kedge["z32"], torch.from_numpy(kedge["big"]["quantizer.embedding"][:k]))[0]
    if k in (129, 4097, 65536):
        assert not (natural == k - 1).any(), "code K-1 wins on natural leaves: a dropped code would show without planting"
    assert np.array_equal(good[pos], rows)
    assert not np.array_equal(wrong[pos], rows)                      # the GPU tests' "each planted position returns its planted row"


@pytest.mark.parametrize("name", vr.REGIMES)
def test_a_groupnorm_eps_of_1e_6_fails_the_layer_bar(name, R, leaves, encoded, monkeypatch):
    w32, w64 = tr.weights_to_torch(R[name], torch.float32), tr.weights_to_torch(R[name], torch.float64)
    x, idx = leaves[list(vr.LAYER_LEAVES)], encoded(name)[list(vr.LAYER_LEAVES)]
    a32, a64 = vr.layer_acts(x, idx, w32), vr.layer_acts(x, idx, w64)
    gn = tr._gn_relu
    monkeypatch.setattr(tr, "_gn_relu", lambda t, w, prefix, eps=1e-5: gn(t, w, prefix, eps=1e-6))
    wrong = vr.layer_acts(x, idx, w32)
    monkeypatch.undo()
    with pytest.raises(AssertionError, match="of the largest value"):
        vr.check_layers(wrong, a32, a64)


@pytest.mark.skipif(not os.path.exists("/root/reference/python/VQVAE_v2.py"), reason="needs a reference checkout")
def test_make_golden_vec3_regimes_reproduces_the_fixture_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_vec3_regimes.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("bit for bit") == 2
