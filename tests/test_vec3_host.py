"""Vec3 model (VQVAE(3, 64, K)), host side: ABI declaration, wrapper argument checks, pack validation messages,
synthetic data regeneration, weight-pack export, and the torch restatement pinned to the reference's fixture.
Runs without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
from torch_ref_vec3 import check_indices_vs_fixture  # noqa: E402
from vqvdb_amd import codec as vc  # noqa: E402
from vqvdb_amd import synth_vec3, weightpack  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_v1.npz")
VEC3_FUNCS = ["vqhip_vec3_create", "vqhip_vec3_destroy", "vqhip_vec3_last_error", "vqhip_vec3_model_info", "vqhip_vec3_encode",
              "vqhip_vec3_decode", "vqhip_vec3_encode_device", "vqhip_vec3_decode_device", "vqhip_vec3_set_chunk_leaves",
              "vqhip_vec3_chunk_leaves", "vqhip_vec3_debug_enable", "vqhip_vec3_debug_fetch"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def w32():
    return tr.weights_to_torch(synth_vec3.make_weights(0), torch.float32)


def _declared():
    with open(os.path.join(ROOT, "include", "vqvdb_hip.h")) as f:
        return re.findall(r"\b(vqhip_vec3_\w+)\s*\(", f.read())


def test_vec3_symbols_declared_and_exported():
    from vqvdb_amd.build import build
    assert sorted(set(_declared())) == sorted(VEC3_FUNCS)
    assert set(VEC3_FUNCS) <= set(vc.ABI_SYMBOLS)
    lib = ctypes.CDLL(build())
    for name in VEC3_FUNCS:
        assert hasattr(lib, name), name
    lib = vc.load_library()
    for name in VEC3_FUNCS:
        assert getattr(lib, name).argtypes is not None, name


def test_vec3_wrapper_argument_checks():
    good = np.zeros((2, 512, 3), np.float32)
    assert vc.HipVec3Codec.check_leaves(good).shape == (2, 512, 3)
    assert vc.HipVec3Codec.check_leaves(np.zeros((2, 8, 8, 8, 3), np.float32)).shape == (2, 512, 3)
    with pytest.raises(TypeError, match="float32"):
        vc.HipVec3Codec.check_leaves(np.zeros((2, 512, 3), np.float64))
    with pytest.raises(ValueError, match="shape"):
        vc.HipVec3Codec.check_leaves(np.zeros((2, 512), np.float32))
    with pytest.raises(ValueError, match="shape"):
        vc.HipVec3Codec.check_leaves(np.zeros((2, 3, 8, 8, 8), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        vc.HipVec3Codec.check_leaves(np.zeros((2, 512, 6), np.float32)[:, :, ::2])
    assert vc.HipVec3Codec.check_indices(np.zeros((3, 4, 4, 4), np.uint16)).shape == (3, 64)
    with pytest.raises(TypeError, match="uint16"):
        vc.HipVec3Codec.check_indices(np.zeros((3, 64), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        vc.HipVec3Codec.check_indices(np.zeros((3, 32), np.uint16))
    with pytest.raises(ValueError, match="contiguous"):
        vc.HipVec3Codec.check_indices(np.zeros((64, 3), np.uint16).T)


def _pack_error(tensors) -> str:
    """vqhip_vec3_create's message for a pack; the pack is validated before any device is touched."""
    with pytest.raises(RuntimeError) as e:
        vc.HipVec3Codec(weightpack.dumps(tensors))
    return str(e.value)


def test_vec3_malformed_packs_fail_with_messages_before_the_device():
    from vqvdb_amd import synth
    w = synth_vec3.make_weights(0, k_codes=8)
    assert "not a Vec3 model pack" in _pack_error(synth.make_weights(0))
    bad = dict(w)
    bad["quantizer.embedding"] = np.zeros((8, 32), np.float32)
    assert "embedding_dim is 32" in _pack_error(bad)
    bad["quantizer.embedding"] = np.zeros((65537, 64), np.float32)
    assert "num_codes is 65537" in _pack_error(bad)
    bad = dict(w)
    bad["encoder.res_stack.1.conv1.weight"] = np.zeros((128, 128, 3, 3, 1), np.float32)
    assert "'encoder.res_stack.1.conv1.weight' has unexpected shape" in _pack_error(bad)
    bad = dict(w)
    del bad["decoder.final.bias"]
    assert "missing tensor 'decoder.final.bias'" in _pack_error(bad)
    with pytest.raises(RuntimeError, match="bad magic"):
        vc.HipVec3Codec(b"x" * 64)


def test_synth_vec3_regenerates_slice_by_slice():
    a = synth_vec3.make_leaves(40, seed=7)
    b = synth_vec3.make_leaves(15, seed=7, start=20)
    assert a.dtype == np.float32 and a.shape == (40, 512, 3)
    assert np.array_equal(a[20:35].view(np.uint32), b.view(np.uint32))
    kinds = [(x == 0).all() for x in synth_vec3.make_leaves(200)]
    assert 0 < sum(kinds) < 50, "exact-zero leaves present but rare"
    w1, w2 = synth_vec3.make_weights(0), synth_vec3.make_weights(0)
    assert [k for k, _s, _ in synth_vec3.TENSORS] == list(w1)
    assert all(np.array_equal(w1[k].view(np.uint32), w2[k].view(np.uint32)) for k in w1)
    small = synth_vec3.make_weights(0, k_codes=1000)
    assert np.array_equal(small["quantizer.embedding"], w1["quantizer.embedding"][:1000])
    e = synth_vec3.edge_leaves()
    d = np.arange(512) // 64
    assert np.array_equal(e[3, :, 0], (d / 7.0).astype(np.float32))   # channel x depends on the d axis only


def test_vec3_weightpack_round_trip_and_state_dict_export():
    w = synth_vec3.make_weights(0)
    assert len(w) == 61 and sum(v.size for v in w.values()) == 5386211
    back = weightpack.loads(weightpack.dumps(w))
    assert list(back) == list(w) and all(np.array_equal(back[k], w[k]) for k in w)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd["quantizer.cluster_size"] = torch.ones(4096)
    sd["quantizer.embed_avg"] = sd["quantizer.embedding"].clone()
    ex = weightpack.from_state_dict(sd)
    assert list(ex) == list(w) and all(np.array_equal(ex[k], w[k]) for k in w)


def test_torch_ref_vec3_reproduces_the_reference_fixture(golden, w32):
    leaves = np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])
    acts = {}
    with torch.no_grad():
        idx, _ = tr.encode(leaves[:1], w32, acts)
        idx_all, _ = tr.encode(leaves, w32)
    n_off, gap = check_indices_vs_fixture(idx_all.numpy().astype(np.uint16), golden)
    print(f"torch_ref_vec3 fp32: {n_off} positions off top-1, largest gap {gap:.2e}")
    g = golden
    with torch.no_grad():
        rec = tr.decode(np.concatenate([g["idx"][:64], g["idx"][512:]]), w32).numpy()
        tr.decode(g["idx"][:1], w32, acts)
    assert float(np.abs(rec - g["rec"]).max()) < 1e-5
    for k in g.files:
        if k.startswith("act_"):
            a = acts[k[4:]][0].reshape(g[k].shape).numpy()
            assert float(np.abs(a - g[k]).max()) <= 1e-5 * float(np.abs(g[k]).max()), k


@pytest.mark.skipif(not os.path.exists("/root/reference/python/VQVAE_v2.py"), reason="needs a reference checkout")
def test_make_golden_vec3_reproduces_the_fixture_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_vec3.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bit for bit" in r.stdout
