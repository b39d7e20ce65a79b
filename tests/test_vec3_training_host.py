"""Vec3 codebook training, host side: the training header's declarations against the library's exports and the bound
argtypes, the fixture's regeneration from the imported reference, the torch restatement against the fixture (three
training-mode steps, eval forward, dead-code reset), metrics from a statistics buffer, a two-rank gloo all-reduce of a
statistics buffer, and the wrappers' argument checks.  Runs without a GPU."""
import ctypes
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
import torch_ref_vec3_train as trt  # noqa: E402
from vqvdb_amd import codec as vc  # noqa: E402
from vqvdb_amd import synth_vec3, vec3_training  # noqa: E402
from vqvdb_amd.codebook_training import dead_code_reset  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_train_v1.npz")
HEADER = os.path.join(ROOT, "include", "vqvdb_hip_vec3_train.h")
K = synth_vec3.K_CODES


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def w32():
    return tr.weights_to_torch(synth_vec3.make_weights(0), torch.float32)


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-30))


def test_train_header_declarations_exports_and_argtypes():
    from vqvdb_amd.build import build
    with open(HEADER) as f:
        declared = re.findall(r"\b(vqhip_vec3_train_\w+)\s*\(", f.read())
    assert sorted(set(declared)) == sorted(vc.VEC3_TRAIN_SYMBOLS)
    assert not set(vc.VEC3_TRAIN_SYMBOLS) & set(vc.ABI_SYMBOLS)
    with open(os.path.join(ROOT, "include", "vqvdb_hip.h")) as f:
        assert not set(re.findall(r"\b(vqhip_\w+)\s*\(", f.read())) & set(vc.VEC3_TRAIN_SYMBOLS)
    lib = ctypes.CDLL(build())
    for name in vc.VEC3_TRAIN_SYMBOLS:
        assert hasattr(lib, name), name
    lib = vc.load_library()
    for name in vc.VEC3_TRAIN_SYMBOLS:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.vqhip_vec3_train_stats_floats.restype == ctypes.c_int64
    # the pointer arguments are bound as pointers (64-bit), the EMA scalars as float
    assert lib.vqhip_vec3_train_vq_update_device.argtypes[2:4] == [ctypes.c_float, ctypes.c_float]
    assert len(lib.vqhip_vec3_train_vq_stats_device.argtypes) == 7 and len(lib.vqhip_vec3_train_eval_device.argtypes) == 7
    # a NULL handle is refused without a device
    assert lib.vqhip_vec3_train_stats_floats(None) == -1
    assert lib.vqhip_vec3_train_begin(None, None, None) == -1


def test_fixture_regenerates_from_reference():
    if not os.path.isdir(os.environ.get("VQVDB_REFERENCE_PYTHON", "/root/reference/python")):
        pytest.skip("reference checkout not available")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_vec3_train.py"), "--check"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bit for bit" in r.stdout


def test_restatement_reproduces_three_training_steps(g, w32):
    st = trt.initial_state(synth_vec3.make_weights(0))
    for s in range(3):
        with torch.no_grad():
            z = tr.encoder(synth_vec3.make_leaves(64, seed=5000 + s), w32)
        if s == 0:
            assert rel(z[:8].reshape(8, 64, 64).numpy(), g["z0"]) < 1e-5
        r = trt.quantizer_step(trt.flat_of(z), st)
        idx = r["idx"].reshape(-1, 64).numpy()
        flips = (idx != g[f"s{s}_idx"])
        assert not (flips & (g[f"s{s}_gap"] >= 1e-3)).any(), f"step {s}: index differs at a clear position"
        assert not flips.any(), f"step {s}: {int(flips.sum())} near-tie flips (the later steps would diverge)"
        assert abs(r["vq_loss"] - g[f"s{s}_loss"][0]) <= 1e-4 * g[f"s{s}_loss"][0]
        assert abs(r["perplexity"] - g[f"s{s}_loss"][1]) <= 1e-4 * g[f"s{s}_loss"][1]
        used = g[f"s{s}_used"]
        assert rel(st["cluster_size"].numpy(), g[f"s{s}_cs"]) < 1e-5
        assert rel(st["embedding"].numpy()[used], g[f"s{s}_emb"]) < 1e-5
        assert rel(st["embed_avg"].numpy()[used], g[f"s{s}_avg"]) < 1e-5
    sums = np.array([[b.double().sum().item(), (b.double() ** 2).sum().item()] for b in (st["embedding"], st["cluster_size"], st["embed_avg"])])
    assert np.allclose(sums, g["final_sums"], rtol=1e-5, atol=1e-3)


def test_restatement_reproduces_eval_forward(g, w32):
    st = trt.initial_state(synth_vec3.make_weights(0))
    r = trt.eval_forward(synth_vec3.make_leaves(64, seed=6000), w32, st)
    got = np.array([r["mse"], r["l1"], r["vq_loss"], r["perplexity"]])
    assert np.all(np.abs(got - g["eval_loss"]) <= 1e-5 * np.abs(g["eval_loss"]))
    assert np.abs(r["rec"][:8] - g["eval_rec"]).max() < 1e-5


def test_dead_code_reset_on_vec3_state_matches_fixture(g, w32):
    st = trt.initial_state(synth_vec3.make_weights(0))
    for s in range(3):
        with torch.no_grad():
            z = tr.encoder(synth_vec3.make_leaves(64, seed=5000 + s), w32)
        trt.quantizer_step(trt.flat_of(z), st)
    flat = trt.flat_of(z)
    gen = torch.Generator().manual_seed(1234)
    n = dead_code_reset(st, flat, 1.0, gen)
    dead, pick = g["reset_dead"], g["reset_pick"]
    assert n == len(dead)
    assert np.array_equal(st["embedding"][dead].numpy(), flat[pick].numpy())
    assert np.array_equal(st["embed_avg"][dead].numpy(), flat[pick].numpy())
    assert (st["cluster_size"][dead] == 1.0).all()


def test_metrics_from_stats():
    k = 8
    rng = np.random.default_rng(0)
    flat = rng.standard_normal((640, 64)).astype(np.float32)
    emb = rng.standard_normal((k, 64)).astype(np.float32)
    idx = rng.integers(0, 5, 640)
    stats = trt.stats_fp64(flat, idx, emb)
    m = vec3_training.metrics_from_stats(stats, k)
    p = np.bincount(idx, minlength=k) / 640
    assert m["rows"] == 640 and m["codes_used"] == 5
    assert np.isclose(m["vq_loss"], 0.25 * ((flat - emb[idx]).astype(np.float64) ** 2).mean())
    assert np.isclose(m["perplexity"], np.exp(-(p * np.log(p + 1e-10)).sum()))
    assert vec3_training.metrics_from_stats(np.zeros(66 * k + 1), k)["rows"] == 0
    with pytest.raises(ValueError, match="66"):
        vec3_training.metrics_from_stats(np.zeros(66 * k), k)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gloo_rank(rank, world, port, q):
    import torch.distributed as dist
    from vqvdb_amd.codebook_training import allreduce_stats
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    t = torch.from_numpy(np.arange(66 * K + 1, dtype=np.float32) * (rank + 1))
    allreduce_stats(t)
    q.put((rank, t.numpy().copy()))
    dist.destroy_process_group()


def test_two_rank_gloo_allreduce_of_stats_buffer():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_gloo_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    want = np.arange(66 * K + 1, dtype=np.float32) * 3
    for r in range(2):
        assert got[r].shape == (66 * K + 1,) and np.array_equal(got[r], want)


def test_wrappers_reject_bad_arguments_before_any_device():
    C = vc.HipVec3Codec
    with pytest.raises(ValueError, match="non-negative"):
        C.check_train_batch(-1, 1)
    with pytest.raises(ValueError, match="NULL"):
        C.check_train_batch(4, 0)
    C.check_train_batch(0, 1)
    for decay, eps in ((-0.1, 1e-4), (1.5, 1e-4), (float("nan"), 1e-4), (0.9, 0.0), (0.9, -1.0)):
        with pytest.raises(ValueError):
            C.check_ema(decay, eps)
    C.check_ema(0.0, 1e-4)
    C.check_ema(1.0, 1e-4)
    with pytest.raises(ValueError, match="embedding"):
        C.check_state(K, embedding=np.zeros((K, 63), np.float32))
    with pytest.raises(ValueError, match="cluster_size"):
        C.check_state(K, cluster_size=np.zeros(K + 1, np.float32))
    e, cs, av = C.check_state(K, None, np.ones(K, np.float64), None)
    assert e is None and av is None and cs.dtype == np.float32
    with pytest.raises(ValueError, match="float32"):
        vec3_training._leaves_arg(torch.zeros(2, 512, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="512 x 3"):
        vec3_training._leaves_arg(torch.zeros(2, 512, dtype=torch.float32))
    with pytest.raises(ValueError, match="decay"):
        vec3_training.Vec3CodebookTrainer(object(), decay=2.0)
