"""Vec3 full training without a GPU: the C ABI of include/vqvdb_hip_vec3_fulltrain.h (declarations, exports, argtypes),
argument checks of the Python wrappers before any device is touched, the torch restatement against the reference
fixture (three steps of the reference loop), the fixture's regeneration where a reference checkout exists, and the
gloo all-reduce of a gradient vector plus aux buffer."""
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

import torch_ref_vec3_fulltrain as tf  # noqa: E402
import torch_ref_vec3_train as trt  # noqa: E402
from vqvdb_amd import codec, synth_vec3, vec3_full_training  # noqa: E402

HEADER = os.path.join(ROOT, "include", "vqvdb_hip_vec3_fulltrain.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_fulltrain_v1.npz")
MAKER = os.path.join(ROOT, "tests", "golden", "make_golden_vec3_fulltrain.py")
REFERENCE = os.environ.get("VQVDB_REFERENCE_PYTHON", "/root/reference/python")


def test_header_declares_exactly_the_symbol_list():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r"\b(vqhip_vec3_fulltrain_\w+)\s*\(", text)))
    assert declared == sorted(codec.VEC3_FULLTRAIN_SYMBOLS)
    assert not set(codec.VEC3_FULLTRAIN_SYMBOLS) & set(codec.ABI_SYMBOLS)
    assert not set(codec.VEC3_FULLTRAIN_SYMBOLS) & set(codec.VEC3_TRAIN_SYMBOLS)


def test_library_exports_and_binds_every_symbol():
    lib = codec.load_library()
    for name in codec.VEC3_FULLTRAIN_SYMBOLS:
        assert getattr(lib, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_vec3_fulltrain_\w+)\b", out))
    assert exported == set(codec.VEC3_FULLTRAIN_SYMBOLS)


def test_size_queries_of_a_null_handle():
    lib = codec.load_library()
    assert lib.vqhip_vec3_fulltrain_param_count(None) == -1
    assert lib.vqhip_vec3_fulltrain_decoder_offset(None) == -1
    assert lib.vqhip_vec3_fulltrain_aux_floats(None) == -1
    assert lib.vqhip_vec3_fulltrain_begin(None) == -1


def test_parameter_layout_matches_the_model():
    names = [n for n, _ in vec3_full_training.PARAM_SPECS]
    assert names == tf.param_names() and len(names) == 60
    sizes = [int(np.prod(s)) for _, s in vec3_full_training.PARAM_SPECS]
    assert sum(sizes) == 5124067
    assert sum(s for n, s in zip(names, sizes) if n.startswith("encoder.")) == 2235712
    W = synth_vec3.make_weights(0)
    for n, shape in vec3_full_training.PARAM_SPECS:
        assert tuple(np.asarray(W[n]).shape) == shape, n
    vec = vec3_full_training.state_to_vec(W)
    back = vec3_full_training.vec_to_state(vec)
    assert all(np.array_equal(back[n], W[n]) for n in names)


class _Stub(codec.HipVec3Codec):
    """A HipVec3Codec without a library or a handle: the wrappers must fail before they reach either."""

    def __init__(self):
        self._lib, self._h = None, None

    def fulltrain_param_count(self):
        return 5124067

    def close(self):
        pass


def test_wrappers_reject_bad_arguments_before_any_device():
    s = _Stub()
    H = codec.HipVec3Codec
    with pytest.raises(ValueError):
        H.fulltrain_fwdbwd_device(s, 1, -1, 4, 1, 1)
    with pytest.raises(ValueError):
        H.fulltrain_fwdbwd_device(s, 1, 8, 4, 1, 1)        # n_global < n
    with pytest.raises(ValueError):
        H.fulltrain_fwdbwd_device(s, 1, 8, 8, 0, 1)        # NULL grads
    with pytest.raises(ValueError):
        H.fulltrain_fwdbwd_device(s, 1, 8, 8, 1, 0)        # NULL aux
    with pytest.raises(ValueError):
        H.fulltrain_forward_device(s, 1, -3)
    with pytest.raises(ValueError):
        H.fulltrain_apply_device(s, 0, 1, 1e-3, 1)          # NULL grads
    with pytest.raises(ValueError):
        H.fulltrain_apply_device(s, 1, 1, 1e-3, 0)          # step 0
    with pytest.raises(ValueError):
        H.fulltrain_apply_device(s, 1, 1, -1.0, 1)          # negative lr
    with pytest.raises(ValueError):
        H.fulltrain_apply_device(s, 1, 1, 1e-3, 1, betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        H.fulltrain_apply_device(s, 1, 1, 1e-3, 1, decay=1.5)
    with pytest.raises(ValueError):
        H.fulltrain_set_params(s, np.zeros(10, np.float32))
    with pytest.raises(ValueError):
        H.fulltrain_set_opt_state(s, np.zeros(5124067, np.float32), np.zeros(3, np.float32))


def test_losses_from_aux():
    k = 8
    aux = np.zeros(66 * k + 4)
    aux[:k] = [64, 0, 0, 0, 0, 0, 0, 0]
    aux[65 * k:66 * k] = [64 * 64 * 0.5] + [0] * 7
    aux[66 * k] = 64
    aux[66 * k + 1:] = [1536 * 0.25, 1536 * 0.5, 1536]
    r = vec3_full_training.losses_from_aux(aux, k)
    assert r["mse"] == 0.25 and r["l1"] == 0.5 and abs(r["vq_loss"] - 0.25 * 0.5) < 1e-12
    assert abs(r["loss"] - (0.8 * 0.25 + 0.2 * 0.5 + 0.125)) < 1e-12 and r["perplexity"] == pytest.approx(1.0)


def test_adamw_fp64_restatement_is_torch_adamw():
    """tf.adamw_fp64 (the reference of the teacher-forced optimizer test on the GPU) against torch.optim.AdamW on float64
    tensors: two steps, gradients over eight decades with exact zeros, to 1e-12 of |value| + |value before the step|."""
    rng = np.random.default_rng(5)
    n = 4099
    hyper = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
    p = rng.standard_normal(n) * 0.1
    grads = [rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n) for _ in range(2)]
    grads[0][::17] = 0.0
    grads[1][::5] = 0.0
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([tp], **hyper)
    m, v = np.zeros(n), np.zeros(n)
    for step, g in enumerate(grads, 1):
        before = (p, m, v)
        p, m, v = tf.adamw_fp64(p, g, m, v, hyper["lr"], step, hyper["betas"], hyper["eps"], hyper["weight_decay"])
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        st = opt.state[tp]
        assert int(st["step"]) == step
        for name, mine, ref, old in (("p", p, tp.detach().numpy(), before[0]), ("m", m, st["exp_avg"].numpy(), before[1]),
                                     ("v", v, st["exp_avg_sq"].numpy(), before[2])):
            assert (np.abs(mine - ref) <= 1e-12 * (np.abs(ref) + np.abs(old))).all(), (step, name, np.abs(mine - ref).max())
    assert np.abs(m).min() == 0.0 and np.abs(m).max() > 0.0      # elements whose gradient was zero in both steps are in


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def restated():
    W = synth_vec3.make_weights(0)
    params = {k: torch.from_numpy(np.array(W[k], np.float32)) for k in tf.param_names()}
    st = trt.initial_state(W)
    batches = [synth_vec3.make_leaves(32, seed=7000 + s) for s in range(3)]
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    recs = tf.train_steps(batches, params, st)
    return recs, params, st


def test_restatement_reproduces_the_reference_fixture(g, restated):
    recs, params, st = restated
    for s, r in enumerate(recs):
        assert np.array_equal(r["idx"].reshape(-1, 64), g["idx"][s]), s
        assert r["lr"] == pytest.approx(float(g["lr"][s]), rel=1e-12)
        for j, key in enumerate(("loss", "mse", "l1", "vq_loss", "perplexity")):
            assert abs(r[key] - g["loss"][s, j]) <= 1e-5 * abs(g["loss"][s, j]), (s, key, r[key], g["loss"][s, j])
    for i, k in enumerate(tf.param_names()):
        gr = recs[0]["grads"][k].reshape(-1)
        h = min(256, gr.size)
        assert np.abs(gr[:h] - g["g_head"][i, :h]).max() <= 1e-5 * np.abs(gr).max(), k
        assert abs(float((gr.astype(np.float64) ** 2).sum()) - g["g_sq"][i]) <= 1e-5 * g["g_sq"][i] + 1e-30, k
        p = params[k].numpy().reshape(-1)
        d = np.abs(p[:h] - g["p_head"][i, :h])
        lr = float(g["lr"][0])
        assert d.max() <= 6.5 * lr and d.mean() < 0.05 * lr, (k, d.max(), d.mean())
    cs = g["cluster_size"]
    assert (np.abs(st["cluster_size"].numpy() - cs) / np.maximum(np.abs(cs), 1.0)).max() < 1e-6


@pytest.mark.skipif(not os.path.exists(os.path.join(REFERENCE, "VQVAE_v2.py")), reason="no reference checkout to regenerate the fixture from")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, MAKER, "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "reproduced bit for bit" in r.stdout


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _allreduce_rank(rank, world, port, q):
    import torch.distributed as dist
    from vqvdb_amd.codebook_training import allreduce_stats
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    rng = np.random.default_rng(rank)
    grads = torch.from_numpy(rng.standard_normal(1000).astype(np.float32))
    aux = torch.from_numpy(rng.integers(0, 50, 66 * 4 + 4).astype(np.float32))
    allreduce_stats(grads)
    allreduce_stats(aux)
    q.put((rank, grads.numpy(), aux.numpy()))
    dist.destroy_process_group()


def test_two_rank_gloo_allreduce_of_gradients_and_aux():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_allreduce_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict((r, (gr, ax)) for r, gr, ax in (q.get(timeout=120) for _ in range(2)))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    exp_g = sum(np.random.default_rng(r).standard_normal(1000).astype(np.float32) for r in range(2))
    rngs = [np.random.default_rng(r) for r in range(2)]
    for r in rngs:
        r.standard_normal(1000)
    exp_a = sum(r.integers(0, 50, 66 * 4 + 4).astype(np.float32) for r in rngs)
    for r in range(2):
        assert np.allclose(got[r][0], exp_g, rtol=0, atol=1e-6)
        assert np.array_equal(got[r][1], exp_a)
