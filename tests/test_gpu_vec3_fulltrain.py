"""Vec3 full training on the GPU: the training forward against inference and the eval forward, all 60 parameter gradients
against fp64 autograd, three AdamW + EMA steps against the torch restatement and against the reference fixture, live
weight tables after training (bit-identical to a fresh handle from the exported pack), determinism, a two-rank rehearsal
on one device, bit-exact checkpoint resume, error paths and the epoch driver with pack export."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
import torch_ref_vec3_fulltrain as tf  # noqa: E402
import torch_ref_vec3_train as trt  # noqa: E402
from vec3_fulltrain_common import _screen, dev, forward, fwdbwd, new_codec, split  # noqa: E402
from vqvdb_amd import synth_vec3, vec3_full_training, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

VQHIP_ERR_INVALID = -1

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_fulltrain_v1.npz")
K = synth_vec3.K_CODES
NAMES = tf.param_names()


@pytest.fixture(scope="module")
def W():
    return synth_vec3.make_weights(0)


def gpu_steps(c, batches, lrs):
    """Steps of the device loop (fwdbwd + apply on one rank): per step the loss record (from aux) and the assignment."""
    recs = []
    for s, b in enumerate(batches):
        idx, _ = forward(c, b)
        x = dev(b)
        g = torch.zeros(c.fulltrain_param_count(), dtype=torch.float32, device="cuda")
        a = torch.zeros(c.fulltrain_aux_floats(), dtype=torch.float32, device="cuda")
        c.fulltrain_fwdbwd_device(x.data_ptr(), len(b), len(b), g.data_ptr(), a.data_ptr())
        c.fulltrain_apply_device(g.data_ptr(), a.data_ptr(), lrs[s], s + 1)
        torch.cuda.synchronize()
        r = vec3_full_training.losses_from_aux(a.cpu().numpy(), K)
        r["idx"], r["grads"] = idx, g.cpu().numpy()
        recs.append(r)
    return recs


def test_sizes(W):
    c = new_codec(W)
    assert c.fulltrain_param_count() == 5124067 and c.fulltrain_decoder_offset() == 2235712
    assert c.fulltrain_aux_floats() == 66 * K + 4
    assert np.array_equal(c.fulltrain_get_params(), vec3_full_training.state_to_vec(W))
    c.close()


def test_forward_consistency(W):
    leaves = synth_vec3.make_leaves(96, seed=9100)
    c = new_codec(W)
    c.debug_enable(True)
    idx, rec = forward(c, leaves)
    layers = {k: c.debug_fetch(k, len(leaves)) for k in ("encoder.pre.0", "encoder.pre", "encoder.down1", "encoder.res_stack.1",
                                                          "encoder.proj", "decoder.stem", "decoder.res_stack.1", "decoder.up_conv")}
    x = dev(leaves)
    ie = torch.zeros((len(leaves), 64), dtype=torch.int16, device="cuda")
    c.encode_device(x.data_ptr(), len(leaves), ie.data_ptr())
    st = torch.zeros(66 * K + 1, dtype=torch.float32, device="cuda")
    sums = torch.zeros(3, dtype=torch.float32, device="cuda")
    re = torch.zeros((len(leaves), 512, 3), dtype=torch.float32, device="cuda")
    c.train_eval_device(x.data_ptr(), len(leaves), st.data_ptr(), sums.data_ptr(), re.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(idx, ie.cpu().numpy().view(np.uint16)), "forward indices differ from vqhip_vec3_encode_device"
    assert np.array_equal(rec.view(np.uint32), re.cpu().numpy().view(np.uint32)), "forward recon differs from train_eval_device"
    acts = {}
    w = tr.weights_to_torch(W)
    tr.encoder(leaves, w, acts)
    tr.decode(idx, w, acts)
    for k, v in layers.items():
        ref = acts[k].numpy().reshape(v.shape)
        err = float(np.abs(v - ref).max() / np.abs(ref).max())
        assert err < 1e-5, f"{k}: {err}"
    c.close()


def test_parameter_gradients_against_fp64_autograd(W):
    cand = synth_vec3.make_leaves(128, seed=9200)
    c = new_codec(W)
    idx, _ = forward(c, cand)
    keep = _screen(cand, W, idx)[:32]
    leaves = np.ascontiguousarray(cand[keep])
    g, aux = fwdbwd(c, leaves)
    idx_b, _ = forward(c, leaves)
    params = {k: np.asarray(W[k]) for k in NAMES}
    vals64, g64 = tf.gradients(leaves, params, W["quantizer.embedding"], idx_b.reshape(-1), torch.float64)
    vals32, g32 = tf.gradients(leaves, params, W["quantizer.embedding"], idx_b.reshape(-1), torch.float32)
    gpu = split(g)
    worst = 0.0
    for k in NAMES:
        ref = g64[k].reshape(-1)
        scale = max(float(np.abs(ref).max()), 1e-30)
        err = float(np.abs(gpu[k] - ref).max()) / scale
        err32 = float(np.abs(g32[k].reshape(-1) - ref).max()) / scale
        print(f"{k:40s} gpu {err:.2e}  torch fp32 {err32:.2e}")
        worst = max(worst, err)
        assert err < 1e-5, f"{k}: {err}"
    print(f"worst parameter-gradient error {worst:.2e} (bar 1e-5)")
    loss = vec3_full_training.losses_from_aux(aux, K)
    assert abs(loss["loss"] - vals64["loss"]) / vals64["loss"] < 1e-5
    c.close()


def test_three_steps_against_torch_and_live_tables(W, tmp_path):
    batches = [synth_vec3.make_leaves(64, seed=9300 + s) for s in range(3)]
    lrs = [tf.cosine_lr(5e-4, s, 150) for s in range(3)]
    c = new_codec(W)
    recs = gpu_steps(c, batches, lrs)
    params = {k: torch.from_numpy(np.array(W[k], np.float32)) for k in NAMES}
    st = trt.initial_state(W)
    ref = tf.train_steps(batches, params, st, idx_list=[r["idx"] for r in recs], lr_list=lrs)
    for s in range(3):
        assert abs(recs[s]["loss"] - ref[s]["loss"]) / ref[s]["loss"] < 2e-5, (s, recs[s]["loss"], ref[s]["loss"])
    got = split(c.fulltrain_get_params())
    for k in NAMES:
        d = np.abs(got[k] - params[k].numpy().reshape(-1))
        assert d.max() <= 6.5 * lrs[0] and d.mean() < 0.05 * lrs[0], (k, d.max(), d.mean())
    state = c.train_get_state()
    assert np.abs(state["embedding"] - st["embedding"].numpy()).max() < 1e-4
    cs = st["cluster_size"].numpy()
    assert (np.abs(state["cluster_size"] - cs) / np.maximum(np.abs(cs), 1.0)).max() < 1e-6
    # live tables: encode / decode of the trained handle equal a fresh handle built from the exported pack
    pack = tmp_path / "base.vqw"
    weightpack.save(str(pack), W)
    vec3_full_training.export_pack(str(pack), {**vec3_full_training.vec_to_state(c.fulltrain_get_params()),
                                               **{f"quantizer.{k}": v for k, v in state.items()}}, str(tmp_path / "out.vqw"))
    fresh = HipVec3Codec(str(tmp_path / "out.vqw"))
    leaves = synth_vec3.make_leaves(520, seed=9400)
    i1, i2 = c.encode(leaves), fresh.encode(leaves)
    assert np.array_equal(i1, i2)
    assert np.array_equal(c.decode(i1).view(np.uint32), fresh.decode(i1).view(np.uint32))
    fresh.close()
    c.close()


def test_reference_fixture(W):
    g = np.load(GOLDEN)
    batches = [synth_vec3.make_leaves(32, seed=7000 + s) for s in range(3)]
    c = new_codec(W)
    recs = gpu_steps(c, batches, list(g["lr"]))
    for s in range(3):
        assert np.array_equal(recs[s]["idx"], g["idx"][s]), f"step {s}: assignment differs from the reference"
        assert abs(recs[s]["loss"] - g["loss"][s, 0]) / g["loss"][s, 0] < 2e-5, (s, recs[s]["loss"], g["loss"][s, 0])
        assert abs(recs[s]["perplexity"] - g["loss"][s, 4]) / g["loss"][s, 4] < 1e-5
    g0 = split(recs[0]["grads"])
    p = split(c.fulltrain_get_params())
    lr = float(g["lr"][0])
    for i, k in enumerate(NAMES):
        h = min(256, g0[k].size)
        assert np.abs(g0[k][:h] - g["g_head"][i, :h]).max() <= 1e-5 * np.abs(g0[k]).max(), k
        assert abs(float((g0[k].astype(np.float64) ** 2).sum()) - g["g_sq"][i]) <= 1e-5 * g["g_sq"][i] + 1e-30, k
        d = np.abs(p[k][:h] - g["p_head"][i, :h])
        assert d.max() <= 6.5 * lr and d.mean() < 0.05 * lr, (k, d.max(), d.mean())
    cs = g["cluster_size"]
    assert (np.abs(c.train_get_state()["cluster_size"] - cs) / np.maximum(np.abs(cs), 1.0)).max() < 1e-6
    c.close()


def test_determinism_across_calls_and_streams(W):
    leaves = synth_vec3.make_leaves(200, seed=9500)
    c = new_codec(W)
    g1, a1 = fwdbwd(c, leaves, 300)
    g2, a2 = fwdbwd(c, leaves, 300)
    s = torch.cuda.Stream()
    g3, a3 = fwdbwd(c, leaves, 300, stream=s.cuda_stream)
    for g, a in ((g2, a2), (g3, a3)):
        assert np.array_equal(g1.view(np.uint32), g.view(np.uint32)) and np.array_equal(a1.view(np.uint32), a.view(np.uint32))
    c.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rehearsal_rank(rank, world, port, batches, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    c = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0)))
    t = vec3_full_training.Vec3FullTrainer(c, group=dist.group.WORLD)
    g1 = None
    for b in batches:
        half = len(b) // world
        t.step(torch.from_numpy(np.ascontiguousarray(b[rank * half:(rank + 1) * half])).cuda())
        g1 = t.grads.cpu().numpy().copy() if g1 is None else g1   # step 1's all-reduced gradient
    q.put((rank, c.fulltrain_get_params(), c.train_get_state()["embedding"], g1))
    c.close()
    dist.destroy_process_group()


def test_two_rank_rehearsal_on_one_device(W):
    batches = [synth_vec3.make_leaves(64, seed=9600 + s) for s in range(3)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rehearsal_rank, args=(r, 2, port, batches, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict((r, (pv, e, g1)) for r, pv, e, g1 in (q.get(timeout=300) for _ in range(2)))
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)), "ranks' parameters differ"
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), "ranks' codebooks differ"
    c = HipVec3Codec(weightpack.dumps(W))
    t = vec3_full_training.Vec3FullTrainer(c)
    g1 = None
    for b in batches:
        t.step(torch.from_numpy(b).cuda())
        g1 = t.grads.cpu().numpy().copy() if g1 is None else g1
    # the gradient sums are grouped differently: step 1's summed gradient agrees to 1e-6 of each tensor's largest value
    ga, gb = split(got[0][2]), split(g1)
    for k in NAMES:
        assert np.abs(ga[k] - gb[k]).max() <= 1e-6 * max(np.abs(gb[k]).max(), 1e-30), k
    # AdamW's step divides by sqrt(v) + eps, so the last-bit differences of near-zero gradient elements grow into small
    # parameter differences over the three steps (measured 4.6e-6 norm-relative, largest 0.18 lr)
    single = c.fulltrain_get_params().astype(np.float64)
    d = got[0][0].astype(np.float64) - single
    rel_norm = float(np.linalg.norm(d) / np.linalg.norm(single))
    print(f"2 ranks vs 1: parameter norm-relative difference {rel_norm:.2e}, largest element difference {np.abs(d).max():.2e}")
    assert rel_norm <= 2e-5 and np.abs(d).max() <= 0.5 * 5e-4
    e = c.train_get_state()["embedding"].astype(np.float64)
    assert np.linalg.norm(got[0][1] - e) / np.linalg.norm(e) <= 1e-5
    c.close()


def test_checkpoint_resume_is_bit_exact(W):
    batches = [synth_vec3.make_leaves(48, seed=9700 + s) for s in range(4)]
    c = HipVec3Codec(weightpack.dumps(W))
    t = vec3_full_training.Vec3FullTrainer(c)
    t.t_max = 20
    for b in batches[:2]:
        t.step(torch.from_numpy(b).cuda())
    ck = {k: np.array(v, copy=True) for k, v in t.checkpoint().items()}
    for b in batches[2:]:
        t.step(torch.from_numpy(b).cuda())
    a_params, a_state = c.fulltrain_get_params(), c.train_get_state()
    c2 = HipVec3Codec(weightpack.dumps(W))
    t2 = vec3_full_training.Vec3FullTrainer(c2)
    t2.load_checkpoint(ck)
    for b in batches[2:]:
        t2.step(torch.from_numpy(b).cuda())
    assert np.array_equal(a_params.view(np.uint32), c2.fulltrain_get_params().view(np.uint32))
    b_state = c2.train_get_state()
    for k in a_state:
        assert np.array_equal(a_state[k].view(np.uint32), b_state[k].view(np.uint32)), k
    c.close()
    c2.close()


def test_error_paths_leave_the_handle_usable(W):
    import ctypes
    leaves = synth_vec3.make_leaves(16, seed=9800)
    c = HipVec3Codec(weightpack.dumps(W))
    lib, h = c._lib, c._h
    x = dev(leaves)
    g = torch.zeros(5124067, dtype=torch.float32, device="cuda")
    a = torch.zeros(66 * K + 4, dtype=torch.float32, device="cuda")
    assert lib.vqhip_vec3_fulltrain_fwdbwd_device(h, x.data_ptr(), 16, 16, g.data_ptr(), a.data_ptr(), None, None) == VQHIP_ERR_INVALID
    assert lib.vqhip_vec3_fulltrain_apply_device(h, g.data_ptr(), a.data_ptr(), ctypes.c_float(1e-3), 1, ctypes.c_float(0.9),
                                                 ctypes.c_float(0.999), ctypes.c_float(1e-8), ctypes.c_float(0.0), ctypes.c_float(0.95),
                                                 ctypes.c_float(1e-4), None) == VQHIP_ERR_INVALID
    c.fulltrain_begin()
    c.set_chunk_leaves(8)
    assert lib.vqhip_vec3_fulltrain_fwdbwd_device(h, x.data_ptr(), 16, 16, g.data_ptr(), a.data_ptr(), None, None) == VQHIP_ERR_INVALID
    c.set_chunk_leaves(1024)
    assert lib.vqhip_vec3_fulltrain_fwdbwd_device(h, x.data_ptr(), 16, 8, g.data_ptr(), a.data_ptr(), None, None) == VQHIP_ERR_INVALID
    assert lib.vqhip_vec3_fulltrain_fwdbwd_device(h, x.data_ptr(), 16, 16, None, a.data_ptr(), None, None) == VQHIP_ERR_INVALID
    g.fill_(1.0)
    a.fill_(1.0)
    assert lib.vqhip_vec3_fulltrain_fwdbwd_device(h, x.data_ptr(), 0, 16, g.data_ptr(), a.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert float(g.abs().sum()) == 0.0 and float(a.abs().sum()) == 0.0
    fresh = HipVec3Codec(weightpack.dumps(W))
    assert np.array_equal(c.encode(leaves), fresh.encode(leaves))
    fresh.close()
    c.close()


def test_epoch_driver_exports_the_trained_model(W, tmp_path):
    pack = tmp_path / "vec3.vqw"
    weightpack.save(str(pack), W)
    model = tmp_path / "m.npz"
    out = vec3_full_training.main(["train", "--pack", str(pack), "--synthetic_leaves", "2048", "--batch_size", "256", "--epochs", "2",
                                   "--log_every", "1", "--model_path", str(model), "--export-pack"])
    h = out["history"]
    assert len(h) == 2 and out["steps_per_epoch"] == 4
    assert h[1]["train_loss"] < h[0]["train_loss"], [r["train_loss"] for r in h]
    final = dict(np.load(str(tmp_path / "m_final.npz")))
    exported = HipVec3Codec(str(tmp_path / "m_final.vqw"))
    live = HipVec3Codec(str(pack))
    live.fulltrain_begin()
    live.fulltrain_set_params(final["params"])
    live.train_set_state(final["quantizer.embedding"], final["quantizer.cluster_size"], final["quantizer.embed_avg"])
    leaves = synth_vec3.make_leaves(300, seed=9900)
    i1 = exported.encode(leaves)
    assert np.array_equal(i1, live.encode(leaves))
    assert np.array_equal(exported.decode(i1).view(np.uint32), live.decode(i1).view(np.uint32))
    assert not np.array_equal(final["params"], vec3_full_training.state_to_vec(W))
    exported.close()
    live.close()
