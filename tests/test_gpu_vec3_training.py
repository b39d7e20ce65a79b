"""Vec3 codebook training on the GPU: the reference's three-step schedule and eval forward (fixture), statistics against an
fp64 one-hot evaluation on ragged, skewed and single-hot-code batches, determinism, live search tables after updates
(bit-identical to a fresh handle), checkpoint resume, error paths, the trainer + epoch driver with pack export, and a
two-rank rehearsal on one device."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3_train as trt  # noqa: E402
from vqvdb_amd import synth_vec3, vec3_training, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vec3_train_v1.npz")
K = synth_vec3.K_CODES
NF = 66 * K + 1


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def W():
    return synth_vec3.make_weights(0)


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(float(np.abs(np.asarray(b, np.float64)).max()), 1e-30))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_stats(c, leaves, stream=0, eval_mode=False):
    """-> stats [NF] (host), indices [n,64], flat latent [n*64,64] of one training-mode statistics call."""
    n = leaves.shape[0]
    x = dev(leaves)
    st = torch.zeros(NF, dtype=torch.float32, device="cuda")
    idx = torch.zeros((max(n, 1), 64), dtype=torch.int16, device="cuda")
    lat = torch.zeros((max(n, 1) * 64, 64), dtype=torch.float32, device="cuda")
    c.train_vq_stats_device(x.data_ptr(), n, st.data_ptr(), idx.data_ptr(), lat.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return st.cpu().numpy(), idx.cpu().numpy().view(np.uint16)[:n], lat.cpu().numpy()[:n * 64]


def update(c, stats, decay=0.95, eps=1e-4):
    s = dev(np.asarray(stats, np.float32))
    c.train_vq_update_device(s.data_ptr(), decay, eps)
    torch.cuda.synchronize()


def fixture_leaves():
    return np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])


def test_reference_schedule_three_steps(g, W):
    c = HipVec3Codec(weightpack.dumps(W))
    c.train_begin()
    flipped = False
    for s in range(3):
        stats, idx, lat = run_stats(c, synth_vec3.make_leaves(64, seed=5000 + s))
        if s == 0:
            z = lat.reshape(64, 64, 64)[:8].transpose(0, 2, 1)   # [leaf][channel][position]
            assert rel(z, g["z0"]) < 1e-5
        off = idx != g[f"s{s}_idx"]
        assert not (off & (g[f"s{s}_gap"] >= 1e-3)).any(), f"step {s}: index differs at a clear position"
        flipped |= bool(off.any())
        assert stats[66 * K] == 4096
        m = vec3_training.metrics_from_stats(stats, K)
        if not flipped:
            assert abs(m["vq_loss"] - g[f"s{s}_loss"][0]) <= 1e-4 * g[f"s{s}_loss"][0]
            assert abs(m["perplexity"] - g[f"s{s}_loss"][1]) <= 1e-4 * g[f"s{s}_loss"][1]
        update(c, stats)
        st = c.train_get_state()
        if not flipped:
            used = g[f"s{s}_used"]
            assert rel(st["cluster_size"], g[f"s{s}_cs"]) < 1e-5
            assert rel(st["embed_avg"][used], g[f"s{s}_avg"]) < 1e-5
            assert rel(st["embedding"][used], g[f"s{s}_emb"]) < 1e-5
    if not flipped:
        sums = np.array([[b.astype(np.float64).sum(), (b.astype(np.float64) ** 2).sum()] for b in (st["embedding"], st["cluster_size"], st["embed_avg"])])
        assert np.allclose(sums, g["final_sums"], rtol=1e-5, atol=1e-3)
    c.close()


def hot_pack(W):
    """Every code but 0 moved far away: every latent row goes to code 0."""
    t = dict(W)
    e = np.array(W["quantizer.embedding"], np.float32)
    e[1:] += 100.0
    t["quantizer.embedding"] = e
    return weightpack.dumps(t)


def skewed_leaves():
    base = synth_vec3.make_leaves(600, seed=77)
    rng = np.random.default_rng(3)
    return np.ascontiguousarray(np.concatenate([np.repeat(base[:3], 300, axis=0), base[rng.integers(0, 600, 700)]]))


@pytest.mark.parametrize("case", ["n1", "n129", "n4099", "skewed", "identical16384"])
def test_stats_against_fp64_onehot(W, case):
    if case == "identical16384":
        c = HipVec3Codec(hot_pack(W))
        leaves = np.ascontiguousarray(np.repeat(synth_vec3.make_leaves(1, seed=9), 16384, axis=0))
    else:
        c = HipVec3Codec(weightpack.dumps(W))
        leaves = skewed_leaves() if case == "skewed" else synth_vec3.make_leaves(int(case[1:]), seed=11)
    c.train_begin()
    stats, idx, lat = run_stats(c, leaves)
    emb = c.train_get_state()["embedding"]
    ref = trt.stats_fp64(lat, idx, emb)
    assert np.array_equal(stats[:K], ref[:K]), "counts"
    assert stats[66 * K] == leaves.shape[0] * 64
    assert rel(stats[K:65 * K], ref[K:65 * K]) < 1e-5, "dw"
    assert rel(stats[65 * K:66 * K], ref[65 * K:66 * K]) < 1e-5, "squared error"
    if case == "identical16384":
        assert stats[0] == 1048576
    # deterministic: the same bits on a repeat and on a caller's stream
    again, _, _ = run_stats(c, leaves)
    assert np.array_equal(again.view(np.uint32), stats.view(np.uint32))
    s = torch.cuda.Stream()
    other, _, _ = run_stats(c, leaves, stream=s.cuda_stream)
    assert np.array_equal(other.view(np.uint32), stats.view(np.uint32))
    c.close()


def test_zero_leaves_writes_zero_stats(W):
    c = HipVec3Codec(weightpack.dumps(W))
    c.train_begin()
    st = torch.full((NF,), 7.0, device="cuda")
    sums = torch.full((3,), 7.0, device="cuda")
    c.train_vq_stats_device(0, 0, st.data_ptr())
    c.train_eval_device(0, 0, st.data_ptr(), sums.data_ptr())
    torch.cuda.synchronize()
    assert not st.any() and not sums.any()
    c.close()


def test_live_tables_match_a_fresh_handle(W):
    leaves = fixture_leaves()
    c = HipVec3Codec(weightpack.dumps(W))
    before = c.encode(leaves)
    c.train_begin()
    assert np.array_equal(c.encode(leaves), before)
    for s in range(3):
        stats, _, _ = run_stats(c, synth_vec3.make_leaves(64, seed=5000 + s))
        update(c, stats)
    idx = c.encode(leaves)
    rec = c.decode(idx)
    t = dict(W)
    t["quantizer.embedding"] = c.train_get_state()["embedding"]
    fresh = HipVec3Codec(weightpack.dumps(t))
    assert np.array_equal(fresh.encode(leaves), idx)
    assert np.array_equal(fresh.decode(idx).view(np.uint32), rec.view(np.uint32))
    assert not np.array_equal(idx, before)   # the codebook did move
    c.close()
    fresh.close()


def test_eval_forward_against_fixture(g, W):
    c = HipVec3Codec(weightpack.dumps(W))
    c.train_begin()
    leaves = synth_vec3.make_leaves(64, seed=6000)
    x = dev(leaves)
    st = torch.zeros(NF, device="cuda")
    sums = torch.zeros(3, device="cuda")
    rec = torch.zeros((64, 512, 3), device="cuda")
    c.train_eval_device(x.data_ptr(), 64, st.data_ptr(), sums.data_ptr(), rec.data_ptr())
    torch.cuda.synchronize()
    sq, ab, elems = sums.cpu().numpy().astype(np.float64)
    assert elems == 64 * 1536
    assert abs(sq / elems - g["eval_loss"][0]) <= 1e-5 * g["eval_loss"][0]
    assert abs(ab / elems - g["eval_loss"][1]) <= 1e-5 * g["eval_loss"][1]
    m = vec3_training.metrics_from_stats(st.cpu().numpy(), K)
    assert abs(m["vq_loss"] - g["eval_loss"][2]) <= 1e-4 * g["eval_loss"][2]
    assert abs(m["perplexity"] - g["eval_loss"][3]) <= 1e-4 * g["eval_loss"][3]
    assert np.abs(rec.cpu().numpy()[:8] - g["eval_rec"]).max() < 1e-5
    # without a reconstruction buffer: the same sums; nothing was updated
    sums2 = torch.zeros(3, device="cuda")
    c.train_eval_device(x.data_ptr(), 64, st.data_ptr(), sums2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(sums, sums2)
    assert np.array_equal(c.train_get_state()["embedding"], np.asarray(W["quantizer.embedding"], np.float32))
    c.close()


def test_checkpoint_resume_is_bit_exact(W):
    batches = [synth_vec3.make_leaves(96, seed=7000 + s) for s in range(4)]
    a = HipVec3Codec(weightpack.dumps(W))
    a.train_begin()
    for b in batches:
        update(a, run_stats(a, b)[0])
    straight = a.train_get_state()
    b1 = HipVec3Codec(weightpack.dumps(W))
    b1.train_begin()
    for b in batches[:2]:
        update(b1, run_stats(b1, b)[0])
    mid = b1.train_get_state()
    b1.close()
    b2 = HipVec3Codec(weightpack.dumps(W))
    b2.train_begin()
    b2.train_set_state(**mid)
    for b in batches[2:]:
        update(b2, run_stats(b2, b)[0])
    resumed = b2.train_get_state()
    for k in straight:
        assert np.array_equal(straight[k].view(np.uint32), resumed[k].view(np.uint32)), k
    a.close()
    b2.close()


def test_error_paths_leave_the_handle_usable(W):
    c = HipVec3Codec(weightpack.dumps(W))
    lib, h = c._lib, c._h
    x = dev(synth_vec3.make_leaves(4, seed=1))
    st = torch.zeros(NF, device="cuda")
    sums = torch.zeros(3, device="cuda")
    assert lib.vqhip_vec3_train_vq_stats_device(h, x.data_ptr(), 4, st.data_ptr(), None, None, None) == -1
    assert "train_begin" in lib.vqhip_vec3_last_error(h).decode()
    assert lib.vqhip_vec3_train_eval_device(h, x.data_ptr(), 4, st.data_ptr(), sums.data_ptr(), None, None) == -1
    assert lib.vqhip_vec3_train_vq_update_device(h, st.data_ptr(), 0.9, 1e-4, None) == -1
    assert lib.vqhip_vec3_train_get_state(h, None, None, None) == -1
    assert lib.vqhip_vec3_train_set_state(h, None, None, None) == -1
    assert lib.vqhip_vec3_train_begin(h, None, None) == 0
    assert lib.vqhip_vec3_train_vq_stats_device(h, x.data_ptr(), 4, None, None, None, None) == -1
    assert "stats_dev" in lib.vqhip_vec3_last_error(h).decode()
    assert lib.vqhip_vec3_train_vq_stats_device(h, x.data_ptr(), -1, st.data_ptr(), None, None, None) == -1
    assert lib.vqhip_vec3_train_vq_stats_device(h, x.data_ptr(), c.chunk_leaves() + 1, st.data_ptr(), None, None, None) == -1
    assert "chunk" in lib.vqhip_vec3_last_error(h).decode()
    assert lib.vqhip_vec3_train_eval_device(h, x.data_ptr(), 4, st.data_ptr(), None, None, None) == -1
    for decay, eps in ((-0.5, 1e-4), (1.5, 1e-4), (float("nan"), 1e-4), (0.9, 0.0), (0.9, -1.0)):
        assert lib.vqhip_vec3_train_vq_update_device(h, st.data_ptr(), decay, eps, None) == -1
    assert lib.vqhip_vec3_train_vq_update_device(h, None, 0.9, 1e-4, None) == -1
    # still usable: a full step and encode agree with a handle that never saw the errors
    leaves = synth_vec3.make_leaves(4, seed=1)
    update(c, run_stats(c, leaves)[0])
    ok = HipVec3Codec(weightpack.dumps(W))
    ok.train_begin()
    update(ok, run_stats(ok, leaves)[0])
    assert np.array_equal(c.encode(fixture_leaves()), ok.encode(fixture_leaves()))
    c.close()
    ok.close()


def test_trainer_and_epoch_driver_export_pack(W, tmp_path):
    pack = tmp_path / "vec3.vqw"
    weightpack.save(str(pack), W)
    model = tmp_path / "q.npz"
    out = vec3_training.main(["train", "--pack", str(pack), "--synthetic_leaves", "4096", "--batch_size", "512", "--epochs", "2",
                              "--log_every", "1", "--model_path", str(model), "--export-pack"])
    assert len(out["history"]) == 2 and out["steps_per_epoch"] == 4
    for r in out["history"]:
        assert np.isfinite(r["val_loss"]) and r["codes_used"] > 0
    final = dict(np.load(str(tmp_path / "q_final.npz")))
    exported = HipVec3Codec(str(tmp_path / "q_final.vqw"))
    live = HipVec3Codec(str(pack))
    live.train_begin()
    live.train_set_state(final["quantizer.embedding"], final["quantizer.cluster_size"], final["quantizer.embed_avg"])
    leaves = fixture_leaves()
    assert np.array_equal(exported.encode(leaves), live.encode(leaves))
    assert not np.array_equal(final["quantizer.embedding"], np.asarray(W["quantizer.embedding"], np.float32))
    exported.close()
    live.close()


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
    t = vec3_training.Vec3CodebookTrainer(c, group=dist.group.WORLD)
    counts = []
    for b in batches:
        half = len(b) // world
        t.step(torch.from_numpy(np.ascontiguousarray(b[rank * half:(rank + 1) * half])).cuda())
        counts.append(t.stats.cpu().numpy()[:K].copy())
    q.put((rank, counts, c.train_get_state()))
    c.close()
    dist.destroy_process_group()


def test_two_rank_rehearsal_on_one_device(W):
    batches = [synth_vec3.make_leaves(128, seed=8000 + s) for s in range(2)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rehearsal_rank, args=(r, 2, port, batches, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict((r, (cnt, st)) for r, cnt, st in (q.get(timeout=300) for _ in range(2)))
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    c = HipVec3Codec(weightpack.dumps(W))
    t = vec3_training.Vec3CodebookTrainer(c)
    for i, b in enumerate(batches):
        t.step(torch.from_numpy(b).cuda())
        one = t.stats.cpu().numpy()[:K]
        for r in range(2):
            assert np.array_equal(got[r][0][i], one), f"step {i} rank {r}: counts"
    single = c.train_get_state()
    for r in range(2):
        for k in single:
            assert rel(got[r][1][k], single[k]) < 1e-5, (r, k)
    c.close()
