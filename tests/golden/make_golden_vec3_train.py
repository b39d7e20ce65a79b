#!/usr/bin/env python3
"""Generate tests/golden/golden_vec3_train_v1.npz by IMPORTING the reference model VQVAE(3, 64, 4096, 0.25)
(python/VQVAE_v2.py) with synth_vec3.make_weights(0) loaded strict, and running its codebook training pieces:
VectorQuantizerEMA.forward in training mode (:107-156), VQVAE.forward in eval mode (:344-348, as python/training.py:183-199
uses it) and check_and_reset_dead_codes (:382-417).

Runs only where a reference checkout and CPU torch are present; the file holds the reference's OUTPUTS only (inputs are
regenerated from synth_vec3).  No reference source is copied.

    python tests/golden/make_golden_vec3_train.py [--check]

Training: three quantizer steps (decay 0.95, eps 1e-4) on z = encoder(synth_vec3.make_leaves(64, seed=5000+s)), s = 0..2:
  s<s>_idx      u16 [64,64]    nearest codes (before the update)
  s<s>_second   u16 [64,64]    second-nearest codes
  s<s>_gap      f32 [64,64]    relative top-2 gap (d2 - d1) / max(|d1|, |z|^2, 1e-30)
  s<s>_loss     f64 [2]        commitment loss, perplexity (the forward's outputs)
  s<s>_cs       f32 [4096]     cluster_size after the step
  s<s>_used     i32 [u]        codes used by the step
  s<s>_emb      f32 [u,64]     embedding rows of those codes after the step
  s<s>_avg      f32 [u,64]     embed_avg rows of those codes after the step
  z0            f32 [8,64,64]  z of the first 8 leaves of step 0 ([leaf][channel][position])
  final_sums    f64 [3,2]      sum and sum of squares of embedding, cluster_size, embed_avg after step 3 (all 4096 codes;
                               rows of codes no step used follow from the initial buffers, so only these sums are kept)
Eval forward of the untrained model on synth_vec3.make_leaves(64, seed=6000):
  eval_loss     f64 [4]        MSE, L1 (F.mse_loss / F.l1_loss of recon vs x), vq_loss, perplexity
  eval_rec      f32 [8,512,3]  reconstruction of the first 8 leaves (channels last)
Dead-code reset after step 3 from step 3's encoder outputs, torch.manual_seed(1234):
  reset_dead    i64 [d]        dead codes (cluster_size < 1)
  reset_pick    i64 [d]        the drawn rows of flat_z (torch.randint)
--check regenerates everything and compares it bit for bit with the committed file instead of writing it.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("VQVDB_REFERENCE_PYTHON", "/root/reference/python"))

from vqvdb_amd import synth_vec3  # noqa: E402
from make_golden_vec3 import build_model, to_model  # noqa: E402  (imports the reference model)

OUT = os.path.join(HERE, "golden_vec3_train_v1.npz")
N_LEAVES, STEPS, STEP_SEED, EVAL_SEED, RESET_SEED, N_KEEP = 64, 3, 5000, 6000, 1234, 8


def top2(flat, e, idx):
    dist = (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * flat @ e.t()
    top = torch.topk(dist, 2, dim=1, largest=False)
    d1 = dist.gather(1, idx.reshape(-1, 1))[:, 0]
    assert torch.equal(d1, top.values[:, 0]), "the quantizer did not pick a minimum of the distances restated here"
    second = torch.where(top.indices[:, 0] == idx, top.indices[:, 1], top.indices[:, 0])
    d2 = dist.gather(1, second.reshape(-1, 1))[:, 0]
    scale = torch.maximum(torch.maximum(d1.abs(), (flat ** 2).sum(1)), torch.full_like(d1, 1e-30))
    return second, (d2 - d1) / scale


@torch.no_grad()
def generate():
    torch.set_num_threads(8)
    m = build_model()
    q = m.quantizer
    out = {}
    # eval forward of the untrained model first (nothing is updated in eval mode)
    m.eval()
    xe = to_model(synth_vec3.make_leaves(N_LEAVES, EVAL_SEED))
    _, rec, vq_loss, perp = m(xe)
    out["eval_loss"] = np.array([F.mse_loss(rec, xe).item(), F.l1_loss(rec, xe).item(), vq_loss.item(), perp.item()], np.float64)
    out["eval_rec"] = rec[:N_KEEP].permute(0, 2, 3, 4, 1).reshape(-1, 512, 3).numpy().astype(np.float32)

    q.train()
    z = None
    for s in range(STEPS):
        x = to_model(synth_vec3.make_leaves(N_LEAVES, STEP_SEED + s))
        z = m.encoder(x)
        flat = m.encoder_outputs_to_flat(z)
        e_before = q.embedding.clone()
        dist = (flat ** 2).sum(1, keepdim=True) + (e_before ** 2).sum(1) - 2 * flat @ e_before.t()
        idx = torch.argmin(dist, dim=1)
        second, gap = top2(flat, e_before, idx)
        _, loss, perp = q(z)
        used = torch.unique(idx)
        out[f"s{s}_idx"] = idx.reshape(-1, 64).numpy().astype(np.uint16)
        out[f"s{s}_second"] = second.reshape(-1, 64).numpy().astype(np.uint16)
        out[f"s{s}_gap"] = gap.reshape(-1, 64).numpy().astype(np.float32)
        out[f"s{s}_loss"] = np.array([loss.item(), perp.item()], np.float64)
        out[f"s{s}_cs"] = q.cluster_size.numpy().astype(np.float32)
        out[f"s{s}_used"] = used.numpy().astype(np.int32)
        out[f"s{s}_emb"] = q.embedding[used].numpy().astype(np.float32)
        out[f"s{s}_avg"] = q.embed_avg[used].numpy().astype(np.float32)
        if s == 0:
            out["z0"] = z[:N_KEEP].reshape(N_KEEP, 64, 64).numpy().astype(np.float32)
    out["final_sums"] = np.array([[b.double().sum().item(), (b.double() ** 2).sum().item()]
                                  for b in (q.embedding, q.cluster_size, q.embed_avg)], np.float64)

    # check_and_reset_dead_codes draws torch.randint(0, rows, (n_dead,)) right after finding the dead codes
    dead = torch.where(q.cluster_size < 1.0)[0]
    torch.manual_seed(RESET_SEED)
    pick = torch.randint(0, N_LEAVES * 64, (len(dead),))
    torch.manual_seed(RESET_SEED)
    m.check_and_reset_dead_codes(z)
    flat = m.encoder_outputs_to_flat(z)
    assert torch.equal(q.embedding[dead], flat[pick]) and torch.equal(q.embed_avg[dead], flat[pick]), "reset draw not restated"
    assert bool((q.cluster_size[dead] == 1.0).all())
    out["reset_dead"] = dead.numpy().astype(np.int64)
    out["reset_pick"] = pick.numpy().astype(np.int64)
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    print("codes used per step:", [len(out[f"s{s}_used"]) for s in range(STEPS)], "dead codes reset:", len(dead),
          "positions with gap < 1e-3:", [int((out[f"s{s}_gap"] < 1e-3).sum()) for s in range(STEPS)])
    return out


if __name__ == "__main__":
    data = generate()
    if "--check" in sys.argv:
        ref = np.load(OUT)
        assert sorted(ref.files) == sorted(data), "fixture keys differ"
        for k, v in data.items():
            assert ref[k].dtype == v.dtype and ref[k].shape == v.shape and np.array_equal(ref[k].view(np.uint8), v.view(np.uint8)), f"{k} differs"
        print("golden_vec3_train_v1.npz reproduced bit for bit")
    else:
        np.savez_compressed(OUT, **data)
        print(f"{OUT}: {os.path.getsize(OUT)} bytes")
