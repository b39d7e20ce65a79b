#!/usr/bin/env python3
"""Generate tests/golden/golden_vec3_fulltrain_v1.npz by IMPORTING the reference model VQVAE(3, 64, 4096, 0.25)
(python/VQVAE_v2.py) with synth_vec3.make_weights(0) loaded strict, and running three steps of the reference training loop
(python/training.py) in plain fp32 on the CPU: model forward in training mode, 0.8 F.mse_loss + 0.2 F.l1_loss + vq_loss,
backward, torch.optim.AdamW(lr 5e-4, betas (0.9, 0.999), weight_decay 1e-4), CosineAnnealingLR(T_max 150) stepped per
batch.  No autocast and no clipping (the reference only unscales).

Runs only where a reference checkout and CPU torch are present; the file holds the reference's OUTPUTS only (inputs are
regenerated from synth_vec3).  No reference source is copied.

    python tests/golden/make_golden_vec3_fulltrain.py [--check]

Batches: synth_vec3.make_leaves(32, seed=7000+s), s = 0..2.
  loss          f64 [3,5]      loss, mse, l1, vq_loss, perplexity of each step (the forward's outputs)
  lr            f64 [3]        learning rate of each step (scheduler.get_last_lr before the step)
  idx           u16 [3,32,64]  each step's code assignment
  g_sum, g_sq   f64 [60]       per-tensor sum and sum of squares of step 1's gradients (model.parameters() order)
  g_head        f32 [60,256]   first 256 elements of each of step 1's gradients (zero padded)
  p_sum, p_sq   f64 [60]       per-tensor sum and sum of squares of the parameters after step 3
  p_head        f32 [60,256]   first 256 elements of each parameter after step 3 (zero padded)
  cluster_size  f32 [4096]     after step 3
  emb_sums      f64 [2]        sum and sum of squares of the embedding after step 3
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

OUT = os.path.join(HERE, "golden_vec3_fulltrain_v1.npz")
N_LEAVES, STEPS, SEED, LR, T_MAX, HEAD = 32, 3, 7000, 5e-4, 150, 256


def head(t):
    v = t.detach().reshape(-1)[:HEAD].numpy().astype(np.float32)
    return np.pad(v, (0, HEAD - v.size))


def generate():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    m = build_model()
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=LR, weight_decay=1e-4, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_MAX)
    params = list(m.parameters())
    assert len(params) == 60 and sum(p.numel() for p in params) == 5124067
    out = {"loss": [], "lr": [], "idx": []}
    for s in range(STEPS):
        x = to_model(synth_vec3.make_leaves(N_LEAVES, SEED + s))
        out["lr"].append(sched.get_last_lr()[0])
        e_before = m.quantizer.embedding.clone()
        with torch.no_grad():
            flat = m.encoder_outputs_to_flat(m.encoder(x))
            dist = (flat ** 2).sum(1, keepdim=True) + (e_before ** 2).sum(1) - 2 * flat @ e_before.t()
            out["idx"].append(torch.argmin(dist, dim=1).reshape(-1, 64).numpy().astype(np.uint16))
        opt.zero_grad()
        _, rec, vq_loss, perp = m(x)
        mse, l1 = F.mse_loss(rec, x), F.l1_loss(rec, x)
        loss = 0.8 * mse + 0.2 * l1 + vq_loss
        loss.backward()
        if s == 0:
            g = [p.grad.detach().double() for p in params]
            out["g_sum"] = np.array([t.sum().item() for t in g], np.float64)
            out["g_sq"] = np.array([(t ** 2).sum().item() for t in g], np.float64)
            out["g_head"] = np.stack([head(p.grad) for p in params])
        opt.step()
        sched.step()
        out["loss"].append([loss.item(), mse.item(), l1.item(), vq_loss.item(), perp.item()])
    out["loss"] = np.array(out["loss"], np.float64)
    out["lr"] = np.array(out["lr"], np.float64)
    out["idx"] = np.stack(out["idx"])
    out["p_sum"] = np.array([p.detach().double().sum().item() for p in params], np.float64)
    out["p_sq"] = np.array([(p.detach().double() ** 2).sum().item() for p in params], np.float64)
    out["p_head"] = np.stack([head(p) for p in params])
    out["cluster_size"] = m.quantizer.cluster_size.numpy().astype(np.float32)
    e = m.quantizer.embedding.double()
    out["emb_sums"] = np.array([e.sum().item(), (e ** 2).sum().item()], np.float64)
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    print("losses:", out["loss"][:, 0], "perplexity:", out["loss"][:, 4])
    return out


if __name__ == "__main__":
    data = generate()
    if "--check" in sys.argv:
        ref = np.load(OUT)
        assert sorted(ref.files) == sorted(data), "fixture keys differ"
        for k, v in data.items():
            assert ref[k].dtype == v.dtype and ref[k].shape == v.shape and np.array_equal(ref[k].view(np.uint8), v.view(np.uint8)), f"{k} differs"
        print("golden_vec3_fulltrain_v1.npz reproduced bit for bit")
    else:
        np.savez_compressed(OUT, **data)
        print(f"{OUT}: {os.path.getsize(OUT)} bytes")
