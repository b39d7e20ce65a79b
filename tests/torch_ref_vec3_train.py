"""Plain PyTorch restatement of the Vec3 model's codebook training pieces — TEST INFRASTRUCTURE.  Written from
VectorQuantizerEMA's training-mode forward (python/VQVAE_v2.py:107-156: expanded distances, first minimum, EMA of
cluster_size / embed_avg, embedding = embed_avg / clamp(cluster_size, eps), commitment loss and perplexity) and from
VQVAE.forward in eval mode (:344-348: decoder on the straight-through value z + (e - z)).  float32 on the CPU, over the
reference's buffer names.  Pinned to the imported reference by tests/golden/make_golden_vec3_train.py ->
tests/test_vec3_training_host.py, and the yardstick of tests/test_gpu_vec3_training.py."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import torch_ref_vec3 as tr


def initial_state(w: dict) -> dict:
    """The buffers a pack's model starts training with: embedding, cluster_size = ones, embed_avg = embedding."""
    e = torch.from_numpy(np.array(w["quantizer.embedding"], dtype=np.float32))
    return {"embedding": e.clone(), "cluster_size": torch.ones(e.shape[0]), "embed_avg": e.clone()}


def flat_of(z: torch.Tensor) -> torch.Tensor:
    """[n,64,4,4,4] (or [n,64,64]) -> the reference's flat rows [n*64, 64], row = leaf*64 + position."""
    return z.reshape(z.shape[0], 64, 64).permute(0, 2, 1).reshape(-1, 64).contiguous()


@torch.no_grad()
def quantizer_step(flat: torch.Tensor, st: dict, decay: float = 0.95, eps: float = 1e-4, commitment_cost: float = 0.25,
                   train: bool = True) -> dict:
    """One forward of the quantizer on flat rows; updates `st` in place when train.  -> idx, vq_loss, perplexity."""
    e = st["embedding"]
    dist = (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * flat @ e.t()
    idx = torch.argmin(dist, dim=1)
    enc = F.one_hot(idx, e.shape[0]).to(flat.dtype)
    quant = enc @ e
    if train:
        st["cluster_size"].mul_(decay).add_(enc.sum(0), alpha=1 - decay)
        st["embed_avg"].mul_(decay).add_(enc.t() @ flat, alpha=1 - decay)
        st["embedding"].copy_(st["embed_avg"] / st["cluster_size"].clamp(min=eps).unsqueeze(1))
    loss = commitment_cost * F.mse_loss(flat, quant)
    p = enc.mean(0)
    return {"idx": idx, "vq_loss": float(loss), "perplexity": float(torch.exp(-torch.sum(p * torch.log(p + 1e-10)))), "quantized": quant}


def decoder_from_q(q: torch.Tensor, w: dict) -> torch.Tensor:
    """DecoderVec3 on a decoder input [n,64,4,4,4] -> leaves [n,512,3] channels last."""
    y = F.conv3d(q, w["decoder.stem.0.weight"], w["decoder.stem.0.bias"], padding=1)
    a = tr._gn_relu(y, w, "decoder.stem.1")
    for i in range(2):
        a = tr._res_block(a, w, f"decoder.res_stack.{i}")
    a = tr._attention(a, w, "decoder.attn")
    u = F.conv3d(a, w["decoder.up_conv.weight"], w["decoder.up_conv.bias"], padding=1)
    out = torch.tanh(F.conv3d(tr.pixel_shuffle3d(u), w["decoder.final.weight"], w["decoder.final.bias"], padding=1))
    return out.permute(0, 2, 3, 4, 1).reshape(-1, 512, 3)


@torch.no_grad()
def eval_forward(leaves: np.ndarray, w: dict, st: dict) -> dict:
    """VQVAE.forward in eval mode: mse, l1, vq_loss, perplexity and the reconstruction [n,512,3]."""
    z = tr.encoder(leaves, w)
    flat = flat_of(z)
    r = quantizer_step(flat, st, train=False)
    q = r["quantized"].reshape(z.shape[0], 64, 64).permute(0, 2, 1).reshape(z.shape)
    rec = decoder_from_q(z + (q - z), w)
    x = torch.from_numpy(np.asarray(leaves, dtype=np.float32)).reshape(rec.shape)
    return {"mse": float(F.mse_loss(rec, x)), "l1": float(F.l1_loss(rec, x)), "vq_loss": r["vq_loss"], "perplexity": r["perplexity"],
            "rec": rec.numpy()}


def stats_fp64(flat: np.ndarray, idx: np.ndarray, emb: np.ndarray) -> np.ndarray:
    """The statistics buffer [66K+1] in fp64 from one-hot products: counts, dw = onehot^T flat, sum |z-e|^2 per code, rows."""
    k = emb.shape[0]
    flat = np.asarray(flat, np.float64).reshape(-1, 64)
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    out = np.zeros(66 * k + 1, np.float64)
    out[:k] = np.bincount(idx, minlength=k)
    dw = np.zeros((k, 64), np.float64)
    order = np.argsort(idx, kind="stable")
    codes, first = np.unique(idx[order], return_index=True)
    if len(codes):
        dw[codes] = np.add.reduceat(flat[order], first, axis=0)
    out[k:65 * k] = dw.reshape(-1)
    out[65 * k:66 * k] = np.bincount(idx, weights=((flat - np.asarray(emb, np.float64)[idx]) ** 2).sum(1), minlength=k)
    out[66 * k] = flat.shape[0]
    return out
