"""Plain PyTorch restatement of one full training step of the Vec3 model — TEST INFRASTRUCTURE.  Written from the reference
loop (python/training.py: 0.8 F.mse_loss + 0.2 F.l1_loss + vq_loss, loss.backward(), AdamW(lr, betas (0.9, 0.999),
weight_decay 1e-4), CosineAnnealingLR stepped per batch) and VectorQuantizerEMA.forward in training mode
(python/VQVAE_v2.py:107-156: the commitment loss and the straight-through decoder input against the codebook before the
EMA update), in plain fp32 (or fp64) with no autocast.  Functional over a dict of tensors named like the reference's
state_dict, on top of the unchanged torch_ref_vec3 / torch_ref_vec3_train.  The code assignment is an input, so an fp64
autograd evaluation can use the GPU's indices.  Pinned to the imported reference by
tests/golden/make_golden_vec3_fulltrain.py -> tests/test_vec3_fulltrain_host.py."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import torch_ref_vec3 as tr
import torch_ref_vec3_train as trt

COMMITMENT = 0.25
MSE_WEIGHT, L1_WEIGHT = 0.8, 0.2


def param_names() -> list:
    """The 60 tensors of VQVAE(3, 64, K).parameters() in order (the flat vector of vqhip_vec3_fulltrain_*)."""
    names = []
    conv = lambda p: names.extend([p + ".weight", p + ".bias"])  # noqa: E731
    gn = conv

    def rb(p):
        gn(p + ".gn1"), conv(p + ".conv1"), gn(p + ".gn2"), conv(p + ".conv2")

    conv("encoder.pre.0"), gn("encoder.pre.1"), rb("encoder.pre.3"), conv("encoder.down1")
    rb("encoder.res_stack.0"), rb("encoder.res_stack.1")
    names += ["encoder.attn.fc.0.weight", "encoder.attn.fc.2.weight"]
    conv("encoder.proj"), conv("decoder.stem.0"), gn("decoder.stem.1")
    rb("decoder.res_stack.0"), rb("decoder.res_stack.1")
    names += ["decoder.attn.fc.0.weight", "decoder.attn.fc.2.weight"]
    conv("decoder.up_conv"), conv("decoder.final")
    return names


def flatten(params: dict) -> np.ndarray:
    return np.concatenate([np.asarray(params[k], np.float32).reshape(-1) for k in param_names()])


def unflatten(vec: np.ndarray, like: dict) -> dict:
    out, off = {}, 0
    for k in param_names():
        shape = np.asarray(like[k]).shape
        size = int(np.prod(shape))
        out[k] = np.asarray(vec[off:off + size]).reshape(shape)
        off += size
    assert off == len(vec)
    return out


def assign(leaves, w: dict, embedding: torch.Tensor) -> torch.Tensor:
    """The training forward's code assignment (first minimum of the expanded distances) in the given dtype."""
    with torch.no_grad():
        z = tr.encoder(leaves, w)
        flat = trt.flat_of(z)
        e = embedding.to(flat.dtype)
        dist = (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * flat @ e.t()
        return torch.argmin(dist, dim=1)


def loss(leaves, w: dict, embedding: torch.Tensor, idx: torch.Tensor) -> dict:
    """The training loss with a given code assignment idx [n*64] (row = leaf*64 + position); differentiable in w."""
    z = tr.encoder(leaves, w)
    flat = trt.flat_of(z)
    quant = embedding.to(z.dtype)[idx]
    q = quant.reshape(z.shape[0], 64, 64).permute(0, 2, 1).reshape(z.shape)
    vq_loss = COMMITMENT * F.mse_loss(z, q.detach())
    rec = trt.decoder_from_q(z + (q - z).detach(), w)
    x = torch.as_tensor(np.asarray(leaves)).to(z.dtype).reshape(rec.shape)
    mse, l1 = F.mse_loss(rec, x), F.l1_loss(rec, x)
    total = MSE_WEIGHT * mse + L1_WEIGHT * l1 + vq_loss
    return {"loss": total, "mse": mse, "l1": l1, "vq_loss": vq_loss, "rec": rec, "z": z, "flat": flat}


def gradients(leaves, params: dict, embedding, idx, dtype=torch.float64) -> tuple:
    """(loss dict of floats, gradients {name: np.ndarray}) of the loss in `dtype` with the assignment idx."""
    w = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items() if k in set(param_names())}
    e = torch.as_tensor(np.asarray(embedding)).to(dtype)
    out = loss(leaves, w, e, torch.as_tensor(np.asarray(idx, np.int64)))
    out["loss"].backward()
    vals = {k: float(out[k].detach()) for k in ("loss", "mse", "l1", "vq_loss")}
    return vals, {k: w[k].grad.numpy() for k in param_names()}


def adamw_step(params: dict, grads: dict, state: dict, lr: float, step: int, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4):
    """torch.optim.AdamW's update (decoupled weight decay) on float32 tensors, functional; state: name -> (m, v)."""
    b1, b2 = betas
    for k in param_names():
        p, g = params[k], grads[k]
        m, v = state.setdefault(k, (torch.zeros_like(p), torch.zeros_like(p)))
        p.mul_(1 - lr * weight_decay)
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (v.sqrt() / math.sqrt(1 - b2 ** step)).add_(eps)
        p.addcdiv_(m, denom, value=-lr / (1 - b1 ** step))


def adamw_fp64(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4) -> tuple:
    """torch.optim.AdamW's update on flat arrays in numpy float64, functional -> (p, m, v).  Every argument enters with the
    value it is given: hand in float32 arrays and np.float32 scalars to restate a float32 kernel's inputs."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = (float(a) for a in (lr, betas[0], betas[1], eps, weight_decay))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps
    p = p * (1.0 - lr * wd) - (lr / (1.0 - b1 ** step)) * (m / denom)
    return p, m, v


def ema_update(st: dict, flat: torch.Tensor, idx: torch.Tensor, decay: float = 0.95, eps: float = 1e-4):
    """The EMA step of VectorQuantizerEMA (VQVAE_v2.py:135-144) with a given assignment; updates st in place."""
    k = st["embedding"].shape[0]
    enc = F.one_hot(idx, k).to(torch.float32)
    st["cluster_size"].mul_(decay).add_(enc.sum(0), alpha=1 - decay)
    st["embed_avg"].mul_(decay).add_(enc.t() @ flat.to(torch.float32), alpha=1 - decay)
    st["embedding"].copy_(st["embed_avg"] / st["cluster_size"].clamp(min=eps).unsqueeze(1))


def cosine_lr(lr0: float, t: int, t_max: int) -> float:
    """CosineAnnealingLR (eta_min 0) after t scheduler steps, closed form."""
    return lr0 * (1 + math.cos(math.pi * t / t_max)) / 2


def train_steps(batches, params: dict, st: dict, lr0=5e-4, t_max=150, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, decay=0.95,
                ema_eps=1e-4, idx_list=None, lr_list=None) -> list:
    """Steps of the reference loop in fp32 on the CPU: forward (assignment from the live codebook unless idx_list gives it),
    backward, AdamW, EMA, scheduler.  params / st are dicts of float32 tensors, updated in place.  -> per-step records."""
    opt, recs = {}, []
    for s, leaves in enumerate(batches):
        lr = cosine_lr(lr0, s, t_max) if lr_list is None else lr_list[s]
        w = {k: params[k].detach().clone().requires_grad_(True) for k in param_names()}
        e = st["embedding"].clone()
        idx = assign(leaves, w, e) if idx_list is None else torch.as_tensor(np.asarray(idx_list[s], np.int64).reshape(-1))
        out = loss(leaves, w, e, idx)
        out["loss"].backward()
        grads = {k: w[k].grad.detach() for k in param_names()}
        p = torch.bincount(idx, minlength=e.shape[0]).to(torch.float32) / idx.numel()
        perp = float(torch.exp(-torch.sum(p * torch.log(p + 1e-10))))
        ema_update(st, out["flat"].detach(), idx, decay, ema_eps)
        with torch.no_grad():
            adamw_step(params, grads, opt, lr, s + 1, betas, eps, weight_decay)
        recs.append({**{k: float(out[k].detach()) for k in ("loss", "mse", "l1", "vq_loss")},
                     "perplexity": perp, "idx": idx.numpy(), "grads": {k: g.numpy().copy() for k, g in grads.items()}, "lr": lr})
    return recs
