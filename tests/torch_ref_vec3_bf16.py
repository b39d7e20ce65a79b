"""Torch restatement of the Vec3 model's bf16-operand inference mode — TEST INFRASTRUCTURE.  The layer
table is tests/torch_ref_vec3.py's; what changes is the arithmetic of every MFMA convolution:

  - both operands are rounded to bf16 (round to nearest even, ``x.to(torch.bfloat16)``): the weight as it is, the activation
    after the fused input transform (GroupNorm + ReLU, attention gate) has been evaluated in float32 with the per-element
    formula of the kernels' fill loop, ``((x - mean) * rstd) * gamma + beta`` and ``x * gate``, every step rounded to float32;
  - the convolution then runs in float64 on the rounded operands: a product of two bf16 numbers is exact in float32, so
    the only difference to the GPU is the order of its float32 accumulation;
  - bias, ``res + 0.1 y``, GroupNorm statistics, attention gates, the codebook search and the final conv + tanh are not
    matrix operands of that mode: they run in ``w``'s dtype exactly as torch_ref_vec3 does.

``transform_dtype=torch.float64`` evaluates the transforms in float64 instead (the flip-cap check: how many activations sit
within an ulp of a bf16 rounding boundary).  Per-stage functions (``STAGES``) compute one debug-fetch layer from the one
before it, for the teacher-forced GPU test."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import torch_ref_vec3 as tr


def rb(x):
    """Round to bf16 and back (round to nearest even)."""
    return x.to(torch.bfloat16).to(x.dtype)


def conv_bf16(x, w, prefix, stride=1, padding=1):
    """conv3d with both operands rounded to bf16, accumulated in float64, + bias; result in x's dtype."""
    y = F.conv3d(rb(x).double(), rb(w[prefix + ".weight"]).double(), None, stride=stride, padding=padding)
    return (y + w[prefix + ".bias"].double()[None, :, None, None, None]).to(x.dtype)


def _butterfly(s):
    """gn_stats_k's xor-butterfly over the 32 lanes (float32 adds; every lane ends with the same sum)."""
    lane = torch.arange(32)
    for m in (16, 8, 4, 2, 1):
        s = s + s[..., lane ^ m]
    return s[..., :1]


def gn_stats(x, eps=1e-5):
    """GroupNorm(8) mean and rstd per (leaf, group) as [n, 8, 1] float32, in the arithmetic of the statistics kernel
    (v3::gn_stats_k): lane j of 32 sums elements j, j + 32, ... of the group in order, a xor-butterfly merges the
    lanes; two passes (mean, then fmaf-accumulated squared deviations, biased), rstd = 1 / sqrt(var + eps), all float32."""
    g = x.float().reshape(x.shape[0], 8, -1)
    ng = g.shape[2]
    g = g.reshape(x.shape[0], 8, ng // 32, 32)
    s = torch.zeros_like(g[:, :, 0])
    for i in range(ng // 32):
        s = s + g[:, :, i]
    mean = _butterfly(s) / torch.tensor(float(ng), dtype=torch.float32)
    q = torch.zeros_like(s)
    for i in range(ng // 32):
        d = (g[:, :, i] - mean).double()
        q = (d * d + q.double()).float()   # fmaf: the square is exact in float64
    var = _butterfly(q) / torch.tensor(float(ng), dtype=torch.float32)
    # sqrtf and the float32 division, each through float64 and rounded once (for one operation on float32 inputs that is the
    # correctly rounded float32 result), so that no host's vectorised float32 sqrt / reciprocal decides the last bit
    t = (var.double() + float(np.float32(eps))).float()
    root = torch.from_numpy(np.sqrt(t.double().numpy())).float()
    return mean, torch.from_numpy(1.0 / root.double().numpy()).float()


def gn_relu(x, w, prefix, transform_dtype=torch.float32):
    """relu(GroupNorm(8)(x)) with the kernels' per-element formula in transform_dtype (statistics: gn_stats, float32)."""
    t = transform_dtype
    mean, rstd = gn_stats(x)
    n, c = x.shape[:2]
    v = x.to(t).reshape(n, 8, -1)
    v = ((v - mean.to(t)) * rstd.to(t)).reshape(n, c, -1)
    v = v * w[prefix + ".weight"].to(t)[None, :, None] + w[prefix + ".bias"].to(t)[None, :, None]
    return torch.clamp_min(v, 0.0).reshape(x.shape).to(x.dtype)


def _fma_chain(wm, v):
    """t[., c] = fmaf(wm[c, k], v[., k], t) for k in order, float32 (the product is exact in float64)."""
    t = torch.zeros(v.shape[0], wm.shape[0], dtype=torch.float32)
    wd, vd = wm.float().double(), v.double()
    for k in range(wm.shape[1]):
        t = (wd[None, :, k] * vd[:, k, None] + t.double()).float()
    return t


def gates(x, w, prefix):
    """ChannelAttention gates [n, C] float32 in the arithmetic of v3::se_k: mean = sequential float32 sum over the positions
    / 64, both fc layers as fmaf chains in input order, ReLU between, 1 / (1 + exp(-t))."""
    v = x.float().reshape(x.shape[0], x.shape[1], -1)
    s = torch.zeros_like(v[:, :, 0])
    for p in range(v.shape[2]):
        s = s + v[:, :, p]
    m = s / torch.tensor(float(v.shape[2]), dtype=torch.float32)
    h = torch.clamp_min(_fma_chain(w[prefix + ".fc.0.weight"], m), 0.0)
    t = _fma_chain(w[prefix + ".fc.2.weight"], h)
    den = (1.0 + torch.exp(-t)).double().numpy()   # expf is the host's; the division is rounded once from float64
    return torch.from_numpy(1.0 / den).float()


def gated(x, w, prefix, transform_dtype=torch.float32):
    t = transform_dtype
    g = gates(x, w, prefix).to(x.dtype)   # the gates are stored as float32 on the device
    return (x.to(t) * g.to(t)[:, :, None, None, None]).to(x.dtype)


def res_block(x, w, prefix, transform_dtype=torch.float32):
    h = conv_bf16(gn_relu(x, w, prefix + ".gn1", transform_dtype), w, prefix + ".conv1")
    return x + 0.1 * conv_bf16(gn_relu(h, w, prefix + ".gn2", transform_dtype), w, prefix + ".conv2")


def leaves_to_ncdhw(leaves, w):
    return torch.as_tensor(leaves).to(w["encoder.pre.0.weight"].dtype).reshape(-1, 8, 8, 8, 3).permute(0, 4, 1, 2, 3)


def _shape(a, ch, s):
    return torch.as_tensor(a).reshape(-1, ch, s, s, s)


# one debug-fetch layer from the previous fetch point: name -> (previous name, function(previous, w, transform_dtype))
STAGES = {
    "encoder.pre.0": ("leaves", lambda x, w, t: conv_bf16(leaves_to_ncdhw(x, w), w, "encoder.pre.0")),
    "encoder.pre.2": ("encoder.pre.0", lambda x, w, t: gn_relu(_shape(x, 64, 8).to(w["encoder.pre.0.weight"].dtype), w, "encoder.pre.1", torch.float32)),
    "encoder.pre": ("encoder.pre.2", lambda x, w, t: res_block(_shape(x, 64, 8), w, "encoder.pre.3", t)),
    "encoder.down1": ("encoder.pre", lambda x, w, t: conv_bf16(_shape(x, 64, 8), w, "encoder.down1", stride=2)),
    "encoder.res_stack.0": ("encoder.down1", lambda x, w, t: res_block(_shape(x, 128, 4), w, "encoder.res_stack.0", t)),
    "encoder.res_stack.1": ("encoder.res_stack.0", lambda x, w, t: res_block(_shape(x, 128, 4), w, "encoder.res_stack.1", t)),
    "encoder.proj": ("encoder.res_stack.1", lambda x, w, t: conv_bf16(gated(_shape(x, 128, 4), w, "encoder.attn", t), w, "encoder.proj", padding=0)),
    "decoder.stem.0": ("codes", lambda x, w, t: conv_bf16(_shape(x, 64, 4), w, "decoder.stem.0")),
    "decoder.stem": ("decoder.stem.0", lambda x, w, t: gn_relu(_shape(x, 128, 4), w, "decoder.stem.1", torch.float32)),
    "decoder.res_stack.0": ("decoder.stem", lambda x, w, t: res_block(_shape(x, 128, 4), w, "decoder.res_stack.0", t)),
    "decoder.res_stack.1": ("decoder.res_stack.0", lambda x, w, t: res_block(_shape(x, 128, 4), w, "decoder.res_stack.1", t)),
    "decoder.up_conv": ("decoder.res_stack.1", lambda x, w, t: conv_bf16(gated(_shape(x, 128, 4), w, "decoder.attn", t), w, "decoder.up_conv")),
}
ENCODER_STAGES = [k for k in STAGES if k.startswith("encoder.")]
DECODER_STAGES = [k for k in STAGES if k.startswith("decoder.")]


def stage(name, prev, w, transform_dtype=torch.float32):
    """Layer `name` [n, C, positions] from its previous fetch point (STAGES[name][0]) as float tensors of w's dtype."""
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(prev)).to(w["encoder.pre.0.weight"].dtype)
        y = STAGES[name][1](x, w, transform_dtype)
    return y.reshape(y.shape[0], y.shape[1], -1)


def encoder(leaves, w, acts=None, transform_dtype=torch.float32):
    """leaves [n,512,3] -> latents [n,64,4,4,4]; acts collects the debug-fetch layers."""
    x = leaves
    for name in ENCODER_STAGES:
        x = STAGES[name][1](x, w, transform_dtype)
        if acts is not None:
            acts[name] = x.detach().clone()
    return x


def encode(leaves, w, acts=None, transform_dtype=torch.float32):
    """-> (indices int64 [n,64], distances [n*64, K]); the search is torch_ref_vec3's (not a matrix operand of the mode)."""
    z = encoder(leaves, w, acts, transform_dtype)
    dist = tr.distances(z, w)
    return torch.argmin(dist, dim=1).reshape(-1, 64), dist


def codes(indices, w):
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64)).reshape(-1, 4, 4, 4)
    return F.embedding(idx, w["quantizer.embedding"]).permute(0, 4, 1, 2, 3)


def decode(indices, w, acts=None, transform_dtype=torch.float32):
    """indices [n,64] -> leaves [n,512,3] channels last."""
    x = codes(indices, w)
    for name in DECODER_STAGES:
        x = STAGES[name][1](x, w, transform_dtype)
        if acts is not None:
            acts[name] = x.detach().clone()
    out = torch.tanh(F.conv3d(tr.pixel_shuffle3d(x), w["decoder.final.weight"], w["decoder.final.bias"], padding=1))
    return out.permute(0, 2, 3, 4, 1).reshape(-1, 512, 3)


def closeness(leaves, w, enc_a, dec_a, enc_b, dec_b):
    """The four end-to-end quantities of pair (a, b) = (bf16, fp32): share of differing indices, RMS and maximum voxel
    difference of decode(encode(x)), ratio of mean |x - decode(encode(x))|^2 (a over b).  enc_* -> indices, dec_* -> voxels."""
    x = np.asarray(leaves, dtype=np.float64)
    ia, ib = np.asarray(enc_a(leaves)), np.asarray(enc_b(leaves))
    ra, rbb = np.asarray(dec_a(ia), dtype=np.float64), np.asarray(dec_b(ib), dtype=np.float64)
    d = ra - rbb
    return {"index_share": float((ia != ib).mean()), "rms": float(np.sqrt((d ** 2).mean())), "max": float(np.abs(d).max()),
            "mse_ratio": float(((x - ra) ** 2).mean() / ((x - rbb) ** 2).mean())}
