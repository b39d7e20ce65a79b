"""Plain PyTorch restatement of the Vec3 model's inference (VQVAE(3, 64, K): python/VQVAE_v2.py EncoderVec3 /
DecoderVec3 / VQVAE.encode / VQVAE.decode) — TEST INFRASTRUCTURE.  Written from the model's layer table (DESIGN.md §11,
"Model"), functional
style over a dict of tensors named like the reference's state_dict; runs in float32 or float64 on the CPU and returns the
per-layer activations under the names vqhip_vec3_debug_fetch uses.  Pinned to the imported reference by
tests/golden/make_golden_vec3.py -> tests/test_vec3_host.py."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def weights_to_torch(w: dict, dtype=torch.float64) -> dict:
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in w.items()}


def _gn_relu(x, w, prefix, eps=1e-5):
    return F.relu(F.group_norm(x, 8, w[prefix + ".weight"], w[prefix + ".bias"], eps=eps))


def _res_block(x, w, prefix):
    t = F.conv3d(_gn_relu(x, w, prefix + ".gn1"), w[prefix + ".conv1.weight"], w[prefix + ".conv1.bias"], padding=1)
    return x + 0.1 * F.conv3d(_gn_relu(t, w, prefix + ".gn2"), w[prefix + ".conv2.weight"], w[prefix + ".conv2.bias"], padding=1)


def _attention(x, w, prefix):
    m = x.mean(dim=(2, 3, 4))
    g = torch.sigmoid(F.linear(F.relu(F.linear(m, w[prefix + ".fc.0.weight"])), w[prefix + ".fc.2.weight"]))
    return x * g[:, :, None, None, None]


def pixel_shuffle3d(x, r=2):
    b, c, d, h, wd = x.shape
    oc = c // r ** 3
    return x.view(b, oc, r, r, r, d, h, wd).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(b, oc, d * r, h * r, wd * r)


def encoder(leaves, w, acts=None):
    """leaves [n,512,3] channels last -> latents [n,64,4,4,4]."""
    x = torch.as_tensor(leaves).to(w["encoder.pre.0.weight"].dtype).reshape(-1, 8, 8, 8, 3).permute(0, 4, 1, 2, 3)
    rec = (lambda k, t: acts.__setitem__(k, t.detach().clone())) if acts is not None else (lambda k, t: None)
    y = F.conv3d(x, w["encoder.pre.0.weight"], w["encoder.pre.0.bias"], padding=1)
    rec("encoder.pre.0", y)
    a = _gn_relu(y, w, "encoder.pre.1")
    rec("encoder.pre.2", a)
    a = _res_block(a, w, "encoder.pre.3")
    rec("encoder.pre", a)
    a = F.conv3d(a, w["encoder.down1.weight"], w["encoder.down1.bias"], stride=2, padding=1)
    rec("encoder.down1", a)
    for i in range(2):
        a = _res_block(a, w, f"encoder.res_stack.{i}")
        rec(f"encoder.res_stack.{i}", a)
    a = _attention(a, w, "encoder.attn")
    z = F.conv3d(a, w["encoder.proj.weight"], w["encoder.proj.bias"])
    rec("encoder.proj", z)
    return z


def distances(z, w):
    """[n*64, K] expanded distances |z|^2 + |e|^2 - 2 z.e of the flattened latents (position-major, as VQVAE.encode)."""
    flat = z.permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
    e = w["quantizer.embedding"]
    return (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * flat @ e.t()


def encode(leaves, w, acts=None):
    """-> (indices int64 [n,64], distances [n*64, K])."""
    z = encoder(leaves, w, acts)
    dist = distances(z, w)
    return torch.argmin(dist, dim=1).reshape(-1, 64), dist


def decode(indices, w, acts=None):
    """indices [n,64] -> leaves [n,512,3] channels last."""
    rec = (lambda k, t: acts.__setitem__(k, t.detach().clone())) if acts is not None else (lambda k, t: None)
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64)).reshape(-1, 4, 4, 4)
    q = F.embedding(idx, w["quantizer.embedding"]).permute(0, 4, 1, 2, 3)
    y = F.conv3d(q, w["decoder.stem.0.weight"], w["decoder.stem.0.bias"], padding=1)
    rec("decoder.stem.0", y)
    a = _gn_relu(y, w, "decoder.stem.1")
    rec("decoder.stem", a)
    for i in range(2):
        a = _res_block(a, w, f"decoder.res_stack.{i}")
        rec(f"decoder.res_stack.{i}", a)
    a = _attention(a, w, "decoder.attn")
    u = F.conv3d(a, w["decoder.up_conv.weight"], w["decoder.up_conv.bias"], padding=1)
    rec("decoder.up_conv", u)
    out = torch.tanh(F.conv3d(pixel_shuffle3d(u), w["decoder.final.weight"], w["decoder.final.bias"], padding=1))
    return out.permute(0, 2, 3, 4, 1).reshape(-1, 512, 3)


def check_indices_vs_fixture(idx, g, n=None):
    """The index bar: equal where the recorded relative top-2 gap is >= 1e-4, one of the two recorded codes below it,
    at most 1 position in 10 000 off top-1.  Returns (positions off top-1, largest gap at which one was off)."""
    ref, second, gap = g["idx"][:n], g["second"][:n], g["gap"][:n]
    off = idx != ref
    assert not (off & (gap >= 1e-4)).any(), f"index differs at a clear position (gap >= 1e-4): {np.argwhere(off & (gap >= 1e-4))[:5]}"
    assert ((idx == ref) | (idx == second)).all(), "index is neither of the two recorded codes"
    assert off.sum() <= max(1, ref.size // 10000), f"{int(off.sum())} of {ref.size} positions off top-1"
    return int(off.sum()), float(gap[off].max()) if off.any() else 0.0
