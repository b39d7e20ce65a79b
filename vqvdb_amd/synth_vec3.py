"""Deterministic synthetic weights and leaves for the Vec3 model VQVAE(3, 64, K) (python/VQVAE_v2.py EncoderVec3 /
DecoderVec3).

Same scheme as ``synth``: every value comes from the counter-based ``synth.uniform01`` over ``(seed, stream, element)``,
so any machine regenerates the same bits from numpy alone and any slice can be regenerated on its own.  Scales are
"trained-like" (convs O(1/sqrt(fan_in)), non-identity GroupNorm affine, residual branches at full scale) and the
codebook is spread over the encoder's latent range so that hundreds of the 4096 codes are in use.

Leaves are float32 [n, 512, 3], channels last: voxel offset d*64 + h*8 + w, then x, y, z (an OpenVDB Vec3f leaf buffer).
"""
from __future__ import annotations

import numpy as np

from .synth import uniform01

K_CODES = 4096
D_EMBED = 64


def _conv(name, co, ci, k):
    return [(name + ".weight", (co, ci, k, k, k), "conv"), (name + ".bias", (co,), "bias")]


def _gn(name, ch):
    return [(name + ".weight", (ch,), "gn_w"), (name + ".bias", (ch,), "gn_b")]


def _rb(name, ch):
    return _gn(name + ".gn1", ch) + _conv(name + ".conv1", ch, ch, 3) + _gn(name + ".gn2", ch) + _conv(name + ".conv2", ch, ch, 3)


def tensors(k_codes: int = K_CODES, d_embed: int = D_EMBED):
    """(name, shape, kind) of every inference tensor of VQVAE(3, d_embed, k_codes).state_dict(), in its order."""
    return (_conv("encoder.pre.0", 64, 3, 3) + _gn("encoder.pre.1", 64) + _rb("encoder.pre.3", 64)
            + _conv("encoder.down1", 128, 64, 3) + _rb("encoder.res_stack.0", 128) + _rb("encoder.res_stack.1", 128)
            + [("encoder.attn.fc.0.weight", (32, 128), "fc"), ("encoder.attn.fc.2.weight", (128, 32), "fc")]
            + _conv("encoder.proj", d_embed, 128, 1)
            + _conv("decoder.stem.0", 128, d_embed, 3) + _gn("decoder.stem.1", 128) + _rb("decoder.res_stack.0", 128)
            + _rb("decoder.res_stack.1", 128)
            + [("decoder.attn.fc.0.weight", (32, 128), "fc"), ("decoder.attn.fc.2.weight", (128, 32), "fc")]
            + _conv("decoder.up_conv", 256, 128, 3) + _conv("decoder.final", 3, 32, 3)
            + [("quantizer.embedding", (k_codes, d_embed), "codebook")])


TENSORS = tensors()
CODEBOOK_SCALE = 0.45   # pseudo-normal spread of the codes, matched to the latents of make_leaves (see make_golden_vec3.py)


def make_weights(seed: int = 0, k_codes: int = K_CODES) -> dict[str, np.ndarray]:
    """Synthetic fp32 parameter set with the Vec3 model's names and shapes (K = k_codes codes).  Streams are offset from
    the scalar model's (1000 + tensor id), and the codebook's stream does not depend on K: code i is the same vector for
    every K > i."""
    f = np.float32
    out: dict[str, np.ndarray] = {}
    for tid, (name, shape, kind) in enumerate(tensors(k_codes)):
        n = int(np.prod(shape))
        stream = 1000 + tid + 1
        u = uniform01(seed, stream, n)
        if kind == "conv":
            a = f(np.sqrt(3.0 / int(np.prod(shape[1:]))))
            v = (u * f(2.0) - f(1.0)) * a
        elif kind == "fc":
            a = f(np.sqrt(3.0 / shape[1]))
            v = (u * f(2.0) - f(1.0)) * a
        elif kind == "bias":
            v = (u * f(2.0) - f(1.0)) * f(0.1)
        elif kind == "gn_w":
            v = f(1.0) + (u * f(2.0) - f(1.0)) * f(0.3)
        elif kind == "gn_b":
            v = (u * f(2.0) - f(1.0)) * f(0.2)
        elif kind == "codebook":
            u4 = uniform01(seed, stream, 4 * n).reshape(n, 4).sum(axis=1, dtype=np.float32)
            v = (u4 - f(2.0)) * f(CODEBOOK_SCALE)
        else:  # pragma: no cover
            raise ValueError(kind)
        out[name] = np.ascontiguousarray(v.astype(np.float32).reshape(shape))
    return out


def _grid():
    d, h, w = np.meshgrid(np.arange(8, dtype=np.float32), np.arange(8, dtype=np.float32), np.arange(8, dtype=np.float32), indexing="ij")
    return d.reshape(-1), h.reshape(-1), w.reshape(-1)


def make_leaves(n: int, seed: int = 4321, start: int = 0) -> np.ndarray:
    """``n`` Vec3 leaves [n, 512, 3]: smooth vortex and shear fields (velocity-like), uniform [-1,1]^3 noise, sparse
    leaves (background with a few active voxels), constant vectors, x20 magnitudes and exact zeros.  Leaf i depends only
    on (seed, start + i); float32 arithmetic with correctly rounded operations only, so it regenerates bit for bit."""
    f = np.float32
    d, h, w = _grid()
    out = np.zeros((n, 512, 3), dtype=np.float32)
    for j in range(n):
        i = start + j
        u = uniform01(seed, 11, 16, start=i * 16)
        noise = uniform01(seed, 12, 1536, start=i * 1536).reshape(512, 3) * f(2.0) - f(1.0)
        k = u[0]
        if k < f(0.30):      # vortex around an axis through a centre (possibly outside the leaf), swirl + drift
            c = u[1:4] * f(12.0) - f(2.0)
            s = (u[4] * f(2.0) - f(1.0)) / f(4.0)
            x, y, z = d - c[0], h - c[1], w - c[2]
            ax = int(u[5] * f(3.0)) % 3
            v = [np.zeros(512, np.float32)] * 3
            if ax == 0:
                v = [np.full(512, u[6] * f(0.2), np.float32), -z * s, y * s]
            elif ax == 1:
                v = [z * s, np.full(512, u[6] * f(0.2), np.float32), -x * s]
            else:
                v = [-y * s, x * s, np.full(512, u[6] * f(0.2), np.float32)]
            out[j] = np.stack(v, axis=1)
        elif k < f(0.50):    # shear: velocity along one axis varying linearly along another, plus offset
            a_dir, a_var = int(u[1] * f(3.0)) % 3, int(u[2] * f(3.0)) % 3
            coord = (d, h, w)[a_var]
            out[j, :, a_dir] = (coord - f(3.5)) * (u[3] * f(0.4) - f(0.2)) + (u[4] * f(2.0) - f(1.0))
            out[j, :, (a_dir + 1) % 3] = u[5] * f(0.2) - f(0.1)
        elif k < f(0.65):    # uniform [-1, 1]^3
            out[j] = noise
        elif k < f(0.75):    # sparse: background with 1..8 active voxels
            cnt = 1 + int(u[1] * f(8.0))
            pos = (uniform01(seed, 13, cnt, start=i * 8) * f(512.0)).astype(np.int64) % 512
            out[j, pos] = noise[:cnt]
        elif k < f(0.85):    # constant vector
            out[j] = (u[1:4] * f(2.0) - f(1.0))[None, :]
        elif k < f(0.95):    # x20 magnitudes
            out[j] = noise * f(20.0)
        # else: exact zeros
    return out


def edge_leaves() -> np.ndarray:
    """Edge-case Vec3 leaves [8, 512, 3]: zeros, ones, a single spike, a per-channel ramp in which channel c depends only on
    axis c (x on d, y on h, z on w: detects swapped channels or axes), the ramp with the axes rotated, a large constant,
    tiny noise, and channel-alternating signs."""
    f = np.float32
    d, h, w = _grid()
    e = np.zeros((8, 512, 3), dtype=np.float32)
    e[1] = 1.0
    e[2, 3 * 64 + 4 * 8 + 5] = (f(1.0), f(-0.5), f(0.25))
    e[3] = np.stack([d / f(7.0), h / f(7.0) * f(0.5), w / f(7.0) * f(0.25)], axis=1)
    e[4] = np.stack([w / f(7.0), d / f(7.0) * f(0.5), h / f(7.0) * f(0.25)], axis=1)
    e[5] = (f(15.0), f(-15.0), f(7.5))
    e[6] = (uniform01(99, 14, 1536).reshape(512, 3) * f(2.0) - f(1.0)) * f(1e-3)
    e[7] = np.stack([np.where((d + h + w) % 2 == 0, f(1.0), f(-1.0))] * 3, axis=1) * np.array([1, -1, 1], np.float32)
    return e
