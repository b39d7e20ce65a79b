"""Torch restatement of the scalar codec's bf16 decode mode — TEST INFRASTRUCTURE.  The mode changes two layers,
decoder.res_stack.0.conv1 and .conv2; this file restates exactly those, from the tensors vqhip_debug_fetch returns
([n, 64 channels, 64 positions], position = (d*4 + h)*4 + w):

  - GroupNorm(8, 64) statistics under §4's 16-block rule in float64: per 4-channel quad and per row of 4 positions one chain from
    zero (positions ascending, channels ascending), the 16 row sums added in row order, a group = low quad + high quad;
    mean and rstd = 1/sqrt(var + 1e-5) rounded to float32 once (``gn_stats``);
  - the transform in float32 with the fp32 path's formula, ``max(fmaf(x, rstd*gamma, fmaf(-mean, rstd*gamma, beta)), 0)``
    (``transform_dtype=torch.float64``: the same in float64, for the flip-cap check);
  - both operands rounded with ``.to(torch.bfloat16)``, products and sums in float64, ``acc + bias`` rounded to float32 once;
    conv2 stores ``skip + 0.1 * (acc + bias)`` with two float32 roundings.  A product of two bf16 numbers is exact in float32,
    so the only difference to the GPU is the order of its float32 accumulation.

``round_operands=False`` leaves the operands alone and accumulates as the fp32 path does (one float32 chain per output, §4's
tap and channel order): the fp32 contract, which tests/test_precision_host.py pins to the oracle.
``tail`` finishes a decode from d_x6 in float64 (attention gate, up conv, pixel shuffle, final conv, sigmoid) for the end-to-end
closeness figures; ``closeness`` compares two decoders."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

import torch_ref as tr

P = "decoder.res_stack.0."


def bf16_bits(x):
    """float32 array -> bf16 bit patterns (uint16): the integer formula of v3b::bf16_bits (vq_bf16.h), round to nearest even,
    NaN kept quiet."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def rb(x):
    """Round to bf16 and back (round to nearest even)."""
    return x.to(torch.bfloat16).to(x.dtype)


def gn_stats(x):
    """x: float32 [n, 64, 64].  (mean, rstd) float32 [n, 8] under the 16-block rule (GnAcc / gn_combine_k<true> / gn_finish)."""
    n = x.shape[0]
    v = np.asarray(x, dtype=np.float64).reshape(n, 16, 4, 16, 4)   # [leaf][quad][channel][block = row][position]
    bs = np.zeros((n, 16, 16))
    bq = np.zeros((n, 16, 16))
    for p in range(4):
        for ch in range(4):
            d = v[:, :, ch, :, p]
            bs = bs + d
            bq = d * d + bq   # fma(d, d, bq): the square of a float32 is exact in float64
    S = np.zeros((n, 16))
    Q = np.zeros((n, 16))
    for b in range(16):
        S = S + bs[:, :, b]
        Q = Q + bq[:, :, b]
    S = S[:, 0::2] + S[:, 1::2]
    Q = Q[:, 0::2] + Q[:, 1::2]
    m = S * (1.0 / 512.0)
    ex2 = Q * (1.0 / 512.0)
    # var = fma(-m, m, ex2): one rounding, through exact rationals
    var = np.array([[float(Fraction(float(ex2[i, g])) - Fraction(float(m[i, g])) ** 2) for g in range(8)] for i in range(n)]).reshape(n, 8)
    var = np.maximum(var, 0.0)
    return m.astype(np.float32), (1.0 / np.sqrt(var + 1e-5)).astype(np.float32)


def transform(x, mean, rstd, gamma, beta, dtype=torch.float32):
    """GroupNorm + ReLU per element.  float32: a = rstd*gamma, b = fmaf(-mean, a, beta), max(fmaf(x, a, b), 0), each fmaf as an
    exact float64 product, a float64 sum and one rounding to float32.  float64: the same expression without the roundings."""
    x = torch.as_tensor(x, dtype=torch.float32).double()
    mean = torch.as_tensor(mean).double().repeat_interleave(8, dim=1)[:, :, None]
    rstd = torch.as_tensor(rstd).double().repeat_interleave(8, dim=1)[:, :, None]
    gamma = torch.as_tensor(gamma, dtype=torch.float32).double()[None, :, None]
    beta = torch.as_tensor(beta, dtype=torch.float32).double()[None, :, None]
    if dtype == torch.float32:
        a = (rstd * gamma).float().double()
        b = (-mean * a + beta).float().double()
        t = (x * a + b).float()
    else:
        a = rstd * gamma
        t = x * a + (-mean * a + beta)
    return torch.clamp_min(t, 0.0)


def _chain_fp32(t, W):
    """The fp32 path's accumulation (§4): one float32 fmaf chain per output, taps ascending (kd,kh,kw), inside a tap the channels
    in P16 order (16-channel blocks ascending, inside a block 0,4,8,12,1,5,...).  Each step is an exact float64 product, a float64
    sum and one rounding to float32; a padding tap adds zero, which leaves the chain as it is."""
    tp_ = F.pad(t.reshape(-1, 64, 4, 4, 4), (1, 1, 1, 1, 1, 1)).double()
    W = W.double()
    acc = torch.zeros((tp_.shape[0], 64, 4, 4, 4), dtype=torch.float32)
    order = [16 * cb + 4 * k + r for cb in range(4) for r in range(4) for k in range(4)]
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                for ci in order:
                    x = tp_[:, ci, kd:kd + 4, kh:kh + 4, kw:kw + 4]
                    acc = (acc.double() + x[:, None] * W[None, :, ci, kd, kh, kw, None, None, None]).float()
    return acc.double()


def _conv(t, w, name, round_operands):
    """conv3d(t, W) + bias on [n, 64, 64], the result rounded to float32 once.  bf16 operands: accumulated in float64 (the GPU's
    float32 accumulation order inside an MFMA is not part of the contract).  Operands as they are: the fp32 path's chain."""
    W = torch.as_tensor(w[P + name + ".weight"], dtype=torch.float32)
    b = torch.as_tensor(w[P + name + ".bias"], dtype=torch.float32)
    if round_operands:
        y = F.conv3d(rb(t).double().reshape(-1, 64, 4, 4, 4), rb(W).double(), None, padding=1)
    else:
        y = _chain_fp32(t, W)
    return (y.reshape(-1, 64, 64) + b.double()[None, :, None]).float()


def conv1(d2, w, transform_dtype=torch.float32, round_operands=True):
    """d_y4 from d_d2 (float32 [n, 64, 64])."""
    mean, rstd = gn_stats(d2)
    t = transform(d2, mean, rstd, w[P + "gn1.weight"], w[P + "gn1.bias"], transform_dtype)
    return _conv(t, w, "conv1", round_operands).numpy()


def conv2(y4, d2, w, transform_dtype=torch.float32, round_operands=True):
    """d_x6 from d_y4 and the skip tensor d_d2."""
    mean, rstd = gn_stats(y4)
    t = transform(y4, mean, rstd, w[P + "gn2.weight"], w[P + "gn2.bias"], transform_dtype)
    v = _conv(t, w, "conv2", round_operands)
    u = v * torch.tensor(0.1, dtype=torch.float32)
    return (torch.as_tensor(d2, dtype=torch.float32) + u).numpy()


def res_block(d2, w, transform_dtype=torch.float32, round_operands=True):
    """(d_y4, d_x6) from d_d2, conv2 fed by this restatement's own d_y4."""
    y4 = conv1(d2, w, transform_dtype, round_operands)
    return y4, conv2(y4, d2, w, transform_dtype, round_operands)


def tail(x6, w):
    """Decoded leaves [n, 512] from d_x6 in float64: attention gate, up conv, pixel shuffle, final conv, sigmoid."""
    w64 = {k: torch.as_tensor(v, dtype=torch.float32).double() for k, v in w.items() if k.startswith("decoder.")}
    a = tr._attention(torch.as_tensor(x6, dtype=torch.float32).double().reshape(-1, 64, 4, 4, 4), w64, "decoder.attn")
    up = F.conv3d(a, w64["decoder.up_conv.weight"], w64["decoder.up_conv.bias"], padding=1)
    pre = F.conv3d(tr.pixel_shuffle3d(up), w64["decoder.final.weight"], w64["decoder.final.bias"], padding=1)
    return torch.sigmoid(pre).reshape(-1, 512).numpy()


def closeness(a, b, x=None):
    """Two decoders' outputs for the same indices (a: the mode under test, b: the baseline), [n, 512]: rms and max of a - b, and
    with the encoded leaves x the ratio of their reconstruction errors mean||x - a||^2 / mean||x - b||^2."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 512), np.asarray(b, dtype=np.float64).reshape(-1, 512)
    d = a - b
    out = {"rms": float(np.sqrt((d * d).mean())), "max": float(np.abs(d).max())}
    if x is not None:
        x = np.asarray(x, dtype=np.float64).reshape(-1, 512)
        out["mse_ratio"] = float(((x - a) ** 2).mean() / ((x - b) ** 2).mean())
    return out


def pair_leaves():
    """The 97 leaves of the end-to-end closeness figures: 89 uniform synthetic leaves and the 8 edge leaves."""
    from vqvdb_amd import synth
    return np.concatenate([synth.make_leaves(89, seed=1234), synth.edge_leaves()])


def ref_pair(oracle, w):
    """REF_PAIR of tests/test_gpu_precision.py: this restatement (bf16 operands, float64 tail) against the oracle's fp32 decode
    on the indices the oracle encodes pair_leaves() to."""
    x = pair_leaves()
    idx = oracle.encode(x)
    rec, dbg = oracle.decode(idx, debug=("d_d2",))
    return closeness(tail(res_block(dbg["d_d2"], w)[1], w), rec, x)
