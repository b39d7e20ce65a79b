"""Shared helpers of tests/test_gpu_precision_regimes.py and tests/test_precision_regimes_host.py — TEST INFRASTRUCTURE
(DESIGN.md §23): the index rows per weight regime, a per-element bound on |bf16 kernel - restatement| for the two convs
(``conv_bound``), the restatement with deliberate defects (``restate``), the float64 tail behind d_x6 in two parts, and the
planted weight sets whose conv results are one float32 number under any accumulation order (``planted_weights`` /
``closed_form``)."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import torch_ref as tr
import torch_ref_precision as tp
from vqvdb_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = tp.P
REGIMES = ["seed0", "seed1", "seed2", "trained", "deadcodes", "default"]
U = 2.0 ** -24          # unit roundoff of float32
ACC_C = 1729            # any-order bound for the float32 sum of 1728 exact products and the bias: gamma_n <= n u / (1 - n u)
WIN_C = 8               # see conv_bound
SLACK = 1.0 + 2.0 ** -12   # second-order terms (u^2, c u * flip) of the three first-order terms
C01 = float(np.float32(0.1))
N_ROWS = 37


@functools.lru_cache(maxsize=1)
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_regimes_v1.npz"))


@functools.lru_cache(maxsize=None)
def weights_of(regime):
    from test_golden_regimes import regime_weights
    return regime_weights(fixture(), regime)


@functools.lru_cache(maxsize=None)
def oracle_of(regime):
    from oracle.oracle import Oracle
    return Oracle(weights_of(regime), [t[0] for t in synth.TENSORS])


@functools.lru_cache(maxsize=None)
def rows(regime):
    """The 37 index rows of a regime (one full tile and a half tile holding 5 leaves): 12 of the uniform, 12 of the sparse and
    all 8 of the edge leaves' encodings, one random row over 0..255, and 4 rows with code (64 r + p) mod 256 at position p, which
    hold every code once.  seed0 has no rows in the regimes fixture: its uniform and edge rows come from golden_v1.npz, its
    sparse rows from the oracle's encoding of the same sparse leaves."""
    if regime == "seed0":
        g = np.load(os.path.join(ROOT, "tests", "golden", "golden_v1.npz"))
        uni, edge = g["idx_rand"][:12], g["idx_edge"]
        spa = oracle_of("seed0").encode(synth.sparse_leaves(12, seed=9002))
    else:
        fx = fixture()
        uni, spa, edge = fx[f"{regime}/idx_uniform"][:12], fx[f"{regime}/idx_sparse"][:12], fx[f"{regime}/idx_edge"]
    rand = np.random.default_rng(2323).integers(0, 256, (1, 64))
    every = (64 * np.arange(4)[:, None] + np.arange(64)[None, :]) % 256
    out = np.ascontiguousarray(np.concatenate([uni, spa, edge, rand, every]).astype(np.uint8))
    assert out.shape == (N_ROWS, 64) and len(np.unique(out[-4:])) == 256
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- the two convs: restatement with options, and the bound

def _abs_conv(t, W):
    return F.conv3d(t.reshape(-1, 64, 4, 4, 4), W, None, padding=1).reshape(-1, 64, 64)


def trunc_bf16(x):
    """float32 tensor -> bf16 by dropping the low 16 bits (the 'weights truncated' defect)."""
    u = x.contiguous().view(torch.int32) & -65536
    return u.view(torch.float32)


def restate(in_tensor, w, gn, conv, skip=None, transform_dtype=torch.float32, mutant=None):
    """d_y4 (gn1 / conv1) or d_x6 (gn2 / conv2 with ``skip``) as tests/torch_ref_precision.py states them; ``mutant`` plants
    one defect a kernel could have:
      "trunc_w"    weights truncated to bf16 instead of rounded;
      "no_round"   neither operand rounded;
      "zero_w"     the weight (co 21, ci 42, tap (0,0,0)) taken as zero;
      "swap_kd_kw" the weight's kd and kw axes exchanged;
      "wrap_pad"   the padding tap (kd,kh,kw) = (1,1,0) of the 16 output positions with w = 0 reads the position before in
                   memory order (w = 3 of the row before; the last position for position 0) instead of being skipped."""
    mean, rstd = tp.gn_stats(in_tensor)
    t = tp.transform(in_tensor, mean, rstd, w[P + gn + ".weight"], w[P + gn + ".bias"], transform_dtype)
    W = torch.as_tensor(w[P + conv + ".weight"], dtype=torch.float32)
    b = torch.as_tensor(w[P + conv + ".bias"], dtype=torch.float32).double()
    tb = t.double() if mutant == "no_round" else tp.rb(t).double()
    Wb = W.double() if mutant == "no_round" else (trunc_bf16(W) if mutant == "trunc_w" else tp.rb(W)).double()
    if mutant == "zero_w":
        Wb = Wb.clone()
        Wb[21, 42, 0, 0, 0] = 0.0
    if mutant == "swap_kd_kw":
        Wb = Wb.permute(0, 1, 4, 3, 2).contiguous()
    y = _abs_conv(tb, Wb)
    if mutant == "wrap_pad":
        t5 = tb.reshape(-1, 64, 64)
        extra = torch.einsum("oc,ncp->nop", Wb[:, :, 1, 1, 0], torch.roll(t5, 1, dims=2))   # input position p - 1
        at_w0 = (torch.arange(64) % 4 == 0).double()[None, None, :]
        y = y + extra * at_w0
    v = (y + b[None, :, None]).float()
    if skip is None:
        return v.numpy()
    return (torch.as_tensor(skip, dtype=torch.float32) + v * torch.tensor(0.1, dtype=torch.float32)).numpy()


def bf16_ulp(v):
    """The spacing of bf16 numbers in the binade of v > 0 (float64 array); 0 for v <= 0."""
    out = np.zeros_like(v)
    pos = v > 0
    out[pos] = 2.0 ** (np.floor(np.log2(v[pos])) - 7)
    return out


def conv_bound(in_tensor, weights, gn, conv, skip=None, parts=False):
    """Per output element of [n, 64, 64] an upper bound on |GPU - restatement| of d64b::conv_k that any kernel meeting the
    contract of DESIGN §23 stays inside, whatever the order of its float32 accumulation.  With u = 2^-24:

    accumulation  ACC_C u (sum |rb(t)| |rb(W)| + |bias|) over the valid taps, ACC_C = 1729: the 1728 products are exact in
                  float32, the kernel adds them and the bias with 1728 rounded additions in some order, and the error of such
                  a sum is at most gamma_1728 = 1728 u / (1 - 1728 u) < 1729 u times the sum of the magnitudes.
    flip          sum jump_k |rb(W_k)| over the inputs k whose bf16 rounding may differ between two correct evaluations of
                  the transform.  The transform in exact arithmetic on the float64 statistics is pre = x a + (-m a + beta),
                  a = rstd gamma.  The kernel evaluates a32 = fl(rstd' gamma), b32 = fl(-m' a32 + beta),
                  fl(x a32 + b32) with m', rstd' within one float32 ulp (relative 2u) of tp.gn_stats: a32 = a (1 + 3u),
                  b32 is off by 5u |m a| from the factors and u (|m a| + |beta|) from its rounding, the last fma adds
                  3u |x a| and u (|x a| + |m a| + |beta|): 4u |x a| + 7u |m a| + 2u |beta| in all, to first order.
                  win = WIN_C u (|x a| + |m a| + |beta|) with WIN_C = 8 covers it with the second-order terms; the
                  restatement's own float32 transform (m' = m) lies inside the same window.  Both values are in
                  [pre - win, pre + win], rounding is monotone, so they round alike unless that interval holds a bf16 tie
                  point (pre > 0) or zero (where ReLU cuts): an input is 'near' when rb(max(pre - win, 0)) differs from
                  rb(max(pre + win, 0)).  A near input moves by at most jump = max(bf16 ulp at pre + win, 2 win):
                  an interval shorter than a bf16 ulp holds one tie point, so the two roundings are neighbours; a longer
                  one occurs only below 2^9 win, next to zero, where the two values are 2 win apart before rounding.
    rounding      u |ref| for the restatement's one rounding of acc + bias; for conv2 the value v = acc + bias passes two more
                  roundings on either side, fl(0.1f v) and fl(skip + .): the bound on v times 0.1f, plus 2u |0.1f v| and
                  2u |skip + 0.1f v|.

    The sum is multiplied by 1 + 2^-12 for the second-order terms.  ``parts``: also the terms, the mass
    sum |products| + |bias| and the share of near inputs."""
    x = np.asarray(in_tensor, dtype=np.float32).astype(np.float64)
    mean, rstd = tp.gn_stats(in_tensor)
    m = np.repeat(mean.astype(np.float64), 8, axis=1)[:, :, None]
    a = np.repeat(rstd.astype(np.float64), 8, axis=1)[:, :, None] * weights[P + gn + ".weight"].astype(np.float64)[None, :, None]
    beta = weights[P + gn + ".bias"].astype(np.float64)[None, :, None]
    pre = x * a + (-m * a + beta)
    win = WIN_C * U * (np.abs(x * a) + np.abs(m * a) + np.abs(beta))
    lo, hi = np.maximum(pre - win, 0.0), np.maximum(pre + win, 0.0)
    rt = tp.rb(torch.from_numpy(np.maximum(pre, 0.0)))
    near = (tp.rb(torch.from_numpy(lo)) != tp.rb(torch.from_numpy(hi))).numpy()
    jump = np.where(near, np.maximum(bf16_ulp(hi), 2.0 * win), 0.0)
    W = tp.rb(torch.as_tensor(weights[P + conv + ".weight"], dtype=torch.float32)).double()
    b = weights[P + conv + ".bias"].astype(np.float64)[None, :, None]
    mass = _abs_conv(rt.abs(), W.abs()).numpy() + np.abs(b)
    flip = _abs_conv(torch.from_numpy(jump), W.abs()).numpy()
    v = _abs_conv(rt, W).numpy() + b
    acc = ACC_C * U * mass
    rnd = U * (np.abs(v) + flip)
    bound = acc + flip + rnd
    if skip is not None:
        out = np.asarray(skip, dtype=np.float32).astype(np.float64) + C01 * v
        rnd2 = 2.0 * U * C01 * (np.abs(v) + bound) + 2.0 * U * (np.abs(out) + C01 * bound)
        bound, mass, acc, flip, rnd = C01 * bound + rnd2, C01 * mass, C01 * acc, C01 * flip, C01 * rnd + rnd2
    bound = SLACK * bound
    if parts:
        return bound, {"acc": acc, "flip": flip, "rnd": rnd, "mass": mass, "near_share": float(near.mean())}
    return bound


def ratios(got, ref, bound, mass):
    """(largest err / bound, largest err / (u * mass), elements over their bound)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float((err / bound).max()), float((err / (U * mass)).max()), int((err > bound).sum())


# ---------------------------------------------------------------- the tail behind d_x6

def tail_parts(x6, w):
    """(d_x7 [n, 64, 64], voxels [n, 512]) from d_x6 in float64: tests/torch_ref_precision.tail with the gated tensor kept."""
    w64 = {k: torch.as_tensor(v, dtype=torch.float32).double() for k, v in w.items() if k.startswith("decoder.")}
    a = tr._attention(torch.as_tensor(x6, dtype=torch.float32).double().reshape(-1, 64, 4, 4, 4), w64, "decoder.attn")
    up = F.conv3d(a, w64["decoder.up_conv.weight"], w64["decoder.up_conv.bias"], padding=1)
    pre = F.conv3d(tr.pixel_shuffle3d(up), w64["decoder.final.weight"], w64["decoder.final.bias"], padding=1)
    return a.reshape(-1, 64, 64).numpy(), torch.sigmoid(pre).reshape(-1, 512).numpy()


def distance(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return {"rms": float(np.sqrt((d * d).mean())), "max": float(np.abs(d).max())}


def ref_tail(regime):
    """REF_TAIL[regime] of tests/test_gpu_precision_regimes.py: the fp32 path's own distance from the float64 tail, the
    oracle's d_x7 and voxels on rows(regime) against tail_parts(the oracle's d_x6)."""
    w = weights_of(regime)
    rec, dbg = oracle_of(regime).decode(rows(regime), debug=("d_x6", "d_x7"))
    x7, vox = tail_parts(dbg["d_x6"], w)
    return {"d_x7": distance(dbg["d_x7"], x7), "voxels": distance(rec, vox)}


# ---------------------------------------------------------------- the exact case: planted ties

E_W, E_T = -4, 0                 # binades of the planted weights and activations
QUANTUM = 2.0 ** (E_W - 7 + E_T - 7)   # every product and every bias is a whole multiple of it
M_MAX = 15                       # mantissa field of the planted values: 0 .. 15, so a rounded operand is (128 .. 144) 2^(E - 7)
LIVE_SETS = 3                    # planted set r keeps the channels c = r (mod 3) positive: 22, 21, 21 live input channels
BIAS_MAX = 1000


def _tie(m, e, d=0):
    """float32 bits of (1 + m/128 + 1/256) 2^e, the midpoint of the bf16 numbers with mantissa m and m + 1, moved by d ulps."""
    base = ((127 + e) << 23) | (np.asarray(m, dtype=np.int64) << 16) | 0x8000
    return (base + np.asarray(d, dtype=np.int64)).astype(np.uint32)


def _as_f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def planted_weights(r):
    """synth.make_weights(0) with the residual block planted: gn1 / gn2 weight zero, so every activation is max(beta_c, 0)
    whatever the statistics; beta of the live channels (c = r mod 3) cycles through ties that round down to even, ties that round
    up to even, and the float32 neighbours of both on either side; the other channels hold negative ties, negative tie
    neighbours, -0.0 and +0.0.  conv weights: ties (half of them) and tie neighbours, random signs, one binade; conv biases:
    whole multiples of the product quantum up to 1000.  No subnormal and no overflowing operand."""
    rng = np.random.default_rng(7100 + r)
    w = {k: np.array(v) for k, v in synth.make_weights(0).items()}
    for gn in ("gn1", "gn2"):
        beta = np.zeros(64, dtype=np.uint32)      # float32 bits
        live = dead = 0
        for c in range(64):
            if c % LIVE_SETS == r:
                k = live % 6
                m = 2 * int(rng.integers(0, 8)) + (1 if k in (1, 4, 5) else 0)      # even: the tie rounds down; odd: up
                beta[c] = _tie(m, E_T, {0: 0, 1: 0, 2: -1, 3: 1, 4: -1, 5: 1}[k])
                live += 1
            else:
                k = dead % 4
                m = int(rng.integers(0, 16))
                beta[c] = (_tie(m, E_T) | 0x80000000, _tie(m, E_T, 1) | 0x80000000, 0x80000000, 0)[k]
                dead += 1
        w[P + gn + ".weight"] = np.zeros(64, dtype=np.float32)
        w[P + gn + ".bias"] = _as_f32(beta)
    for conv in ("conv1", "conv2"):
        shape = (64, 64, 3, 3, 3)
        m = rng.integers(0, M_MAX + 1, shape)
        d = rng.choice(np.array([0, 0, -1, 1]), shape)
        sign = rng.integers(0, 2, shape).astype(np.uint32) << np.uint32(31)
        w[P + conv + ".weight"] = _as_f32(_tie(m, E_W, d) | sign).reshape(shape)
        w[P + conv + ".bias"] = (rng.integers(-BIAS_MAX, BIAS_MAX + 1, 64) * QUANTUM).astype(np.float32)
    return w


def round_rne(u):
    return tp.bf16_bits(u.view(np.float32))


def round_half_away(u):
    return ((u.astype(np.uint64) + 0x8000) >> 16).astype(np.uint16)


def round_half_up(u):
    """Ties towards +infinity: the magnitude goes up for a positive number, down for a negative one."""
    neg = (u >> np.uint32(31)).astype(np.uint64)
    return ((u.astype(np.uint64) + 0x8000 - neg) >> 16).astype(np.uint16)


def round_trunc(u):
    return (u >> np.uint32(16)).astype(np.uint16)


def _units(x, e, rounding):
    """float32 array -> signed integers k with bf16(x) = k 2^(e - 7) under ``rounding``."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    val = (rounding(u).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64) * 2.0 ** (7 - e)
    k = np.rint(val).astype(np.int64)
    assert np.array_equal(k.astype(np.float64), val)
    return k


TAP_VALID = np.zeros((27, 64), dtype=np.int64)      # [tap][output position]: the tap's input lies inside the leaf
for _p in range(64):
    for _t in range(27):
        _in = [(_p >> 4) + _t // 9 - 1, ((_p >> 2) & 3) + (_t // 3) % 3 - 1, (_p & 3) + _t % 3 - 1]
        TAP_VALID[_t, _p] = all(0 <= c <= 3 for c in _in)


def closed_form(w, gn, conv, rounding=round_rne):
    """-> (value [64 couts, 64 positions] float32, budget): the planted conv in whole numbers of QUANTUM.  The input is
    max(beta, 0) at every position of every leaf, so an output is sum over its valid taps of sum_ci k_W k_t, plus the bias;
    ``budget`` is the largest sum |k_W| k_t + |bias| of an output.  Below 2^24 every partial sum of every order is a float32
    number, so the float32 result does not depend on the order."""
    kt = _units(np.maximum(w[P + gn + ".bias"], np.float32(0.0)), E_T, rounding)          # [ci]
    kw = _units(w[P + conv + ".weight"], E_W, rounding).reshape(64, 64, 27)               # [co][ci][tap]
    kb = np.rint(w[P + conv + ".bias"].astype(np.float64) / QUANTUM).astype(np.int64)
    assert np.array_equal(kb * QUANTUM, w[P + conv + ".bias"].astype(np.float64))
    per_tap = np.einsum("oct,c->ot", kw, kt)
    abs_tap = np.einsum("oct,c->ot", np.abs(kw), np.abs(kt))
    total = per_tap @ TAP_VALID + kb[:, None]
    budget = int((abs_tap @ TAP_VALID + np.abs(kb)[:, None]).max())
    val = (total.astype(np.float64) * QUANTUM).astype(np.float32)
    assert budget >= 2 ** 24 or np.array_equal(val.astype(np.float64), total * QUANTUM)
    return val, budget


def planted_x6(d2, v):
    """fl(d_d2 + fl(0.1f v)) in float32, v [64, 64] broadcast over the leaves: the epilogue's two roundings, no fma."""
    uu = (np.float32(0.1) * np.asarray(v, dtype=np.float32)).astype(np.float32)
    return (np.asarray(d2, dtype=np.float32) + uu[None]).astype(np.float32)
