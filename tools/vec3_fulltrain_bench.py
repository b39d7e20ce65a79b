#!/usr/bin/env python3
"""Time of one full Vec3 training step (VQVAE(3, 64, 4096), fp32) on one GPU: fwdbwd_device + apply_device, against the
same batch's encode_device + decode_device in the same process.  Inputs are resident on the device; device events around
each call, after a warm-up, median of the repeats.  Prints one JSON object and writes it with --out.

FLOPs counted are the ones the result needs (2 per multiply-add, zero-padding taps not counted): the forward (the
581 MFLOP/leaf of DESIGN.md §11, codebook search included), the data gradients of every conv but encoder.pre.0 and the
weight gradients of every conv (as many as the conv's forward each).  The fraction of peak is against 155 TFLOP/s, the measured
fp32-MFMA rate of the MI355X.

    python tools/vec3_fulltrain_bench.py [--sizes 1024,4096] [--reps 10] [--out profiles/vec3_fulltrain_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 155.0
VQ_SEARCH = 2 * 64 * 64 * 4096   # the forward's nearest-code search (its distances), per leaf
# (name, cin, cout, input size, output size, k, stride, pad)
CONVS = [("encoder.pre.0", 3, 64, 8, 8, 3, 1, 1)] + [("encoder.pre.3", 64, 64, 8, 8, 3, 1, 1)] * 2 + \
        [("encoder.down1", 64, 128, 8, 4, 3, 2, 1)] + [("encoder.res_stack", 128, 128, 4, 4, 3, 1, 1)] * 4 + \
        [("encoder.proj", 128, 64, 4, 4, 1, 1, 0), ("decoder.stem.0", 64, 128, 4, 4, 3, 1, 1)] + \
        [("decoder.res_stack", 128, 128, 4, 4, 3, 1, 1)] * 4 + [("decoder.up_conv", 128, 256, 4, 4, 3, 1, 1),
                                                                ("decoder.final", 32, 3, 8, 8, 3, 1, 1)]


def valid_taps(si, so, k, stride, pad):
    """Multiply-adds per (input channel, output channel) pair of one leaf: taps inside the input, summed over outputs."""
    per_axis = sum(sum(1 for t in range(k) if 0 <= o * stride - pad + t < si) for o in range(so))
    return per_axis ** 3


def flops_per_leaf():
    fwd = sum(2 * ci * co * valid_taps(si, so, k, s, p) for _, ci, co, si, so, k, s, p in CONVS) + VQ_SEARCH
    convs = fwd - VQ_SEARCH
    dgrad = convs - 2 * 3 * 64 * valid_taps(8, 8, 3, 1, 1)    # no data gradient of encoder.pre.0
    wgrad = convs
    return fwd, dgrad, wgrad


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import HipVec3Codec

    W = synth_vec3.make_weights(0)
    fwd, dgrad, wgrad = flops_per_leaf()
    total = fwd + dgrad + wgrad
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "peak_tflops": PEAK_TFLOPS,
           "mflop_per_leaf": {"forward": fwd / 1e6, "data_gradients": dgrad / 1e6, "weight_gradients": wgrad / 1e6, "step": total / 1e6},
           "sizes": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        c = HipVec3Codec(weightpack.dumps(W))
        c.fulltrain_begin()
        x = torch.from_numpy(synth_vec3.make_leaves(n, seed=11)).cuda()
        idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
        rec = torch.empty((n, 512, 3), dtype=torch.float32, device="cuda")
        g = torch.zeros(c.fulltrain_param_count(), device="cuda")
        aux = torch.zeros(c.fulltrain_aux_floats(), device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            inf = timed(lambda: (c.encode_device(x.data_ptr(), n, idx.data_ptr(), stream=h),
                                 c.decode_device(idx.data_ptr(), n, rec.data_ptr(), stream=h)), a.reps, a.warmup)
            fb = timed(lambda: c.fulltrain_fwdbwd_device(x.data_ptr(), n, n, g.data_ptr(), aux.data_ptr(), stream=h), a.reps, a.warmup)
            # lr 0, weight decay 0 and no aux: AdamW moves nothing and the codebook stays, so every repeat does the same work
            ap_ms = timed(lambda: c.fulltrain_apply_device(g.data_ptr(), 0, 0.0, 1, weight_decay=0.0, stream=h), a.reps, a.warmup)
        c.close()
        step = fb + ap_ms
        out["sizes"].append({"leaves": n, "encode_decode_ms": round(inf, 3), "fwdbwd_ms": round(fb, 3), "apply_ms": round(ap_ms, 3),
                             "step_ms": round(step, 3), "step_over_encode_decode": round(step / inf, 2),
                             "leaves_per_s": round(n / (step / 1e3)), "tflops": round(total * n / (step / 1e3) / 1e12, 2),
                             "frac_of_peak": round(total * n / (step / 1e3) / 1e12 / PEAK_TFLOPS, 3)})
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
