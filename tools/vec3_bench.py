#!/usr/bin/env python3
"""Throughput of the Vec3 model (VQVAE(3, 64, 4096)) on one GPU: encode and decode with inputs resident on the device,
timed with device events after a warm-up, at 16 384 and 65 536 leaves.  Prints one JSON object (and writes it with --out).

FLOPs per leaf are counted here from the layer shapes, taps inside the leaf only (zero padding skipped, as the kernels do),
2 FLOPs per multiply-add; the fraction of peak is against 155 TFLOP/s, the measured fp32-MFMA rate of the MI355X.

    python tools/vec3_bench.py [--sizes 16384,65536] [--reps 5] [--precision fp32|bf16|both] [--out profiles/vec3_bench.json]

--precision bf16 / both adds the bf16-operand inference mode on the same handle, under "bf16" per size; its
fraction of peak is still against the fp32-MFMA rate, so that the two modes' columns compare directly.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 155.0


def conv_macs(cin, cout, si, k, stride, pad):
    """Multiply-adds of one conv over one leaf, counting only taps that land inside the input."""
    so = (si + 2 * pad - k) // stride + 1
    valid = 0
    for o in range(so):
        valid += sum(1 for t in range(k) if 0 <= o * stride - pad + t < si)
    return cin * cout * valid ** 3


def flops_per_leaf(k_codes=4096):
    enc = (conv_macs(3, 64, 8, 3, 1, 1) + 2 * conv_macs(64, 64, 8, 3, 1, 1) + conv_macs(64, 128, 8, 3, 2, 1)
           + 4 * conv_macs(128, 128, 4, 3, 1, 1) + conv_macs(128, 64, 4, 1, 1, 0) + 64 * k_codes * 64)
    dec = (conv_macs(64, 128, 4, 3, 1, 1) + 4 * conv_macs(128, 128, 4, 3, 1, 1) + conv_macs(128, 256, 4, 3, 1, 1)
           + conv_macs(32, 3, 8, 3, 1, 1))
    return 2.0 * enc, 2.0 * dec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import HipVec3Codec

    fe, fd = flops_per_leaf()
    c = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0)))
    res = {"model": "VQVAE(3, 64, 4096)", "chunk_leaves": c.chunk_leaves(), "encode_mflop_per_leaf": fe / 1e6,
           "decode_mflop_per_leaf": fd / 1e6, "peak_tflops": PEAK_TFLOPS, "sizes": {}}
    base = torch.from_numpy(synth_vec3.make_leaves(1024, seed=4321)).cuda()
    st = torch.cuda.Stream()   # the codec's work and the events on one stream (a null handle would mean the codec's own stream)
    for n in [int(s) for s in a.sizes.split(",")]:
        leaves = base.repeat((n + 1023) // 1024, 1, 1)[:n].contiguous()
        idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
        out = torch.empty((n, 512, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        row = {}
        modes = {"fp32": ("fp32",), "bf16": ("bf16",), "both": ("fp32", "bf16")}[a.precision]
        for mode, name, fn, flop in [(m, *t) for m in modes for t in (
                ("encode", lambda: c.encode_device(leaves.data_ptr(), n, idx.data_ptr(), st.cuda_stream), fe),
                ("decode", lambda: c.decode_device(idx.data_ptr(), n, out.data_ptr(), st.cuda_stream), fd))]:
            c.precision = mode
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(st)
                fn()
                e.record(st)
                torch.cuda.synchronize()
                times.append(s.elapsed_time(e) / 1e3)
            t = float(np.median(times))
            dst = row if mode == "fp32" else row.setdefault("bf16", {})
            dst[name] = {"median_s": t, "min_s": float(min(times)), "leaves_per_s": n / t,
                         "tflops": flop * n / t / 1e12, "frac_of_peak": flop * n / t / 1e12 / PEAK_TFLOPS}
        res["sizes"][str(n)] = row
    c.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
