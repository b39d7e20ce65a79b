#!/usr/bin/env python3
"""Throughput of the Vec3 model (VQVAE(3, 64, 4096)) on one GPU: encode and decode with inputs resident on the device,
timed with device events after a warm-up, at 16 384 and 65 536 leaves.  Prints one JSON object (and writes it with --out).

FLOPs per leaf are counted here from the layer shapes, taps inside the leaf only (zero padding skipped, as the kernels do),
2 FLOPs per multiply-add; the fraction of peak is against 155 TFLOP/s, the measured fp32-MFMA rate of the MI355X.

    python tools/vec3_bench.py [--sizes 16384,65536] [--reps 5] [--precision fp32|bf16|both] [--out profiles/vec3_bench.json]

--precision bf16 / both adds the bf16-operand inference mode on the same handle, under "bf16" per size; its
fraction of peak is still against the fp32-MFMA rate, so that the two modes' columns compare directly.

    python tools/vec3_bench.py --roundtrip [--precision both] [--out profiles/vec3_bounded_bench.json]

--roundtrip times the error-bounded round trip instead: encode_device, decode_device, roundtrip_device without
and with a stored reconstruction, and select_outliers_device, per precision mode; 3 warm-ups and the median of 10 unless
--warmup / --reps say otherwise.
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


def timed(torch, st, fn, warmup, reps):
    """Median and minimum seconds of fn() between two device events on stream st."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / 1e3)
    return float(np.median(times)), float(min(times))


def roundtrip_bench(a):
    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import HipVec3Codec

    warmup, reps = (3 if a.warmup is None else a.warmup), (10 if a.reps is None else a.reps)
    c = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0)))
    res = {"model": "VQVAE(3, 64, 4096)", "chunk_leaves": c.chunk_leaves(), "warmup": warmup, "reps": reps, "sizes": {}}
    base = torch.from_numpy(synth_vec3.make_leaves(1024, seed=4321)).cuda()
    st = torch.cuda.Stream()
    h = st.cuda_stream
    for n in [int(s) for s in a.sizes.split(",")]:
        leaves = base.repeat((n + 1023) // 1024, 1, 1)[:n].contiguous()
        idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
        out = torch.empty((n, 512, 3), dtype=torch.float32, device="cuda")
        err = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        ids = torch.empty(n, dtype=torch.int64, device="cuda")
        cnt = torch.empty(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        row = {}
        for mode in {"fp32": ("fp32",), "bf16": ("bf16",), "both": ("fp32", "bf16")}[a.precision]:
            c.precision = mode
            r = {}
            for name, fn in (
                    ("encode", lambda: c.encode_device(leaves.data_ptr(), n, idx.data_ptr(), h)),
                    ("decode", lambda: c.decode_device(idx.data_ptr(), n, out.data_ptr(), h)),
                    ("roundtrip", lambda: c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), 0, h)),
                    ("roundtrip_recon", lambda: c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), out.data_ptr(), h))):
                t, tmin = timed(torch, st, fn, warmup, reps)
                r[name] = {"median_s": t, "min_s": tmin, "leaves_per_s": n / t}
            tol = float(err[:, 0].median())      # half of the leaves are outliers
            t, tmin = timed(torch, st, lambda: c.select_outliers_device(err.data_ptr(), n, tol, ids.data_ptr(), cnt.data_ptr(), h), warmup, reps)
            r["select_outliers"] = {"median_s": t, "min_s": tmin, "outliers": int(cnt.item()), "tol": tol}
            both = r["encode"]["median_s"] + r["decode"]["median_s"]
            r["encode_plus_decode_s"] = both
            r["roundtrip_over_encode_plus_decode"] = r["roundtrip"]["median_s"] / both
            r["roundtrip_recon_over_encode_plus_decode"] = r["roundtrip_recon"]["median_s"] / both
            row[mode] = r
        res["sizes"][str(n)] = row
    c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--reps", type=int, default=None, help="default 5 (10 with --roundtrip)")
    ap.add_argument("--warmup", type=int, default=None, help="default 2 (3 with --roundtrip)")
    ap.add_argument("--roundtrip", action="store_true", help="time the error-bounded round trip and the selection (DESIGN §15)")
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.roundtrip:
        res = roundtrip_bench(a)
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    a.reps, a.warmup = (5 if a.reps is None else a.reps), (2 if a.warmup is None else a.warmup)
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
