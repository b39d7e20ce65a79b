#!/usr/bin/env python3
"""Encode speed of the scalar codec's two encode modes on one GPU: encode_device at 8 192 and 65 536 leaves
resident in HBM, fp32 and bf16 mode alternating call by call in one process, timed on device events (3 warm-ups per mode, the
median of 10), the per-kernel times of both modes from vqhip_profile_read, and the effective bytes per second of the two bf16
launches against the bytes they must move (conv1 reads and writes 32 KiB per leaf, conv2 reads 64 KiB and writes 32 KiB).
Prints one JSON object and writes it to --out.

    python tools/encode_mode_bench.py [--sizes 8192,65536] [--reps 10] [--warmup 3] [--out profiles/encode_mode_bench.json]

    python tools/encode_mode_bench.py --modes fp32 --root <another checkout, built> --out <file>

--modes fp32 never touches the switch, so with --root it also runs on a checkout from before the switch existed: the "fp32 mode
unchanged" comparison against the parent commit.  --parent <that file> then adds the parent's numbers and the ratio.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_PER_LEAF = {"enc_res16_conv1_bf16": 2 * 32768, "enc_res16_conv2_bf16": 3 * 32768}


def event_ms(torch, st, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(st)
    fn()
    e.record(st)
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--root", default=ROOT, help="checkout whose vqvdb_amd package (built) is measured")
    ap.add_argument("--parent", default=None, help="JSON of a --modes fp32 run on the parent commit, to compare fp32 mode against")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_mode_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from vqvdb_amd import synth, weightpack
    from vqvdb_amd.codec import HipCodec

    modes = a.modes.split(",")
    c = HipCodec(weightpack.dumps(synth.make_weights(0)))

    def set_mode(m):
        if modes != ["fp32"]:
            c.encode_precision = m

    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "modes": modes, "sizes": {}}
    st = torch.cuda.Stream()   # the codec's work and the events on one stream (a null handle would mean the codec's own stream)
    for n in [int(s) for s in a.sizes.split(",")]:
        x = torch.from_numpy(synth.make_leaves(n, seed=4242)).cuda()
        out = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def encode():
            c.encode_device(x.data_ptr(), n, out.data_ptr(), st.cuda_stream)

        for m in modes:
            set_mode(m)
            for _ in range(a.warmup):
                encode()
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for _ in range(a.reps):          # alternating: both modes see the same clocks and the same neighbours
            for m in modes:
                set_mode(m)
                times[m].append(event_ms(torch, st, encode))
        row = {m: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for m, t in times.items()}
        # per-kernel times: three profiled passes per mode (an event pair around every launch)
        for m in modes:
            set_mode(m)
            c.profile_enable(True)
            for _ in range(3):
                encode()
            torch.cuda.synchronize()
            row[m]["kernels_ms"] = {k["name"]: k["total_ms"] / k["launches"] for k in c.profile_read()}
            c.profile_enable(False)
        if "bf16" in row and "fp32" in row:
            row["bf16_over_fp32"] = row["bf16"]["median_ms"] / row["fp32"]["median_ms"]
            kf, kb = row["fp32"]["kernels_ms"], row["bf16"]["kernels_ms"]
            row["conv_speedup"], row["bf16_effective_TBps"] = {}, {}
            for conv in ("enc_res16_conv1", "enc_res16_conv2"):
                f = kf.get(conv, kf.get(conv + "_s"))
                if f is not None and conv + "_bf16" in kb:
                    row["conv_speedup"][conv] = f / kb[conv + "_bf16"]
                if conv + "_bf16" in kb:
                    row["bf16_effective_TBps"][conv + "_bf16"] = BYTES_PER_LEAF[conv + "_bf16"] * n / (kb[conv + "_bf16"] * 1e-3) / 1e12
        res["sizes"][str(n)] = row
    c.close()
    if a.parent:
        with open(a.parent) as f:
            par = json.load(f)
        res["parent_fp32"] = {n: par["sizes"][n]["fp32"]["median_ms"] for n in res["sizes"] if n in par["sizes"]}
        res["fp32_over_parent"] = {n: res["sizes"][n]["fp32"]["median_ms"] / v for n, v in res["parent_fp32"].items()}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
