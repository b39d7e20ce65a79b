#!/usr/bin/env python3
"""Decode speed of the scalar codec's two precision modes on one GPU: decode_device at 65 536 and 8 192 leaves
resident in HBM, fp32 and bf16 mode alternating call by call in one process, timed on device events (3 warm-ups per mode, the
median of 10), and the per-kernel times of both modes from vqhip_profile_read.  Prints one JSON object and writes it to --out.

    python tools/precision_bench.py [--sizes 65536,8192] [--reps 10] [--warmup 3] [--out profiles/precision_bench.json]

    python tools/precision_bench.py --modes fp32 --root <another checkout, built> --out <file>

--modes fp32 never touches the precision switch, so with --root it also runs on a checkout from before the switch existed:
the "fp32 mode unchanged" comparison against the parent commit, same process layout, same session.  --parent <that file> then
adds the parent's numbers and the ratio to this run's output.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_ms(torch, st, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(st)
    fn()
    e.record(st)
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,8192")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--root", default=ROOT, help="checkout whose vqvdb_amd package (built) is measured")
    ap.add_argument("--parent", default=None, help="JSON of a --modes fp32 run on the parent commit, to compare fp32 mode against")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precision_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from vqvdb_amd import synth, weightpack
    from vqvdb_amd.codec import HipCodec

    modes = a.modes.split(",")
    c = HipCodec(weightpack.dumps(synth.make_weights(0)))

    def set_mode(m):
        if modes != ["fp32"]:
            c.decode_precision = m

    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "modes": modes, "sizes": {}}
    st = torch.cuda.Stream()   # the codec's work and the events on one stream (a null handle would mean the codec's own stream)
    rng = np.random.default_rng(23)
    for n in [int(s) for s in a.sizes.split(",")]:
        idx = torch.from_numpy(rng.integers(0, 256, (n, 64), dtype=np.uint8)).cuda()
        out = torch.empty((n, 512), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def decode():
            c.decode_device(idx.data_ptr(), n, out.data_ptr(), st.cuda_stream)

        for m in modes:
            set_mode(m)
            for _ in range(a.warmup):
                decode()
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for _ in range(a.reps):          # alternating: both modes see the same clocks and the same neighbours
            for m in modes:
                set_mode(m)
                times[m].append(event_ms(torch, st, decode))
        row = {m: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for m, t in times.items()}
        # per-kernel times: three profiled passes per mode (an event pair around every launch)
        for m in modes:
            set_mode(m)
            c.profile_enable(True)
            for _ in range(3):
                decode()
            torch.cuda.synchronize()
            row[m]["kernels_ms"] = {k["name"]: k["total_ms"] / k["launches"] for k in c.profile_read()}
            c.profile_enable(False)
        if "bf16" in row and "fp32" in row:
            row["bf16_over_fp32"] = row["bf16"]["median_ms"] / row["fp32"]["median_ms"]
            kf, kb = row["fp32"]["kernels_ms"], row["bf16"]["kernels_ms"]
            row["conv_speedup"] = {}
            for conv in ("dec_res64_conv1", "dec_res64_conv2"):
                f = kf.get(conv, kf.get(conv + "_s"))
                if f is not None and conv + "_bf16" in kb:
                    row["conv_speedup"][conv] = f / kb[conv + "_bf16"]
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
