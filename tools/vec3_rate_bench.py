#!/usr/bin/env python3
"""Cost of the Vec3 handle's size sweep and budget compress on one GPU, against the existing calls in the same
process, per precision mode.

    python tools/vec3_rate_bench.py [--leaves 65536] [--warmup 3] [--reps 10] [--host-reps 3] [--precision fp32|bf16|both]
                                    [--out profiles/vec3_rate_bench.json]

Device part, leaves resident in HBM, tolerance ladders geometric around the mode's median leaf error (a factor of 16 either way, so
that most rungs select a good share of the leaves), device events on one stream, the sides alternating rep by rep:
    roundtrip_device (with a stored reconstruction) + rate_sweep_device at 1, 16 and 64 rungs   against   that roundtrip_device alone
then rate_sweep_device alone at each rung count, on this ladder and on one whose every rung selects every leaf (the most arithmetic).
Host part, host memory in and out, wall clock, alternating (16 rungs, budget = the payload of the ladder's middle rung):
    rate_compress   against   rate_sweep followed by compress_residual at the same tolerance   and   compress_residual alone
with the payload asserted equal, to the byte, to what the histogram row predicted and to compress_residual's.
Prints one JSON object (and writes it with --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNGS = (1, 16, 64)
BAR = 1.03   # DESIGN §17's bar for a pass that rides behind a round trip, applied to 16 rungs


def summary(times, n):
    t = float(np.median(times))
    return {"median_s": t, "min_s": float(min(times)), "max_s": float(max(times)), "leaves_per_s": n / t}


def ladder(med, rungs):
    return [med] if rungs == 1 else [float(v) for v in np.geomspace(med / 16, med * 16, rungs).astype(np.float32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import VEC3_RATE_CLASSES, HipVec3Codec, vec3_rate_payload_bytes

    n = a.leaves
    c = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0)))
    base = synth_vec3.make_leaves(1024, seed=4321)
    host = np.ascontiguousarray(np.tile(base, ((n + 1023) // 1024, 1, 1))[:n])
    leaves = torch.from_numpy(host).cuda()
    idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
    rec = torch.empty((n, 512, 3), dtype=torch.float32, device="cuda")
    err = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    hist = torch.zeros((64, VEC3_RATE_CLASSES), dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    h = st.cuda_stream
    res = {"model": "VQVAE(3, 64, 4096)", "leaves": n, "chunk_leaves": c.chunk_leaves(), "warmup": a.warmup, "reps": a.reps,
           "host_reps": a.host_reps, "bar": BAR, "modes": {}}

    def event_time(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    def wall(fn):
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    def roundtrip():
        c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)

    def sweep(tols):
        return lambda: c.rate_sweep_device(leaves.data_ptr(), rec.data_ptr(), err.data_ptr(), n, tols, hist.data_ptr(), h)

    for mode in {"fp32": ("fp32",), "bf16": ("bf16",), "both": ("fp32", "bf16")}[a.precision]:
        c.precision = mode
        torch.cuda.synchronize()
        roundtrip()
        torch.cuda.synchronize()
        med = float(err[:, 0].median())
        r = {"median_leaf_error": med, "behind_a_roundtrip": {}, "sweep_alone": {}, "sweep_alone_every_leaf_selected": {}}
        for rungs in RUNGS:
            tols = ladder(med, rungs)
            one = sweep(tols)

            def both():
                roundtrip()
                one()

            for _ in range(a.warmup):
                both()
                roundtrip()
            torch.cuda.synchronize()
            t_both, t_rt = [], []
            for _ in range(a.reps):
                t_both.append(event_time(both))
                t_rt.append(event_time(roundtrip))
            b = {"roundtrip_plus_sweep": summary(t_both, n), "roundtrip": summary(t_rt, n)}
            b["with_sweep_over_roundtrip"] = b["roundtrip_plus_sweep"]["median_s"] / b["roundtrip"]["median_s"]
            b["ratio_of_paired_reps"] = summary([x / y for x, y in zip(t_both, t_rt)], 1.0)
            del b["ratio_of_paired_reps"]["leaves_per_s"]
            b["meets_bar"] = b["with_sweep_over_roundtrip"] <= BAR
            r["behind_a_roundtrip"][str(rungs)] = b
            hist.zero_()
            torch.cuda.synchronize()
            one()
            torch.cuda.synchronize()
            hh = hist[:rungs].cpu().numpy()
            assert (hh.sum(axis=1) == n).all(), "a histogram row does not sum to the leaves"
            alone = summary([event_time(one) for _ in range(a.reps)], n)
            alone["selected_share_per_rung"] = [float(x) for x in 1.0 - hh[:, VEC3_RATE_CLASSES - 1] / n]
            r["sweep_alone"][str(rungs)] = alone
            tight = [float(v) for v in np.geomspace(med / 4096, med / 64, rungs).astype(np.float32)] if rungs > 1 else [med / 4096]
            worst = sweep(tight)
            worst()
            torch.cuda.synchronize()
            r["sweep_alone_every_leaf_selected"][str(rungs)] = summary([event_time(worst) for _ in range(a.reps)], n)
        r["largest_rung_count_within_bar"] = max([k for k in RUNGS if r["behind_a_roundtrip"][str(k)]["meets_bar"]], default=0)

        # ---- the host calls: host leaves in, host arrays out, the handle's default chunk ----
        tols = ladder(med, 16)
        sizes = [vec3_rate_payload_bytes(row) for row in c.rate_sweep(host, tols)]
        budget = sizes[8]
        names = ("rate_compress", "rate_sweep_then_compress_residual", "compress_residual")
        runs = {k: [] for k in names}
        for rep in range(a.host_reps + 1):               # the first round warms the buffers up and is dropped
            t0, (used, hh, i0, c0, p0) = wall(lambda: c.rate_compress(host, tols, budget))

            def two_calls():
                h2 = c.rate_sweep(host, tols)
                fits = [t for t, row in enumerate(h2) if vec3_rate_payload_bytes(row) <= budget]
                return c.compress_residual(host, min(tols[t] for t in fits))

            t1, (i1, c1, p1) = wall(two_calls)
            t2, (i2, c2, p2) = wall(lambda: c.compress_residual(host, used))
            t = int(np.argmin([abs(v - used) for v in tols]))
            assert len(p0) == vec3_rate_payload_bytes(hh[t]) == sizes[t] <= budget, "the histogram's prediction and the payload disagree"
            assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in ((i0, i1, i2), (c0, c1, c2), (p0, p1, p2))), \
                "rate_compress and compress_residual disagree"
            if rep:
                for k, v in zip(names, (t0, t1, t2)):
                    runs[k].append(v)
        hp = {k: summary(v, n) for k, v in runs.items()}
        two = hp["rate_sweep_then_compress_residual"]
        hp["rate_compress_over_two_calls"] = hp["rate_compress"]["median_s"] / two["median_s"]
        hp["rate_compress_over_compress_residual"] = hp["rate_compress"]["median_s"] / hp["compress_residual"]["median_s"]
        hp["two_calls_spread_s"] = two["max_s"] - two["min_s"]
        hp["saved_against_two_calls_s"] = two["median_s"] - hp["rate_compress"]["median_s"]
        hp["faster_than_two_calls_by_more_than_their_spread"] = hp["saved_against_two_calls_s"] > hp["two_calls_spread_s"]
        hp.update(rungs=16, budget_bytes=budget, tol_used=used, payload_bytes=len(p0), predicted_payload_bytes=sizes[t],
                  predicted_payload_bytes_per_rung=sizes)
        r["host_calls"] = hp
        res["modes"][mode] = r
    c.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
