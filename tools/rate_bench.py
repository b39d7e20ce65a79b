#!/usr/bin/env python3
"""Cost of the scalar handle's size sweep on one GPU, against the existing calls in the same process.

    python tools/rate_bench.py [--leaves 65536] [--warmup 3] [--reps 15] [--file-reps 3] [--out profiles/rate_bench.json]

Device part, leaves resident in HBM, tolerance ladders geometric around the median leaf error (a factor of 16 either way, so that
most rungs select a good share of the leaves), device events on one stream, the sides alternating rep by rep:
    roundtrip_device + rate_sweep_device at 1, 16 and 64 rungs   against   roundtrip_device alone
then rate_sweep_device alone at each rung count, on this ladder and on one whose every rung selects every leaf (the most arithmetic).
File part, host memory to files in a temporary directory, wall clock, alternating:
    rate_sweep_file (16 rungs),  rate_compress_file (16 rungs, budget = the median rung's size),  compress_file_residual (median)
Prints one JSON object (and writes it with --out)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--file-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from vqvdb_amd import synth, weightpack
    from vqvdb_amd.codec import RATE_CLASSES, HipCodec, rate_payload_bytes, rate_sidecar_bytes

    n = a.leaves
    c = HipCodec(weightpack.dumps(synth.make_weights(0)))
    base = np.concatenate([synth.make_leaves(1024, seed=4321), synth.sparse_leaves(1024)])
    host = np.ascontiguousarray(np.tile(base, ((n + 2047) // 2048, 1))[:n])
    leaves = torch.from_numpy(host).cuda()
    idx = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    rec = torch.empty((n, 512), dtype=torch.float32, device="cuda")
    err = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    hist = torch.zeros((64, RATE_CLASSES), dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    h = st.cuda_stream
    torch.cuda.synchronize()
    c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)
    torch.cuda.synchronize()
    med = float(err[:, 0].median())

    def roundtrip():
        c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)

    def sweep(tols):
        return lambda: c.rate_sweep_device(leaves.data_ptr(), rec.data_ptr(), err.data_ptr(), n, tols, hist.data_ptr(), h)

    def event_time(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    res = {"model": "VQVAE(1, 128, 256)", "leaves": n, "chunk_leaves": c.chunk_leaves(), "warmup": a.warmup, "reps": a.reps, "median_leaf_error": med,
           "bar": BAR, "behind_a_roundtrip": {}, "sweep_alone": {}, "sweep_alone_every_leaf_selected": {}}
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
        r = {"roundtrip_plus_sweep": summary(t_both, n), "roundtrip": summary(t_rt, n)}
        r["with_sweep_over_roundtrip"] = r["roundtrip_plus_sweep"]["median_s"] / r["roundtrip"]["median_s"]
        r["ratio_of_paired_reps"] = summary([x / y for x, y in zip(t_both, t_rt)], 1.0)
        del r["ratio_of_paired_reps"]["leaves_per_s"]
        r["meets_bar"] = r["with_sweep_over_roundtrip"] <= BAR
        res["behind_a_roundtrip"][str(rungs)] = r
        hist.zero_()
        torch.cuda.synchronize()
        one()
        torch.cuda.synchronize()
        hh = hist[:rungs].cpu().numpy()
        assert (hh.sum(axis=1) == n).all(), "a histogram row does not sum to the leaves"
        alone = summary([event_time(one) for _ in range(a.reps)], n)
        alone["selected_share_per_rung"] = [float(x) for x in 1.0 - hh[:, 18] / n]
        res["sweep_alone"][str(rungs)] = alone
        tight = [float(v) for v in np.geomspace(med / 4096, med / 64, rungs).astype(np.float32)] if rungs > 1 else [med / 4096]
        worst = sweep(tight)
        worst()
        torch.cuda.synchronize()
        res["sweep_alone_every_leaf_selected"][str(rungs)] = summary([event_time(worst) for _ in range(a.reps)], n)
    res["largest_rung_count_within_bar"] = max([r for r in RUNGS if res["behind_a_roundtrip"][str(r)]["meets_bar"]], default=0)

    # ---- the file calls: two grids, host leaves, default batch (one chunk per step) ----
    half = n // 2
    org = np.arange(n * 3, dtype=np.int32).reshape(n, 3)
    grids = [("density", org[:half], host[:half], None), ("temperature", org[half:], host[half:], None)]
    tols = ladder(med, 16)
    tmp = tempfile.mkdtemp(prefix="rate_bench_")
    try:
        lossy, side, lossy2, side2 = (os.path.join(tmp, f) for f in ("a.vqvdb", "a.vqres", "b.vqvdb", "b.vqres"))

        def wall(fn):
            t = time.perf_counter()
            r = fn()
            return time.perf_counter() - t, r

        fh, _ = c.rate_sweep_file(grids, tols)
        sizes = [rate_sidecar_bytes(r, 2) for r in fh]
        budget = sizes[8]
        names = ("rate_sweep_file", "rate_compress_file", "compress_file_residual")
        runs = {k: [] for k in names}
        used = rst = None
        for rep in range(a.file_reps + 1):           # the first round warms the buffers up and is dropped
            t0, _ = wall(lambda: c.rate_sweep_file(grids, tols))
            t1, (used, _, _, _, rst) = wall(lambda: c.rate_compress_file(lossy, side, grids, tols, budget))
            t2, _ = wall(lambda: c.compress_file_residual(lossy2, side2, grids, used))
            if rep:
                for k, t in zip(names, (t0, t1, t2)):
                    runs[k].append(t)
        fp = {k: summary(v, n) for k, v in runs.items()}
        fp["sweep_file_over_compress_file_residual"] = fp["rate_sweep_file"]["median_s"] / fp["compress_file_residual"]["median_s"]
        fp["rate_compress_file_over_compress_file_residual"] = fp["rate_compress_file"]["median_s"] / fp["compress_file_residual"]["median_s"]
        t = tols.index(used) if used in tols else int(np.argmin([abs(v - used) for v in tols]))
        assert os.path.getsize(side) == sizes[t] == os.path.getsize(side2) <= budget, "the prediction and the files disagree"
        assert rst["payload_bytes"] == rate_payload_bytes(fh[t])
        fp.update(rungs=16, budget_bytes=budget, tol_used=used, sidecar_bytes=os.path.getsize(side), predicted_sidecar_bytes=sizes[t],
                  predicted_sidecar_bytes_per_rung=sizes, file_reps=a.file_reps)
        res["file_calls"] = fp
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    c.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
