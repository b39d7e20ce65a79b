#!/usr/bin/env python3
"""Cost of the scalar handle's error-bounded calls on one GPU, against the existing calls in the same process.

    python tools/bounded_bench.py [--leaves 65536] [--warmup 3] [--reps 15] [--file-reps 3] [--out profiles/bounded_bench.json]

Device part, leaves resident in HBM, device events on one stream, the two sides alternating rep by rep:
    roundtrip_device without a stored reconstruction   against   encode_device + decode_device on the same leaves
and select_outliers_device at the median error (half of the leaves selected).
File part, host memory to files in a temporary directory, wall clock, alternating:
    compress_file_bounded / decompress_file_bounded    against   compress_file / decompress_file
at the median error, with the outlier share beside the rates.  Prints one JSON object (and writes it with --out)."""
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


def summary(times, n):
    t = float(np.median(times))
    return {"median_s": t, "min_s": float(min(times)), "max_s": float(max(times)), "leaves_per_s": n / t}


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
    from vqvdb_amd.codec import HipCodec

    n = a.leaves
    c = HipCodec(weightpack.dumps(synth.make_weights(0)))
    base = np.concatenate([synth.make_leaves(1024, seed=4321), synth.sparse_leaves(1024)])
    host = np.ascontiguousarray(np.tile(base, ((n + 2047) // 2048, 1))[:n])
    leaves = torch.from_numpy(host).cuda()
    idx = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 512), dtype=torch.float32, device="cuda")
    err = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int64, device="cuda")
    cnt = torch.empty(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    h = st.cuda_stream
    torch.cuda.synchronize()

    def roundtrip():
        c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), 0, h)

    def encode_decode():
        c.encode_device(leaves.data_ptr(), n, idx.data_ptr(), h)
        c.decode_device(idx.data_ptr(), n, out.data_ptr(), h)

    def event_time(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    for _ in range(a.warmup):
        roundtrip()
        encode_decode()
    torch.cuda.synchronize()
    t_rt, t_ed = [], []
    for _ in range(a.reps):
        t_rt.append(event_time(roundtrip))
        t_ed.append(event_time(encode_decode))
    res = {"model": "VQVAE(1, 128, 256)", "leaves": n, "chunk_leaves": c.chunk_leaves(), "warmup": a.warmup, "reps": a.reps,
           "roundtrip": summary(t_rt, n), "encode_plus_decode": summary(t_ed, n)}
    res["roundtrip_over_encode_plus_decode"] = res["roundtrip"]["median_s"] / res["encode_plus_decode"]["median_s"]
    res["ratio_of_paired_reps"] = summary([x / y for x, y in zip(t_rt, t_ed)], 1.0)
    del res["ratio_of_paired_reps"]["leaves_per_s"]

    tol = float(err[:, 0].median())
    sel = lambda: c.select_outliers_device(err.data_ptr(), n, tol, ids.data_ptr(), cnt.data_ptr(), h)   # noqa: E731
    for _ in range(a.warmup):
        sel()
    res["select_outliers"] = summary([event_time(sel) for _ in range(a.reps)], n)
    res["select_outliers"].update(tol=tol, outliers=int(cnt.item()))

    # ---- the file pair: two grids, host leaves, default batch (one chunk per step) ----
    half = n // 2
    org = np.arange(n * 3, dtype=np.int32).reshape(n, 3)
    grids = [("density", org[:half], host[:half], None), ("temperature", org[half:], host[half:], None)]
    pool = np.empty((n, 512), dtype=np.float32)
    tmp = tempfile.mkdtemp(prefix="bounded_bench_")
    try:
        plain, lossy, side = (os.path.join(tmp, f) for f in ("plain.vqvdb", "bounded.vqvdb", "bounded.vqres"))

        def wall(fn):
            t = time.perf_counter()
            r = fn()
            return time.perf_counter() - t, r

        runs = {"compress_file": [], "compress_file_bounded": [], "decompress_file": [], "decompress_file_bounded": []}
        bst = None
        for rep in range(a.file_reps + 1):           # the first round warms the buffers up and is dropped
            t0, _ = wall(lambda: c.compress_file(plain, grids))
            t1, (_, bst) = wall(lambda: c.compress_file_bounded(lossy, side, grids, tol))
            t2, _ = wall(lambda: c.decompress_file(plain, out=pool))
            if rep == 0:
                assert np.array_equal(pool.view(np.uint32), c.decode(c.encode(host)).view(np.uint32)), "decompress_file differs from decode"
            t3, _ = wall(lambda: c.decompress_file_bounded(lossy, side, out=pool))
            if rep:
                for k, t in zip(runs, (t0, t1, t2, t3)):
                    runs[k].append(t)
        worst = float(np.abs(pool - host).max())
        fp = {k: summary(v, n) for k, v in runs.items()}
        fp["compress_bounded_over_plain"] = fp["compress_file_bounded"]["median_s"] / fp["compress_file"]["median_s"]
        fp["decompress_bounded_over_plain"] = fp["decompress_file_bounded"]["median_s"] / fp["decompress_file"]["median_s"]
        fp.update(tol=tol, outliers=bst["outliers"], outlier_share=bst["outliers"] / n, max_err_kept=bst["max_err_kept"],
                  largest_error_after_decompress=worst, vqvdb_bytes=os.path.getsize(lossy), vqres_bytes=os.path.getsize(side),
                  file_reps=a.file_reps)
        assert worst <= tol, (worst, tol)
        res["file_pair"] = fp
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
