#!/usr/bin/env python3
"""Cost and size of the scalar handle's quantised residuals on one GPU, against the existing calls in the same process.

    python tools/residual_bench.py [--leaves 65536] [--warmup 3] [--reps 15] [--file-reps 3] [--out profiles/residual_bench.json]

Device part, leaves resident in HBM, tolerance = the median leaf error, device events on one stream, the sides alternating rep by rep:
    roundtrip_device + residual_encode_device   against   roundtrip_device alone
then residual_encode_device (class, scan and pack) and residual_apply_device on their own, and the three launches of the
encode from the handle's kernel profile.
Size: payload bytes per selected leaf and the v2 sidecar against the v1 layout (2052 B per selected leaf) for the same leaves.
File part, host memory to files in a temporary directory, wall clock, alternating:
    compress_file_residual / decompress_file_residual,  compress_file_bounded / decompress_file_bounded,  compress_file / decompress_file
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
    from vqvdb_amd.codec import HipCodec, RES_KEPT, RES_RAW

    n = a.leaves
    c = HipCodec(weightpack.dumps(synth.make_weights(0)))
    base = np.concatenate([synth.make_leaves(1024, seed=4321), synth.sparse_leaves(1024)])
    host = np.ascontiguousarray(np.tile(base, ((n + 2047) // 2048, 1))[:n])
    leaves = torch.from_numpy(host).cuda()
    idx = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    rec = torch.empty((n, 512), dtype=torch.float32, device="cuda")
    err = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    pay = torch.empty(n * 2048, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    h = st.cuda_stream
    torch.cuda.synchronize()
    c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)
    torch.cuda.synchronize()
    tol = float(err[:, 0].median())

    def roundtrip():
        c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)

    def encode():
        c.residual_encode_device(leaves.data_ptr(), rec.data_ptr(), err.data_ptr(), n, tol, cls.data_ptr(), off.data_ptr(), pay.data_ptr(), n * 2048, h)

    def both():
        roundtrip()
        encode()

    def event_time(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    for _ in range(a.warmup):
        both()
        roundtrip()
    torch.cuda.synchronize()
    t_both, t_rt = [], []
    for _ in range(a.reps):
        t_both.append(event_time(both))
        t_rt.append(event_time(roundtrip))
    res = {"model": "VQVAE(1, 128, 256)", "leaves": n, "chunk_leaves": c.chunk_leaves(), "warmup": a.warmup, "reps": a.reps, "tol": tol,
           "roundtrip_plus_residual_encode": summary(t_both, n), "roundtrip": summary(t_rt, n)}
    res["with_residual_over_roundtrip"] = res["roundtrip_plus_residual_encode"]["median_s"] / res["roundtrip"]["median_s"]
    res["ratio_of_paired_reps"] = summary([x / y for x, y in zip(t_both, t_rt)], 1.0)
    del res["ratio_of_paired_reps"]["leaves_per_s"]
    res["residual_encode"] = summary([event_time(encode) for _ in range(a.reps)], n)

    # the three launches of the encode, from the handle's per-launch events
    c.profile_enable(True)
    for _ in range(a.reps):
        encode()
    torch.cuda.synchronize()
    prof = {p["name"]: p for p in c.profile_read() if p["name"].startswith("residual_")}
    c.profile_enable(False)
    res["residual_encode_launches"] = prof

    hcls, hoff = cls.cpu().numpy(), off.cpu().numpy()
    total = int(hoff[-1])
    dec = torch.empty((n, 512), dtype=torch.float32, device="cuda")

    def apply():
        c.residual_apply_device(dec.data_ptr(), n, tol, cls.data_ptr(), off.data_ptr(), pay.data_ptr(), h)

    t_ap = []
    for i in range(a.warmup + a.reps):
        dec.copy_(rec)
        torch.cuda.synchronize()
        t = event_time(apply)
        if i >= a.warmup:
            t_ap.append(t)
    res["residual_apply"] = summary(t_ap, n)
    worst_dev = float((leaves - dec).abs().max())
    assert worst_dev <= tol, (worst_dev, tol)

    sel = int((hcls != RES_KEPT).sum())
    hist = {int(k): int((hcls == k).sum()) for k in np.unique(hcls)}
    sizes = np.where(hcls == RES_KEPT, 0, np.where(hcls == RES_RAW, 2048, 64 * hcls.astype(np.int64)))
    assert sizes.sum() == total, "the offsets are not the sum of the class sizes"
    res["size"] = {"selected": sel, "raw": int((hcls == RES_RAW).sum()), "class_histogram": hist, "payload_bytes": total,
                   "payload_bytes_per_selected_leaf": total / max(sel, 1), "largest_error_after_apply": worst_dev}

    # ---- the file pairs: two grids, host leaves, default batch (one chunk per step) ----
    half = n // 2
    org = np.arange(n * 3, dtype=np.int32).reshape(n, 3)
    grids = [("density", org[:half], host[:half], None), ("temperature", org[half:], host[half:], None)]
    pool = np.empty((n, 512), dtype=np.float32)
    tmp = tempfile.mkdtemp(prefix="residual_bench_")
    try:
        plain, lossy, side1, side2 = (os.path.join(tmp, f) for f in ("plain.vqvdb", "lossy.vqvdb", "v1.vqres", "v2.vqres"))

        def wall(fn):
            t = time.perf_counter()
            r = fn()
            return time.perf_counter() - t, r

        names = ("compress_file", "compress_file_bounded", "compress_file_residual", "decompress_file", "decompress_file_bounded",
                 "decompress_file_residual")
        runs = {k: [] for k in names}
        rst = bst = None
        for rep in range(a.file_reps + 1):           # the first round warms the buffers up and is dropped
            t0, _ = wall(lambda: c.compress_file(plain, grids))
            t1, _ = wall(lambda: c.compress_file_bounded(lossy, side1, grids, tol))
            t2, (_, bst, rst) = wall(lambda: c.compress_file_residual(lossy, side2, grids, tol))
            t3, _ = wall(lambda: c.decompress_file(plain, out=pool))
            t4, _ = wall(lambda: c.decompress_file_bounded(lossy, side1, out=pool))
            t5, _ = wall(lambda: c.decompress_file_residual(lossy, side2, out=pool))
            if rep:
                for k, t in zip(names, (t0, t1, t2, t3, t4, t5)):
                    runs[k].append(t)
        worst = float(np.abs(pool - host).max())
        assert worst <= tol, (worst, tol)
        fp = {k: summary(v, n) for k, v in runs.items()}
        for k in ("compress", "decompress"):
            fp[f"{k}_residual_over_plain"] = fp[f"{k}_file_residual"]["median_s"] / fp[f"{k}_file"]["median_s"]
            fp[f"{k}_residual_over_bounded"] = fp[f"{k}_file_residual"]["median_s"] / fp[f"{k}_file_bounded"]["median_s"]
        assert rst["payload_bytes"] == total and bst["outliers"] == sel, "the file pair and the device call disagree"
        fp.update(selected=bst["outliers"], selected_share=bst["outliers"] / n, raw=rst["raw"], largest_error_after_decompress=worst,
                  vqvdb_bytes=os.path.getsize(lossy), vqres_v1_bytes=os.path.getsize(side1), vqres_v2_bytes=os.path.getsize(side2),
                  vqres_v2_predicted_bytes=11 + 4 * len(grids) + 5 * sel + total, file_reps=a.file_reps)
        fp["vqres_v2_over_v1"] = fp["vqres_v2_bytes"] / fp["vqres_v1_bytes"]
        assert fp["vqres_v2_bytes"] == fp["vqres_v2_predicted_bytes"]
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
