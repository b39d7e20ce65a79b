#!/usr/bin/env python3
"""Cost and size of the Vec3 handle's quantised residuals on one GPU, against the existing round trip in the same
process, per precision mode.

    python tools/vec3_residual_bench.py [--leaves 65536] [--warmup 3] [--reps 10] [--precision fp32|bf16|both]
                                        [--out profiles/vec3_residual_bench.json]

Leaves resident in HBM, tolerance = the median leaf error of the mode, device events on one stream, the sides alternating rep by rep:
    roundtrip_device (with a stored reconstruction) + residual_encode_device   against   that roundtrip_device alone
then residual_encode_device (class, scan and pack) and residual_apply_device on their own.  The three launches of the encode are
not timed one by one here (the Vec3 handle keeps no per-launch events): a kernel trace of this tool gives them.
Size: payload bytes per selected leaf against 6144 (raw) and against what one width shared by the three channels would have cost
(3 * max b_c * 64 per quantised leaf, from the codes), and the payload asserted equal to what the codes predict.
Prints one JSON object (and writes it with --out)."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import HipVec3Codec, VEC3_RES_KEPT, VEC3_RES_RAW

    n = a.leaves
    c = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0)))
    base = torch.from_numpy(synth_vec3.make_leaves(1024, seed=4321)).cuda()
    leaves = base.repeat((n + 1023) // 1024, 1, 1)[:n].contiguous()
    idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
    rec = torch.empty((n, 512, 3), dtype=torch.float32, device="cuda")
    dec = torch.empty((n, 512, 3), dtype=torch.float32, device="cuda")
    err = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    code = torch.empty(n, dtype=torch.int16, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    pay = torch.empty(n * 6144, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    h = st.cuda_stream
    res = {"model": "VQVAE(3, 64, 4096)", "leaves": n, "chunk_leaves": c.chunk_leaves(), "warmup": a.warmup, "reps": a.reps, "modes": {}}

    def event_time(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    for mode in {"fp32": ("fp32",), "bf16": ("bf16",), "both": ("fp32", "bf16")}[a.precision]:
        c.precision = mode
        torch.cuda.synchronize()
        c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)
        torch.cuda.synchronize()
        tol = float(err[:, 0].median())

        def roundtrip():
            c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)

        def encode():
            c.residual_encode_device(leaves.data_ptr(), rec.data_ptr(), err.data_ptr(), n, tol, code.data_ptr(), off.data_ptr(), pay.data_ptr(),
                                     n * 6144, h)

        def both():
            roundtrip()
            encode()

        def apply():
            c.residual_apply_device(dec.data_ptr(), n, tol, code.data_ptr(), off.data_ptr(), pay.data_ptr(), h)

        for _ in range(a.warmup):
            both()
            roundtrip()
        torch.cuda.synchronize()
        t_both, t_rt = [], []
        for _ in range(a.reps):
            t_both.append(event_time(both))
            t_rt.append(event_time(roundtrip))
        r = {"tol": tol, "roundtrip_plus_residual_encode": summary(t_both, n), "roundtrip": summary(t_rt, n)}
        r["with_residual_over_roundtrip"] = r["roundtrip_plus_residual_encode"]["median_s"] / r["roundtrip"]["median_s"]
        r["ratio_of_paired_reps"] = summary([x / y for x, y in zip(t_both, t_rt)], 1.0)
        del r["ratio_of_paired_reps"]["leaves_per_s"]
        for _ in range(a.warmup):
            encode()
        r["residual_encode"] = summary([event_time(encode) for _ in range(a.reps)], n)
        t_ap = []
        for i in range(a.warmup + a.reps):
            dec.copy_(rec)
            torch.cuda.synchronize()
            t = event_time(apply)
            if i >= a.warmup:
                t_ap.append(t)
        r["residual_apply"] = summary(t_ap, n)
        worst = float((leaves - dec).abs().max())
        assert worst <= tol, (worst, tol)

        hcode, hoff = code.cpu().numpy().view(np.uint16), off.cpu().numpy()
        total = int(hoff[-1])
        sizes = HipVec3Codec.residual_record_sizes(hcode)
        assert sizes.sum() == total and np.array_equal(np.cumsum(sizes), hoff[1:]), "the offsets are not the sums of the code sizes"
        sel = hcode != VEC3_RES_KEPT
        raw = hcode == VEC3_RES_RAW
        q = hcode[sel & ~raw].astype(np.int64)
        b = np.stack([q & 31, (q >> 5) & 31, (q >> 10) & 31], axis=1)
        shared = int(3 * 64 * b.max(axis=1).sum()) + 6144 * int(raw.sum()) if len(b) else 6144 * int(raw.sum())
        nsel = int(sel.sum())
        r["size"] = {"selected": nsel, "raw": int(raw.sum()), "payload_bytes": total, "payload_bytes_predicted_from_codes": int(sizes.sum()),
                     "payload_bytes_per_selected_leaf": total / max(nsel, 1), "raw_bytes_per_selected_leaf": 6144,
                     "payload_over_raw": total / max(nsel * 6144, 1), "shared_width_bytes": shared,
                     "shared_width_bytes_per_selected_leaf": shared / max(nsel, 1), "payload_over_shared_width": total / max(shared, 1),
                     "mean_planes_per_channel": b.mean(axis=0).tolist() if len(b) else None, "largest_error_after_apply": worst}
        res["modes"][mode] = r
    c.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
