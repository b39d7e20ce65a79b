#!/usr/bin/env python3
"""Time of one Vec3 codebook-training step (VQVAE(3, 64, 4096)) on one GPU, split into the encoder (encode_device: encoder
chain + nearest-code search, the work a step shares with inference) and what training adds: the statistics call
(train_vq_stats_device = encoder + search + flat latent + statistics) minus the encoder, and the EMA update with the table
rebuild (train_vq_update_device).  Inputs are resident on the device; device events around each call, after a warm-up,
median of the repeats.  At 1 024 and 16 384 leaves per rank, plus the 16 384-identical-leaf batch whose rows all fall into
one code (its statistics against the uniform batch's).  Prints one JSON object and writes it with --out.

    python tools/vec3_train_bench.py [--sizes 1024,16384] [--reps 10] [--out profiles/vec3_train_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--sizes", default="1024,16384")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import HipVec3Codec

    W = synth_vec3.make_weights(0)
    hot = dict(W)
    e = np.array(W["quantizer.embedding"], np.float32)
    e[1:] += 100.0   # every row goes to code 0
    hot["quantizer.embedding"] = e
    stream = torch.cuda.Stream()
    h = stream.cuda_stream

    def measure(pack, leaves):
        c = HipVec3Codec(weightpack.dumps(pack))
        c.train_begin()
        n = leaves.shape[0]
        x = torch.from_numpy(np.ascontiguousarray(leaves)).cuda()
        idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
        st = torch.zeros(66 * c.model_info()["num_codes"] + 1, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enc = timed(lambda: c.encode_device(x.data_ptr(), n, idx.data_ptr(), stream=h), a.reps, a.warmup)
            stats = timed(lambda: c.train_vq_stats_device(x.data_ptr(), n, st.data_ptr(), stream=h), a.reps, a.warmup)
            # a zero-statistics update (decay 1) keeps the codebook as it is, so every repeat does the same work
            upd = timed(lambda: c.train_vq_update_device(st.data_ptr(), 1.0, 1e-4, stream=h), a.reps, a.warmup)
        used = int((st.cpu().numpy()[:c.model_info()["num_codes"]] > 0).sum())
        c.close()
        added = stats - enc + upd
        return {"leaves": n, "encoder_ms": round(enc, 4), "stats_call_ms": round(stats, 4), "stats_only_ms": round(stats - enc, 4),
                "update_ms": round(upd, 4), "step_ms": round(stats + upd, 4), "training_overhead": round(added / enc, 4),
                "codes_used": used, "leaves_per_s": round(n / ((stats + upd) / 1e3))}

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "uniform": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        out["uniform"].append(measure(W, synth_vec3.make_leaves(n, seed=11)))
    nmax = max(int(s) for s in a.sizes.split(","))
    out["identical"] = measure(hot, np.repeat(synth_vec3.make_leaves(1, seed=9), nmax, axis=0))
    uni = [r for r in out["uniform"] if r["leaves"] == nmax][0]
    out["identical_vs_uniform_stats"] = round(out["identical"]["stats_only_ms"] / max(uni["stats_only_ms"], 1e-9), 3)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
