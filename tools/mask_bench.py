#!/usr/bin/env python3
"""Cost and gain of the active-voxel masks on one GPU, against the unmasked calls in the same process.

    python tools/mask_bench.py [--leaves 16384] [--warmup 3] [--reps 15] [--out profiles/mask_bench.json]

Vec3 leaves resident in HBM, device events on one stream, the two sides alternating rep by rep:
    mask_residual_encode_device with an all-ones mask   against   residual_encode_device, same inputs, median tolerance   (bar 1.05)
    mask_sweep_device with an all-ones mask             against   rate_sweep_device at 1, 16 and 64 rungs                 (bar 1.05)
    mask_leaf_err_device: ms, effective GB/s over (12288 + 64) n bytes, and its share of roundtrip_device                  (no bar)
and the payload of a masked against an unmasked encode at the median tolerance on the same leaves thinned voxel by voxel to active
densities of 1.0, 0.5 and 0.1 with mask = (x != 0) (no bar: it depends on the data).
Prints one JSON object and writes it to --out (profiles/mask_bench.json by default)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNGS = (1, 16, 64)
BAR = 1.05


def summary(times):
    return {"median_ms": float(np.median(times)) * 1e3, "min_ms": float(min(times)) * 1e3, "max_ms": float(max(times)) * 1e3}


def ladder(med, rungs):
    return [med] if rungs == 1 else [float(v) for v in np.geomspace(med / 16, med * 16, rungs).astype(np.float32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_bench.json"))
    a = ap.parse_args()

    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import HipVec3Codec, pack_masks

    st = torch.cuda.Stream()
    h = st.cuda_stream

    def event_time(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    def paired(masked, plain):
        for _ in range(a.warmup):
            masked()
            plain()
        torch.cuda.synchronize()
        tm, tp = [], []
        for _ in range(a.reps):
            tm.append(event_time(masked))
            tp.append(event_time(plain))
        r = {"masked": summary(tm), "unmasked": summary(tp)}
        r["masked_over_unmasked"] = r["masked"]["median_ms"] / r["unmasked"]["median_ms"]
        r["median_of_paired_ratios"] = float(np.median([x / y for x, y in zip(tm, tp)]))
        r["meets_bar"] = r["masked_over_unmasked"] <= BAR
        return r

    def handle(c, host):
        n = len(host)
        C, leaf, classes = 3, (512, 3), 51
        leaves = torch.from_numpy(host).cuda()
        idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
        rec = torch.empty((n,) + leaf, dtype=torch.float32, device="cuda")
        err, merr = (torch.empty((n, 2), dtype=torch.float32, device="cuda") for _ in range(2))
        ones = torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
        code = torch.empty((n,), dtype=torch.int16, device="cuda")
        off = torch.empty((n + 1,), dtype=torch.int64, device="cuda")
        cap = n * 2048 * C
        pay = torch.empty((cap,), dtype=torch.uint8, device="cuda")
        hist = torch.zeros((64, classes), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def roundtrip():
            c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)

        def masked_err():
            c.mask_leaf_err_device(leaves.data_ptr(), rec.data_ptr(), ones.data_ptr(), n, merr.data_ptr(), h)

        roundtrip()
        masked_err()
        torch.cuda.synchronize()
        assert torch.equal(err.view(torch.int32), merr.view(torch.int32)), "an all-ones mask does not give the unmasked error bits"
        med = float(err[:, 0].median())
        res = {"leaves": n, "chunk_leaves": c.chunk_leaves(), "median_leaf_error": med}

        def enc_masked():
            c.mask_residual_encode_device(leaves.data_ptr(), rec.data_ptr(), ones.data_ptr(), err.data_ptr(), n, med, code.data_ptr(), off.data_ptr(),
                                          pay.data_ptr(), cap, h)

        def enc_plain():
            c.residual_encode_device(leaves.data_ptr(), rec.data_ptr(), err.data_ptr(), n, med, code.data_ptr(), off.data_ptr(), pay.data_ptr(), cap, h)

        enc_masked()
        torch.cuda.synchronize()
        keep = (code.clone(), off.clone(), pay[:int(off[-1])].clone())
        enc_plain()
        torch.cuda.synchronize()
        assert torch.equal(keep[0], code) and torch.equal(keep[1], off) and torch.equal(keep[2], pay[:int(off[-1])]), "all-ones encode differs"
        res["encode_all_ones"] = paired(enc_masked, enc_plain)
        res["encode_all_ones"]["payload_bytes"] = int(off[-1])
        res["sweep_all_ones"] = {}
        for rungs in RUNGS:
            tols = ladder(med, rungs)
            res["sweep_all_ones"][str(rungs)] = paired(
                lambda: c.mask_sweep_device(leaves.data_ptr(), rec.data_ptr(), ones.data_ptr(), err.data_ptr(), n, tols, hist.data_ptr(), h),
                lambda: c.rate_sweep_device(leaves.data_ptr(), rec.data_ptr(), err.data_ptr(), n, tols, hist.data_ptr(), h))
        for _ in range(a.warmup):
            masked_err()
            roundtrip()
        t_err, t_rt = [], []
        for _ in range(a.reps):
            t_err.append(event_time(masked_err))
            t_rt.append(event_time(roundtrip))
        e = summary(t_err)
        e["effective_GB_per_s"] = (4096 * C + 64) * n / (e["median_ms"] * 1e-3) / 1e9
        e["roundtrip_device"] = summary(t_rt)
        e["share_of_roundtrip_device"] = e["median_ms"] / e["roundtrip_device"]["median_ms"]
        res["masked_error_pass"] = e
        return res

    out = {"bar": BAR, "warmup": a.warmup, "reps": a.reps}
    c = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0)))
    n = a.leaves
    host = np.ascontiguousarray(np.tile(synth_vec3.make_leaves(512, 4321), ((n + 511) // 512, 1, 1))[:n])
    out["vec3"] = handle(c, host)

    # the payload on the same leaves thinned voxel by voxel to three active densities, mask = (x != 0)
    rng = np.random.default_rng(5)
    out["vec3"]["payload_by_density"] = {}
    for density in (1.0, 0.5, 0.1):
        x = np.ascontiguousarray(np.where(rng.random((n, 512, 1)) < density, host, np.float32(0)) if density < 1 else host)
        active = (x != 0).any(axis=2) if density < 1 else np.ones((n, 512), bool)
        leaves, masks = torch.from_numpy(x).cuda(), torch.from_numpy(pack_masks(active).view(np.int64)).cuda()
        idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
        rec = torch.empty((n, 512, 3), dtype=torch.float32, device="cuda")
        err, merr = (torch.empty((n, 2), dtype=torch.float32, device="cuda") for _ in range(2))
        code, off = torch.empty((n,), dtype=torch.int16, device="cuda"), torch.empty((n + 1,), dtype=torch.int64, device="cuda")
        pay = torch.empty((n * 6144,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)
        c.mask_leaf_err_device(leaves.data_ptr(), rec.data_ptr(), masks.data_ptr(), n, merr.data_ptr(), h)
        torch.cuda.synchronize()
        tol = float(err[:, 0].median())
        c.residual_encode_device(leaves.data_ptr(), rec.data_ptr(), err.data_ptr(), n, tol, code.data_ptr(), off.data_ptr(), pay.data_ptr(), n * 6144, h)
        torch.cuda.synchronize()
        plain, plain_sel = int(off[-1]), int((code != -2).sum())       # -2: the bits of VQHIP_VEC3_RES_KEPT in an int16
        c.mask_residual_encode_device(leaves.data_ptr(), rec.data_ptr(), masks.data_ptr(), merr.data_ptr(), n, tol, code.data_ptr(), off.data_ptr(),
                                      pay.data_ptr(), n * 6144, h)
        torch.cuda.synchronize()
        masked, masked_sel = int(off[-1]), int((code != -2).sum())
        assert masked <= plain
        out["vec3"]["payload_by_density"][str(density)] = {
            "active_share": float(active.mean()), "tolerance": tol, "unmasked_payload_bytes": plain, "masked_payload_bytes": masked,
            "masked_over_unmasked": masked / plain if plain else None, "unmasked_selected": plain_sel, "masked_selected": masked_sel}
        del leaves, masks, idx, rec, err, merr, code, off, pay
    c.close()
    r = out["vec3"]
    out["over_the_bar"] = [name for name, v in [("encode_all_ones", r["encode_all_ones"])] + [(f"sweep_all_ones.{g}", v) for g, v in r["sweep_all_ones"].items()]
                           if not v["meets_bar"]]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
