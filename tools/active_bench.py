#!/usr/bin/env python3
"""Cost and gain of the compact residual records on one GPU, against the masked and unmasked calls in the same process.

    python tools/active_bench.py [--leaves 16384] [--warmup 3] [--reps 15] [--out profiles/active_bench.json]

Vec3 leaves resident in HBM, device events on one stream, the two sides alternating rep by rep, for three masks: all ones, and the
same leaves thinned voxel by voxel at densities 0.5 and 0.1 with mask = (x != 0) (tools/mask_bench.py's thinning: active shares 0.43
and 0.086), each at the median leaf error of its own round trip:
    active_encode_device   against   mask_residual_encode_device, same inputs            (bar 1.10 at the all-ones mask, none elsewhere)
    active_apply_device    against   residual_apply_device on the masked records         (no bar)
    active_sweep_device    against   mask_sweep_device at 1, 16 and 64 rungs              (no bar)
and the payload bytes of the compact against the masked encode.  At the all-ones mask the two payloads must be the same bytes.
Prints one JSON object and writes it to --out (profiles/active_bench.json by default)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNGS = (1, 16, 64)
BAR = 1.10
DENSITIES = (1.0, 0.5, 0.1)


def summary(times):
    return {"median_ms": float(np.median(times)) * 1e3, "min_ms": float(min(times)) * 1e3, "max_ms": float(max(times)) * 1e3}


def ladder(med, rungs):
    return [med] if rungs == 1 else [float(v) for v in np.geomspace(med / 16, med * 16, rungs).astype(np.float32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "active_bench.json"))
    a = ap.parse_args()

    import torch
    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd.codec import HipVec3Codec, pack_masks

    st = torch.cuda.Stream()
    h = st.cuda_stream

    def event_time(fn, before=None):
        if before:
            before()
            torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        fn()
        e.record(st)
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    def paired(compact, other, other_name, before=None):
        for _ in range(a.warmup):
            compact()
            other()
        torch.cuda.synchronize()
        tc, to = [], []
        for _ in range(a.reps):
            tc.append(event_time(compact, before))
            to.append(event_time(other, before))
        r = {"compact": summary(tc), other_name: summary(to)}
        r["compact_over_" + other_name] = r["compact"]["median_ms"] / r[other_name]["median_ms"]
        r["median_of_paired_ratios"] = float(np.median([x / y for x, y in zip(tc, to)]))
        return r

    c = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0)))
    n = a.leaves
    host = np.ascontiguousarray(np.tile(synth_vec3.make_leaves(512, 4321), ((n + 511) // 512, 1, 1))[:n])
    rng = np.random.default_rng(5)
    out = {"bar_encode_all_ones": BAR, "warmup": a.warmup, "reps": a.reps, "leaves": n, "masks": {}}
    for density in DENSITIES:
        x = np.ascontiguousarray(np.where(rng.random((n, 512, 1)) < density, host, np.float32(0)) if density < 1 else host)
        active = (x != 0).any(axis=2) if density < 1 else np.ones((n, 512), bool)
        leaves, masks = torch.from_numpy(x).cuda(), torch.from_numpy(pack_masks(active).view(np.int64)).cuda()
        idx = torch.empty((n, 64), dtype=torch.int16, device="cuda")
        rec, work = (torch.empty((n, 512, 3), dtype=torch.float32, device="cuda") for _ in range(2))
        err, merr = (torch.empty((n, 2), dtype=torch.float32, device="cuda") for _ in range(2))
        code, mcode = (torch.empty((n,), dtype=torch.int16, device="cuda") for _ in range(2))
        off, moff = (torch.empty((n + 1,), dtype=torch.int64, device="cuda") for _ in range(2))
        cap = n * 6144
        pay, mpay = (torch.empty((cap,), dtype=torch.uint8, device="cuda") for _ in range(2))
        sums = torch.zeros(64, dtype=torch.int64, device="cuda")
        hist = torch.zeros((64, 51), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        c.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr(), h)
        c.mask_leaf_err_device(leaves.data_ptr(), rec.data_ptr(), masks.data_ptr(), n, merr.data_ptr(), h)
        torch.cuda.synchronize()
        tol = float(err[:, 0].median())
        p = lambda t: t.data_ptr()                                     # noqa: E731

        def enc_compact():
            c.active_encode_device(p(leaves), p(rec), p(masks), p(merr), n, tol, p(code), p(off), p(pay), cap, h)

        def enc_masked():
            c.mask_residual_encode_device(p(leaves), p(rec), p(masks), p(merr), n, tol, p(mcode), p(moff), p(mpay), cap, h)

        enc_compact()
        enc_masked()
        torch.cuda.synchronize()
        total, mtotal = int(off[-1]), int(moff[-1])
        assert torch.equal(code, mcode), "the compact encode's codes differ from the masked encode's"
        assert total <= mtotal
        if density == 1.0:
            assert torch.equal(off, moff) and torch.equal(pay[:total], mpay[:mtotal]), "all active: the records are not the masked bytes"
        r = {"active_share": float(active.mean()), "tolerance": tol, "selected": int((code != -2).sum()),   # -2: VQHIP_VEC3_RES_KEPT as int16
             "compact_payload_bytes": total, "masked_payload_bytes": mtotal, "compact_over_masked_payload": total / mtotal if mtotal else None}
        r["encode"] = paired(enc_compact, enc_masked, "masked")
        if density == 1.0:
            r["encode"]["meets_bar"] = r["encode"]["compact_over_masked"] <= BAR

        def reset():
            work.copy_(rec)

        r["apply"] = paired(lambda: c.active_apply_device(p(work), p(masks), n, tol, p(code), p(off), p(pay), None, h),
                            lambda: c.residual_apply_device(p(work), n, tol, p(mcode), p(moff), p(mpay), h), "existing", before=reset)
        r["apply_with_background"] = paired(lambda: c.active_apply_device(p(work), p(masks), n, tol, p(code), p(off), p(pay), [0.0, 0.0, 0.0], h),
                                            lambda: c.residual_apply_device(p(work), n, tol, p(mcode), p(moff), p(mpay), h), "existing", before=reset)
        r["sweep"] = {}
        for rungs in RUNGS:
            tols = ladder(tol, rungs)
            r["sweep"][str(rungs)] = paired(
                lambda: c.active_sweep_device(p(leaves), p(rec), p(masks), p(merr), n, tols, p(sums), h),
                lambda: c.mask_sweep_device(p(leaves), p(rec), p(masks), p(merr), n, tols, p(hist), h), "masked")
        sums.zero_()
        torch.cuda.synchronize()
        c.active_sweep_device(p(leaves), p(rec), p(masks), p(merr), n, [tol], p(sums), h)
        torch.cuda.synchronize()
        assert int(sums[0]) == total, "the sweep's bytes are not the encode's"
        out["masks"][str(density)] = r
        del leaves, masks, idx, rec, work, err, merr, code, mcode, off, moff, pay, mpay, sums, hist
    c.close()
    out["over_the_bar"] = [] if out["masks"]["1.0"]["encode"]["meets_bar"] else ["masks.1.0.encode"]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
