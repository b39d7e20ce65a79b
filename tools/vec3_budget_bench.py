#!/usr/bin/env python3
"""Cost of the Vec3 handle's byte-budget calls on compact records on one GPU, each against the two calls it replaces, in
the same process.

    python tools/vec3_budget_bench.py [--leaves 16384] [--warmup 3] [--reps 10] [--dir DIR] [--out profiles/vec3_budget_bench.json]

Wall times of the C calls through ctypes with every buffer allocated beforehand, the two sides alternating rep by rep, in both
precision modes, on the all-ones mask and on the 0.086-share mask of tools/vec3_file_bench.py (same leaves, same thinning), with a
ladder of 16 rungs, geometric around the median leaf error of the fp32 round trip over a factor of 16 either way, and a budget that is
the size at the ladder's ninth rung:
    budget_compress        against   active_sweep + active_compress at the rung it picks
    budget_file_compress   against   active_sweep + file_compress_active at the rung it picks
Bar: the new call <= 1.02 x the sum of its siblings (it saves the second encoder pass; 0.02 is the run-to-run movement).  Also
recorded, without a bar: the time of pass 2 alone, as the one-rung call minus the one-rung sweep, at tolerances that select none,
about half and all of the leaves.  The file goes to --dir: /dev/shm (tmpfs) where it exists, else the working directory.  Prints one
JSON object and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BAR = 1.02
RUNGS = 16
DENSITIES = (1.0, 0.5, 0.1)      # vec3_file_bench's sequence; 0.5 is drawn and dropped so that 0.1 sees the same random numbers
MEASURED = (1.0, 0.1)
NAME = "velocity"


def summary(times):
    return {"median_ms": float(np.median(times)) * 1e3, "min_ms": float(min(times)) * 1e3, "max_ms": float(max(times)) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vec3_budget_bench.json"))
    a = ap.parse_args()

    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd import codec as vc
    from vqvdb_amd.codec import HipVec3Codec, StreamStats, pack_masks

    tmpfs = a.dir is None and os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK)
    where = a.dir or ("/dev/shm" if tmpfs else os.getcwd())
    path = os.path.join(where, f"vec3_budget_bench_{os.getpid()}.vqv3")
    ref_path = path + ".ref"
    n = a.leaves

    def paired(new_call, siblings, check=None):
        for _ in range(a.warmup):
            new_call()
            siblings()
        tn, ts = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            new_call()
            tn.append(time.perf_counter() - t)
            t = time.perf_counter()
            siblings()
            ts.append(time.perf_counter() - t)
        if check:
            check()
        r = {"new_call": summary(tn), "siblings": summary(ts)}
        r["new_over_siblings"] = r["new_call"]["median_ms"] / r["siblings"]["median_ms"]
        r["median_of_paired_ratios"] = float(np.median([x / y for x, y in zip(tn, ts)]))
        r["meets_bar"] = r["new_over_siblings"] <= BAR
        return r

    pack = weightpack.dumps(synth_vec3.make_weights(0))
    host = np.ascontiguousarray(np.tile(synth_vec3.make_leaves(512, 4321), ((n + 511) // 512, 1, 1))[:n])
    rng = np.random.default_rng(5)
    data = {}
    ref = HipVec3Codec(pack)
    for density in DENSITIES:
        x = np.ascontiguousarray(np.where(rng.random((n, 512, 1)) < density, host, np.float32(0)) if density < 1 else host)
        if density not in MEASURED:
            continue
        active = (x != 0).any(axis=2) if density < 1 else np.ones((n, 512), bool)
        _, err = ref.roundtrip(x)
        tol = float(np.sort(err[:, 0])[(n - 1) // 2])                   # torch.median's choice: the lower of the two middle values
        data[density] = (x, pack_masks(active), float(active.mean()), tol)
    ref.close()

    perm = np.random.default_rng(11).permutation(n).astype(np.uint64)
    slot = perm.astype(np.int64)
    pool = np.empty((n, 512, 3), np.float32)                             # leaf i lives in slot perm[i]
    ptrs = np.ascontiguousarray(pool.ctypes.data + perm * np.uint64(6144), dtype=np.uint64)
    origins = (np.random.default_rng(3).integers(-4096, 4096, (n, 3)) * 8).astype(np.int32)
    out = {"bar": BAR, "rungs": RUNGS, "warmup": a.warmup, "reps": a.reps, "leaves": n,
           "output": "tmpfs (/dev/shm)" if tmpfs else "a directory (--dir or the working directory)", "modes": {}}
    over = []
    for mode in ("fp32", "bf16"):
        c = HipVec3Codec(pack, precision=mode)
        lib, h = c._lib, c._h
        out["modes"][mode] = {}

        def ok(rc):
            if rc != 0:
                raise RuntimeError(lib.vqhip_vec3_last_error(h).decode())

        for density in MEASURED:
            x, masks, share, tol = data[density]
            pool[slot] = x
            ladder = np.geomspace(tol / 16, tol * 16, RUNGS).astype(np.float32)
            src = (vc._Vec3GridSource * 1)()
            src[0].name, src[0].leaf_ptrs, src[0].origins, src[0].n_leaves, src[0].masks = NAME.encode(), ptrs.ctypes.data, origins.ctypes.data, n, masks.ctypes.data
            sizes, bsizes = np.empty(RUNGS, np.int64), np.empty(RUNGS, np.int64)
            idx, bidx = np.empty((n, 64), np.uint16), np.empty((n, 64), np.uint16)
            code, bcode = np.empty(n, np.uint16), np.empty(n, np.uint16)
            payload, bpayload = np.empty(n * 6144, np.uint8), np.empty(n * 6144, np.uint8)
            nbytes, bnbytes, used, fused, fsize, pb, rpb = (ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_float(0), ctypes.c_float(0), ctypes.c_int64(0),
                                                            ctypes.c_int64(0), ctypes.c_int64(0))
            st, rst = StreamStats(), StreamStats()

            def sweep(t=ladder, dst=sizes):
                ok(lib.vqhip_vec3_active_sweep(h, x.ctypes.data, masks.ctypes.data, n, t.ctypes.data, len(t), dst.ctypes.data))

            sweep()
            budget = int(sizes[8])
            picked = vc.vec3_active_rate_pick(sizes, ladder, budget)
            tol_used = float(ladder[picked])
            file_budget = 24 + 102 + len(NAME) + n * 206 + budget
            r = {"active_share": share, "median_tolerance": tol, "ladder": [float(t) for t in ladder], "sizes": [int(s) for s in sizes],
                 "payload_budget": budget, "file_budget": file_budget, "picked_rung": picked, "tol_used": tol_used}

            def budget_compress(t=ladder, b=budget):
                ok(lib.vqhip_vec3_budget_compress(h, x.ctypes.data, masks.ctypes.data, n, t.ctypes.data, len(t), b, ctypes.byref(used), bsizes.ctypes.data,
                                                  bidx.ctypes.data, None, bcode.ctypes.data, bpayload.ctypes.data, ctypes.byref(bnbytes)))

            def compress():
                ok(lib.vqhip_vec3_active_compress(h, x.ctypes.data, masks.ctypes.data, n, tol_used, idx.ctypes.data, None, code.ctypes.data, payload.ctypes.data,
                                                  ctypes.byref(nbytes)))

            def two_calls():
                sweep()
                compress()

            def same_memory():
                assert used.value == np.float32(tol_used) and bnbytes.value == nbytes.value == sizes[picked] <= budget
                assert np.array_equal(bsizes, sizes) and np.array_equal(bidx, idx) and np.array_equal(bcode, code)
                assert bpayload[:bnbytes.value].tobytes() == payload[:nbytes.value].tobytes(), "the budget call is not compress_active at its rung"

            r["budget_compress"] = paired(budget_compress, two_calls, same_memory)
            r["selected_leaves_at_the_picked_rung"] = int((code != vc.VEC3_RES_KEPT).sum())

            def budget_file():
                ok(lib.vqhip_vec3_budget_file_compress(h, path.encode(), src, 1, ladder.ctypes.data, RUNGS, file_budget, 0, ctypes.byref(st), ctypes.byref(fused),
                                                       ctypes.byref(pb), ctypes.byref(fsize)))

            def two_file_calls():
                sweep()
                ok(lib.vqhip_vec3_file_compress_active(h, ref_path.encode(), src, 1, tol_used, 0, ctypes.byref(rst), ctypes.byref(rpb)))

            def same_file():
                assert fused.value == np.float32(tol_used) and pb.value == rpb.value == sizes[picked]
                assert fsize.value == os.path.getsize(path) == os.path.getsize(ref_path) <= file_budget
                with open(path, "rb") as f, open(ref_path, "rb") as g:
                    assert f.read() == g.read(), "the budget file is not compress_file_active's at its rung"

            r["budget_file_compress"] = paired(budget_file, two_file_calls, same_file)
            r["budget_file_compress"]["stream_stats"] = st.as_dict()
            r["file_bytes"] = fsize.value

            # pass 2 alone: the one-rung call minus the one-rung sweep
            _, _, _, merr = c.compress_active(x[:2048], masks[:2048], float("inf"), return_leaf_err=True)
            half = float(np.sort(merr[:, 0])[len(merr) // 2])
            low = float(np.float32(merr[:, 0].min()) / 2)
            r["pass_2"] = {}
            one = np.empty(1, np.int64)
            for label, t1 in (("none_selected", float("inf")), ("half_selected", half), ("all_selected", low)):
                rung = np.array([t1], np.float32)
                for _ in range(a.warmup):
                    budget_compress(rung, 1 << 40)
                    sweep(rung, one)
                tc, tsw = [], []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    budget_compress(rung, 1 << 40)
                    tc.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    sweep(rung, one)
                    tsw.append(time.perf_counter() - t)
                r["pass_2"][label] = {"tolerance": t1, "selected_leaves": int((bcode != vc.VEC3_RES_KEPT).sum()), "payload_bytes": bnbytes.value,
                                      "call": summary(tc), "sweep": summary(tsw),
                                      "pass_2_ms": (float(np.median(tc)) - float(np.median(tsw))) * 1e3}
            over += [f"modes.{mode}.{density}.{k}" for k in ("budget_compress", "budget_file_compress") if not r[k]["meets_bar"]]
            out["modes"][mode][str(density)] = r
        c.close()
    for p in (path, ref_path):
        if os.path.exists(p):
            os.remove(p)
    out["over_the_bar"] = over
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
