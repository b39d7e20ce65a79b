#!/usr/bin/env python3
"""Cost of the Vec3 handle's leaf-pointer and .vqv3 file calls on one GPU, each against its in-memory sibling in the
same process.

    python tools/vec3_file_bench.py [--leaves 16384] [--warmup 3] [--reps 10] [--dir DIR] [--out profiles/vec3_file_bench.json]

Wall times of the C calls through ctypes with every buffer allocated beforehand, the two sides alternating rep by rep, in both
precision modes, on the all-ones mask and on the 0.086-share mask of tools/active_bench.py (same leaves, same thinning, same
tolerance: the median leaf error of the fp32 round trip):
    file_compress_active   against   active_compress on the same leaves packed contiguously
    file_decompress        against   active_decompress
    encode_leaves          against   encode
    decode_leaves          against   decode
The leaf pointers address the slots of one pool in a shuffled order, so that gather and scatter do not walk memory in sequence.
Bar: file call <= 1.10 x its sibling in bf16 mode.  The file goes to --dir: /dev/shm (tmpfs) where it exists, else the working
directory; the JSON says which.  Also written down: the file's bytes per leaf, which are the payload of profiles/active_bench.json
(fp32 mode) plus 12 + 128 + 64 + 2 B per leaf plus the headers.  Prints one JSON object and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BAR = 1.10
DENSITIES = (1.0, 0.5, 0.1)      # active_bench's sequence; 0.5 is drawn and dropped so that 0.1 sees the same random numbers
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vec3_file_bench.json"))
    a = ap.parse_args()

    from vqvdb_amd import synth_vec3, weightpack
    from vqvdb_amd import codec as vc
    from vqvdb_amd.codec import HipVec3Codec, StreamStats, pack_masks

    tmpfs = a.dir is None and os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK)
    where = a.dir or ("/dev/shm" if tmpfs else os.getcwd())
    path = os.path.join(where, f"vec3_file_bench_{os.getpid()}.vqv3")
    n = a.leaves

    def paired(file_call, sibling, check=None):
        for _ in range(a.warmup):
            file_call()
            sibling()
        tf, ts = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            file_call()
            tf.append(time.perf_counter() - t)
            t = time.perf_counter()
            sibling()
            ts.append(time.perf_counter() - t)
        if check:
            check()
        r = {"file_call": summary(tf), "sibling": summary(ts)}
        r["file_over_sibling"] = r["file_call"]["median_ms"] / r["sibling"]["median_ms"]
        r["median_of_paired_ratios"] = float(np.median([x / y for x, y in zip(tf, ts)]))
        r["meets_bar"] = r["file_over_sibling"] <= BAR
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
    try:
        with open(os.path.join(ROOT, "profiles", "active_bench.json")) as f:
            recorded = {k: v["compact_payload_bytes"] for k, v in json.load(f)["masks"].items()} if n == 16384 else {}
    except OSError:
        recorded = {}

    perm = np.random.default_rng(11).permutation(n).astype(np.uint64)
    slot = perm.astype(np.int64)
    pool = np.empty((n, 512, 3), np.float32)                             # leaf i lives in slot perm[i]
    ptrs = np.ascontiguousarray(pool.ctypes.data + perm * np.uint64(6144), dtype=np.uint64)
    origins = (np.random.default_rng(3).integers(-4096, 4096, (n, 3)) * 8).astype(np.int32)
    out = {"bar_bf16": BAR, "warmup": a.warmup, "reps": a.reps, "leaves": n,
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
            src = (vc._Vec3GridSource * 1)()
            src[0].name, src[0].leaf_ptrs, src[0].origins, src[0].n_leaves, src[0].masks = NAME.encode(), ptrs.ctypes.data, origins.ctypes.data, n, masks.ctypes.data
            st_c, st_d, pb = StreamStats(), StreamStats(), ctypes.c_int64(0)
            idx, fidx = np.empty((n, 64), np.uint16), np.empty((n, 64), np.uint16)
            code, payload, nbytes = np.empty(n, np.uint16), np.empty(n * 6144, np.uint8), ctypes.c_int64(0)
            dec = np.empty((n, 512, 3), np.float32)

            def file_compress():
                ok(lib.vqhip_vec3_file_compress_active(h, path.encode(), src, 1, tol, 0, ctypes.byref(st_c), ctypes.byref(pb)))

            def mem_compress():
                ok(lib.vqhip_vec3_active_compress(h, x.ctypes.data, masks.ctypes.data, n, tol, idx.ctypes.data, None, code.ctypes.data, payload.ctypes.data,
                                                  ctypes.byref(nbytes)))

            r = {"active_share": share, "tolerance": tol}
            r["compress_file_active"] = paired(file_compress, mem_compress)
            assert pb.value == nbytes.value, "the file's payload is not compress_active's"
            size = os.path.getsize(path)
            assert size == 24 + 102 + len(NAME) + n * 206 + nbytes.value
            r.update(payload_bytes=nbytes.value, file_bytes=size, payload_bytes_per_leaf=nbytes.value / n, file_bytes_per_leaf=size / n,
                     fixed_bytes_per_leaf=206, header_bytes=24 + 102 + len(NAME))
            if mode == "fp32" and str(density) in recorded:
                r["active_bench_payload_bytes"] = recorded[str(density)]
                r["agrees_with_active_bench"] = recorded[str(density)] == nbytes.value
            r["compress_file_active"]["stream_stats"] = st_c.as_dict()
            at = [0]

            def on_alloc(_user, _g, _origins, _masks, m, out_ptrs):
                ctypes.memmove(out_ptrs, ptrs.ctypes.data + 8 * at[0], 8 * m)
                at[0] = (at[0] + m) % n
                return 0

            cb_g, cb_a = vc.VEC3_GRID_BEGIN_FN(), vc.VEC3_LEAF_ALLOC_FN(on_alloc)
            pl = payload[:nbytes.value]

            def file_decompress():
                ok(lib.vqhip_vec3_file_decompress(h, path.encode(), 0, cb_g, cb_a, None, ctypes.byref(st_d)))

            def mem_decompress():
                ok(lib.vqhip_vec3_active_decompress(h, idx.ctypes.data, masks.ctypes.data, n, tol, code.ctypes.data, pl.ctypes.data, nbytes.value, None,
                                                    dec.ctypes.data))

            def same_leaves():
                assert pool[slot].tobytes() == dec.tobytes(), "the leaf-pointer side is not its sibling"

            def same_indices():
                assert np.array_equal(fidx, idx), "encode_leaves is not encode"

            r["decompress_file"] = paired(file_decompress, mem_decompress, same_leaves)
            r["decompress_file"]["stream_stats"] = st_d.as_dict()
            pool[slot] = x
            r["encode_leaves"] = paired(lambda: ok(lib.vqhip_vec3_encode_leaves(h, ptrs.ctypes.data, n, fidx.ctypes.data)),
                                        lambda: ok(lib.vqhip_vec3_encode(h, x.ctypes.data, n, idx.ctypes.data)), same_indices)
            r["decode_leaves"] = paired(lambda: ok(lib.vqhip_vec3_decode_leaves(h, idx.ctypes.data, n, ptrs.ctypes.data)),
                                        lambda: ok(lib.vqhip_vec3_decode(h, idx.ctypes.data, n, dec.ctypes.data)), same_leaves)
            if mode == "bf16":
                over += [f"modes.bf16.{density}.{k}" for k in ("compress_file_active", "decompress_file", "encode_leaves", "decode_leaves") if not r[k]["meets_bar"]]
            out["modes"][mode][str(density)] = r
        c.close()
    if os.path.exists(path):
        os.remove(path)
    out["over_the_bar"] = over
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
