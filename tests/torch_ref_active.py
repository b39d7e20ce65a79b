"""numpy restatement of the compact residual records of the Vec3 handle (include/vqvdb_hip_vec3_active.h) — TEST
INFRASTRUCTURE, written from the format's definition, not from the kernels: A = the active voxels of a leaf, W = ceil(A / 64), the
rank of an active voxel = the active voxels with a smaller index.

    kept        no record
    quantised   8 W (b0 + b1 + b2) bytes: channel by channel, plane k of channel c = W little-endian u64 words,
                bit L of word j = bit k of zz(q) of the active voxel of rank 64 j + L, 0 at ranks >= A
    raw         8 ceil(3 A / 2) bytes: the active voxels' three float32 each in rank order, then zero bytes

Classification (the codes) and quantise are tests/torch_ref_masked.py's, unchanged; three channels only."""
import numpy as np

import torch_ref_masked as trm
import torch_ref_vec3_residual as t3r

F = np.float32
KEPT, RAW = t3r.KEPT, t3r.RAW


def ranks(active) -> np.ndarray:
    """bool [n,512] -> int64 [n,512]: the number of active voxels with a smaller index (meaningful at active voxels)."""
    a = np.asarray(active, bool).reshape(-1, 512).astype(np.int64)
    return np.cumsum(a, axis=1) - a


def record_size(code, A):
    """bytes of the record of a code (array or scalar) on a leaf with A active voxels"""
    c, A = np.asarray(code).astype(np.int64), np.asarray(A).astype(np.int64)
    planes = t3r.widths(c).sum(axis=-1)
    return np.where(c == KEPT, 0, np.where(c == RAW, 8 * -(-3 * A // 2), 8 * -(-A // 64) * planes))


def offsets(code, active) -> np.ndarray:
    off = np.zeros(len(code) + 1, np.int64)
    np.cumsum(record_size(code, np.asarray(active, bool).reshape(-1, 512).sum(axis=1)), out=off[1:])
    return off


def _planes(zz_by_rank, b, W):
    """the 8 W b bytes of one channel: zz uint32 [A] in rank order -> planes 0 .. b-1 of W words"""
    z = np.zeros(64 * W, np.uint64)
    z[:len(zz_by_rank)] = zz_by_rank
    z = z.reshape(W, 64)
    words = np.zeros((int(b), W), dtype="<u8")
    for k in range(int(b)):
        plane = (z >> np.uint64(k)) & np.uint64(1)
        words[k] = (plane << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return words.tobytes()


def pack(x, recon, tol, code, active) -> bytes:
    """-> payload bytes: the compact records of all leaves in leaf order"""
    xs = trm._values(x, 3)
    act = np.asarray(active, bool).reshape(-1, 512)
    zz, _ = trm.quantise(x, recon, tol, act, 3)
    zz = zz.reshape(len(xs), 512, 3)
    out = []
    for i, c in enumerate(code):
        c = int(c)
        if c == KEPT:
            continue
        on = np.flatnonzero(act[i])                                    # ascending index = rank order
        A = len(on)
        if c == RAW:
            rec = np.ascontiguousarray(xs[i][on], "<f4").tobytes()
            out.append(rec + bytes(-len(rec) % 8))
            continue
        W = -(-A // 64)
        for ch in range(3):
            out.append(_planes(zz[i, on, ch], (c >> (5 * ch)) & 31, W))
    return b"".join(out)


def records(code, payload, active):
    off = offsets(code, active)
    assert off[-1] == len(payload), (off[-1], len(payload))
    return [bytes(payload[off[i]:off[i + 1]]) for i in range(len(code))]


def unpack_leaf(rec, code, A) -> np.ndarray:
    """q int32 [A,3] in rank order of a quantised record"""
    W = -(-A // 64)
    q = np.zeros((A, 3), np.int32)
    at = 0
    for ch, b in enumerate(t3r.widths(int(code))):
        b = int(b)
        words = np.frombuffer(rec[at:at + 8 * W * b], dtype="<u8").reshape(b, W)
        at += 8 * W * b
        zz = np.zeros(64 * W, np.uint32)
        for k in range(b):
            bits = (words[k][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
            zz |= bits.reshape(-1).astype(np.uint32) << np.uint32(k)
        assert not zz[A:].any(), "bits at ranks >= A"
        q[:, ch] = t3r.unzigzag(zz[:A])
    assert at == len(rec)
    return q


def apply(recon, tol, code, payload, active, background=None) -> np.ndarray:
    """-> float32 [n,512,3]: active values x^ + float32(q) * step (quantised), the record's value (raw) or x^ (kept), one float32
    operation each; inactive values keep the bits of ``recon`` or, with a background of three floats, receive its bits."""
    out = np.array(recon, dtype=F).reshape(-1, 512, 3).copy()
    act = np.asarray(active, bool).reshape(-1, 512)
    step = t3r.step_of(tol)
    for i, (c, rec) in enumerate(zip(code, records(code, payload, act))):
        c = int(c)
        on = np.flatnonzero(act[i])
        if background is not None:
            out[i][~act[i]] = np.asarray(background, F)
        if c == KEPT or len(on) == 0:
            continue
        if c == RAW:
            out[i][on] = np.frombuffer(rec[:12 * len(on)], dtype="<f4").reshape(len(on), 3)
        else:
            with np.errstate(all="ignore"):
                out[i][on] = out[i][on] + unpack_leaf(rec, c, len(on)).astype(F) * step
    return out


def sweep_bytes(x, recon, leaf_err, tols, active) -> np.ndarray:
    """-> int64 [T]: the payload bytes at every rung"""
    return np.array([offsets(trm.classify(x, recon, leaf_err, tol, active, 3)[0], active)[-1] for tol in tols], np.int64)
