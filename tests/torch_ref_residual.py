"""numpy float32 restatement of the quantised residuals (include/vqvdb_hip_residual.h): classify, pack, apply and
record_size, written from the arithmetic and the record layout alone.  Every operation is one float32 numpy operation (no fma),
so the GPU kernels' unfused float32 arithmetic gives the same bits.

    step = 1.875f * tol      d = x - x^      t = d / step      q = rint(t)      x~ = x^ + float32(q) * step
    a voxel verifies iff |t| <= 32767 and |x - x~| <= tol (false on NaN)
"""
import numpy as np

KEPT, RAW = 254, 255
F = np.float32


def record_size(cls):
    """bytes of the record of one class (array or scalar)."""
    c = np.asarray(cls).astype(np.int64)
    return np.where(c == KEPT, 0, np.where(c == RAW, 2048, 64 * c))


def step_of(tol):
    with np.errstate(all="ignore"):
        return F(1.875) * F(tol)


def quantise(x, recon, tol):
    """-> (q int32 [n,512] (0 where the voxel does not fit), verified bool [n,512])."""
    x, recon, tol = np.asarray(x, F), np.asarray(recon, F), F(tol)
    step = step_of(tol)
    with np.errstate(all="ignore"):
        t = (x - recon) / step
        fits = np.abs(t) <= F(32767.0)
        q = np.where(fits, np.rint(t), F(0)).astype(np.int32)
        xt = recon + q.astype(F) * step
        ok = fits & (np.abs(x - xt) <= tol)
    return q, ok


def zigzag(q):
    q = np.asarray(q, np.int32)
    return ((q << 1) ^ (q >> 31)).astype(np.uint32)


def unzigzag(zz):
    zz = np.asarray(zz, np.uint32)
    return (zz >> np.uint32(1)).astype(np.int32) ^ -(zz & np.uint32(1)).astype(np.int32)


def classify(x, recon, leaf_err, tol):
    """-> (class uint8 [n], offsets int64 [n+1]): offsets[i] the start of leaf i's record, offsets[n] the payload's size."""
    x = np.asarray(x, F).reshape(-1, 512)
    n = len(x)
    with np.errstate(invalid="ignore"):
        kept = np.asarray(leaf_err, F).reshape(n, -1)[:, 0] <= F(tol)
    q, ok = quantise(x, np.asarray(recon, F).reshape(n, 512), tol)
    top = zigzag(q).max(axis=1) if n else np.zeros(0, np.uint32)
    bits = np.array([int(v).bit_length() for v in top], dtype=np.int64)
    cls = np.where(kept, KEPT, np.where(ok.all(axis=1), bits, RAW)).astype(np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(record_size(cls), out=off[1:])
    return cls, off


def pack_leaf(x_leaf, recon_leaf, tol, cls):
    """the record bytes of one leaf of class cls."""
    if cls == KEPT:
        return b""
    if cls == RAW:
        return np.asarray(x_leaf, "<f4").tobytes()
    q, _ = quantise(x_leaf.reshape(1, 512), recon_leaf.reshape(1, 512), tol)
    zz = zigzag(q[0]).astype(np.uint64).reshape(8, 64)              # [word j][bit L] = voxel 64 j + L
    words = np.zeros((int(cls), 8), dtype="<u8")
    for k in range(int(cls)):
        plane = (zz >> np.uint64(k)) & np.uint64(1)
        words[k] = (plane << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return words.tobytes()


def pack(x, recon, tol, cls):
    """-> payload bytes: the records of all leaves in leaf order."""
    x, recon = np.asarray(x, F).reshape(-1, 512), np.asarray(recon, F).reshape(-1, 512)
    return b"".join(pack_leaf(x[i], recon[i], tol, int(c)) for i, c in enumerate(cls))


def records(cls, payload):
    """-> list of the record bytes of every leaf (b'' for kept leaves)."""
    off = np.concatenate([[0], np.cumsum(record_size(cls))])
    assert off[-1] == len(payload)
    return [bytes(payload[off[i]:off[i + 1]]) for i in range(len(cls))]


def unpack_leaf(rec, cls):
    """q int32 [512] of a quantised record."""
    words = np.frombuffer(rec, dtype="<u8").reshape(int(cls), 8).astype(np.uint64)
    zz = np.zeros((8, 64), np.uint32)
    for k in range(int(cls)):
        bit = (words[k][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
        zz |= bit.astype(np.uint32) << np.uint32(k)
    return unzigzag(zz.reshape(512))


def apply(recon, tol, cls, payload):
    """-> x~ float32 [n,512]: decoded leaves with their records applied."""
    out = np.array(recon, dtype=F).reshape(-1, 512).copy()
    step = step_of(tol)
    for i, (c, rec) in enumerate(zip(cls, records(cls, payload))):
        c = int(c)
        if c == KEPT:
            continue
        if c == RAW:
            out[i] = np.frombuffer(rec, dtype="<f4")
        else:
            with np.errstate(all="ignore"):
                out[i] = out[i] + unpack_leaf(rec, c).astype(F) * step
    return out


def leaf_with_max_q(qmax, tol=0.5, rng=None, negative=False):
    """(x, recon) of one leaf whose q of largest magnitude is +-qmax (at voxel 7), the others 0 or, with rng, in -1 .. 1.
    recon = 0 and x = q * step; with tol = 0.5 the step is 0.9375, so x and t = x / step = q are exact."""
    q = np.zeros(512, np.int64)
    if rng is not None and qmax >= 1:
        q[:] = rng.integers(-1, 2 if qmax >= 2 else 1, 512)          # +1 has zz = 2, two bits: not beside a largest q of -1
    q[7] = -qmax if negative else qmax
    return (q.astype(F) * step_of(tol)).astype(F), np.zeros(512, F)
