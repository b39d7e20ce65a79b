"""numpy float32 restatement of the Vec3 handle's quantised residuals (include/vqvdb_hip_vec3_residual.h):
quantise, classify, pack, apply and record_size, written from the arithmetic and the record layout alone.  The arithmetic per
value is the scalar format's (tests/torch_ref_residual.py: one float32 numpy operation each, no fma); what is restated here is
the leaf [512][3] with channels last, the code with one bit width per channel and the record walked channel by channel.

    step = 1.875f * tol      d = x - x^      t = d / step      q = rint(t)      x~ = x^ + float32(q) * step
    a value verifies iff |t| <= 32767 and |x - x~| <= tol (false on NaN)
    code = 0xFFFE kept | 0xFFFF raw | b0 | b1 << 5 | b2 << 10, b_c the bits of max zz(q) over channel c
"""
import numpy as np

import torch_ref_residual as trr

KEPT, RAW = 0xFFFE, 0xFFFF
RAW_BYTES = 6144
F = np.float32
step_of, zigzag, unzigzag = trr.step_of, trr.zigzag, trr.unzigzag


def widths(code):
    """-> int64 [..., 3]: the three fields of a quantised code (meaningless for the two sentinels)."""
    c = np.asarray(code).astype(np.int64)
    return np.stack([c & 31, (c >> 5) & 31, (c >> 10) & 31], axis=-1)


def make_code(b0, b1, b2):
    return int(b0) | int(b1) << 5 | int(b2) << 10


def record_size(code):
    """bytes of the record of one code (array or scalar)."""
    c = np.asarray(code).astype(np.int64)
    return np.where(c == KEPT, 0, np.where(c == RAW, RAW_BYTES, 64 * widths(c).sum(axis=-1)))


def quantise(x, recon, tol):
    """-> (q int32 [n,512,3] (0 where the value does not fit), verified bool [n,512,3])."""
    q, ok = trr.quantise(np.asarray(x, F).reshape(-1, 512, 3), np.asarray(recon, F).reshape(-1, 512, 3), tol)
    return q, ok


def classify(x, recon, leaf_err, tol):
    """-> (code uint16 [n], offsets int64 [n+1]): offsets[i] the start of leaf i's record, offsets[n] the payload's size."""
    x = np.asarray(x, F).reshape(-1, 512, 3)
    n = len(x)
    with np.errstate(invalid="ignore"):
        kept = np.asarray(leaf_err, F).reshape(n, -1)[:, 0] <= F(tol)
    q, ok = quantise(x, recon, tol)
    top = zigzag(q).max(axis=1) if n else np.zeros((0, 3), np.uint32)                  # [n, 3]
    bits = np.array([[int(v).bit_length() for v in row] for row in top], dtype=np.int64).reshape(n, 3)
    quant = bits[:, 0] | bits[:, 1] << 5 | bits[:, 2] << 10
    code = np.where(kept, KEPT, np.where(ok.all(axis=(1, 2)), quant, RAW)).astype(np.uint16)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(record_size(code), out=off[1:])
    return code, off


def pack_channel(q, b):
    """the 64 * b bytes of one channel: q int32 [512] -> planes 0 .. b-1, eight little-endian u64 words each."""
    zz = zigzag(q).astype(np.uint64).reshape(8, 64)                                   # [word j][bit L] = voxel 64 j + L
    words = np.zeros((int(b), 8), dtype="<u8")
    for k in range(int(b)):
        plane = (zz >> np.uint64(k)) & np.uint64(1)
        words[k] = (plane << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return words.tobytes()


def pack_leaf(x_leaf, recon_leaf, tol, code):
    """the record bytes of one leaf [512,3] of the given code."""
    code = int(code)
    if code == KEPT:
        return b""
    if code == RAW:
        return np.ascontiguousarray(x_leaf, "<f4").tobytes()
    q, _ = quantise(x_leaf, recon_leaf, tol)
    return b"".join(pack_channel(q[0, :, ch], b) for ch, b in enumerate(widths(code)))


def pack(x, recon, tol, code):
    """-> payload bytes: the records of all leaves in leaf order."""
    x, recon = np.asarray(x, F).reshape(-1, 512, 3), np.asarray(recon, F).reshape(-1, 512, 3)
    return b"".join(pack_leaf(x[i], recon[i], tol, int(c)) for i, c in enumerate(code))


def records(code, payload):
    """-> list of the record bytes of every leaf (b'' for kept leaves)."""
    off = np.concatenate([[0], np.cumsum(record_size(code))])
    assert off[-1] == len(payload)
    return [bytes(payload[off[i]:off[i + 1]]) for i in range(len(code))]


def unpack_leaf(rec, code):
    """q int32 [512,3] of a quantised record."""
    q = np.zeros((512, 3), np.int32)
    at = 0
    for ch, b in enumerate(widths(int(code))):
        q[:, ch] = trr.unpack_leaf(rec[at:at + 64 * int(b)], int(b)) if b else 0
        at += 64 * int(b)
    assert at == len(rec)
    return q


def apply(recon, tol, code, payload):
    """-> x~ float32 [n,512,3]: decoded leaves with their records applied."""
    out = np.array(recon, dtype=F).reshape(-1, 512, 3).copy()
    step = step_of(tol)
    for i, (c, rec) in enumerate(zip(code, records(code, payload))):
        c = int(c)
        if c == KEPT:
            continue
        if c == RAW:
            out[i] = np.frombuffer(rec, dtype="<f4").reshape(512, 3)
        else:
            with np.errstate(all="ignore"):
                out[i] = out[i] + unpack_leaf(rec, c).astype(F) * step
    return out


def leaf_with_max_q(qmax3, tol=0.5, rng=None, negative=(False, False, False)):
    """(x, recon) of one leaf [512,3]: channel c is torch_ref_residual.leaf_with_max_q(qmax3[c]) (its q of largest magnitude
    +-qmax3[c] at voxel 7, the others 0 or, with rng, in -1 .. 1; recon = 0, x = q * step)."""
    cols = [trr.leaf_with_max_q(int(qm), tol, rng, negative=bool(ng)) for qm, ng in zip(qmax3, negative)]
    return np.stack([c[0] for c in cols], axis=1), np.zeros((512, 3), F)


def qmax_of_width(b):
    """a q whose zz has exactly b bits: 0, -1 (zz 1), then 2^(b-2) (zz 2^(b-1))."""
    return 0 if b == 0 else -1 if b == 1 else 1 << (b - 2)


def format_leaves(tol=0.5):
    """51 leaves: every width 0 .. 16 in every channel, the other two channels at other widths ((b + 5) % 17, (b + 11) % 17);
    x^ = 0, x = q * step (with tol 0.5 the step is 0.9375 and every product is exact).  -> (x, recon, err, widths [51,3]); the
    reported error is 9 tol, so every leaf is selected by it alone (an all-zero channel changes nothing)."""
    xs, ws = [], []
    for b in range(17):
        for ch in range(3):
            w = [0, 0, 0]
            w[ch], w[(ch + 1) % 3], w[(ch + 2) % 3] = b, (b + 5) % 17, (b + 11) % 17
            q = [qmax_of_width(v) for v in w]
            x, _ = leaf_with_max_q([abs(v) for v in q], tol, np.random.default_rng(3 * b + ch), negative=[v < 0 for v in q])
            xs.append(x)
            ws.append(w)
    x = np.stack(xs)
    return x, np.zeros_like(x), np.full((len(x), 2), 9.0 * tol, F), np.array(ws)
