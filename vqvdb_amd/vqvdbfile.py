"""`.vqvdb` v3 container in numpy (byte layout: SURVEY.md App. B; reference writer/reader
src/Utils/VQVDB_Reader.cpp:81-150,168-300).  Host-side framing only — no codec work happens here.  The `.vqres` sidecar of
an error-bounded compress is framed at the end of this file.

    file : "VQVDB" | u8 version=3 | u8 numGrids | u32 numEmbeddings | u8 latentDimCount
    grid : u32 nameLength | name | f32 transform[16] | u16 latentShape[latentDimCount] | u32 totalBlocks
           totalBlocks x { i32 origin[3] | u8 indices[prod(latentShape)] }        (76 B per leaf)
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import List

import numpy as np

MAGIC = b"VQVDB"
VERSION = 3
RECORD = np.dtype([("origin", "<i4", (3,)), ("indices", "u1", (64,))])
assert RECORD.itemsize == 76

IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


@dataclass
class Grid:
    name: str
    origins: np.ndarray                      # int32 [n,3]
    indices: np.ndarray                      # uint8 [n,64]
    transform: np.ndarray = field(default_factory=lambda: IDENTITY.copy())
    latent_shape: tuple = (4, 4, 4)


def dumps(grids: List[Grid], num_embeddings: int = 256) -> bytes:
    if not 1 <= len(grids) <= 255:
        raise ValueError("a .vqvdb file holds 1..255 grids")
    out = [MAGIC + struct.pack("<BBIB", VERSION, len(grids), num_embeddings, 3)]
    for g in grids:
        n = len(g.origins)
        if n >= 1 << 32:
            raise ValueError("more than 2^32-1 leaves in one grid")
        name = g.name.encode()
        out.append(struct.pack("<I", len(name)) + name)
        out.append(np.asarray(g.transform, dtype="<f4").reshape(16).tobytes())
        out.append(struct.pack("<3H", *g.latent_shape) + struct.pack("<I", n))
        rec = np.empty(n, dtype=RECORD)
        rec["origin"] = np.asarray(g.origins, dtype=np.int32).reshape(n, 3)
        rec["indices"] = np.asarray(g.indices, dtype=np.uint8).reshape(n, 64)
        out.append(rec.tobytes())
    return b"".join(out)


def loads(buf: bytes) -> List[Grid]:
    if len(buf) < 12:
        raise ValueError("Failed to read file header.")
    if buf[:5] != MAGIC:
        raise ValueError("Invalid file magic; not a .vqvdb file.")
    version, n_grids, _num_emb, dim_count = struct.unpack_from("<BBIB", buf, 5)
    if version != VERSION:
        raise ValueError(f"Unsupported .vqvdb version {version} (expected 3).")
    off, grids = 12, []
    for _ in range(n_grids):
        (name_len,) = struct.unpack_from("<I", buf, off); off += 4
        name = buf[off:off + name_len].decode(); off += name_len
        transform = np.frombuffer(buf, dtype="<f4", count=16, offset=off).copy(); off += 64
        shape = struct.unpack_from(f"<{dim_count}H", buf, off); off += 2 * dim_count
        (total,) = struct.unpack_from("<I", buf, off); off += 4
        block = int(np.prod(shape))
        if block != 64:
            raise ValueError(f"grid '{name}' has latent shape {list(shape)}; only [4,4,4] is supported")
        if off + total * 76 > len(buf):
            raise ValueError("File truncated: incomplete block data.")
        rec = np.frombuffer(buf, dtype=RECORD, count=total, offset=off); off += total * 76
        grids.append(Grid(name, rec["origin"].copy(), rec["indices"].copy(), transform, tuple(shape)))
    return grids


def save(path, grids: List[Grid], num_embeddings: int = 256) -> None:
    with open(path, "wb") as f:
        f.write(dumps(grids, num_embeddings))


def load(path) -> List[Grid]:
    with open(path, "rb") as f:
        return loads(f.read())


# ---- `.vqres` v1: the raw leaves of an error-bounded compress, beside a .vqvdb (include/vqvdb_hip_bounded.h) ----
#     file : "VQRES" | u8 version=1 | u8 numGrids | f32 tol
#     grid : u32 nOutliers | nOutliers x { u32 record_index | f32 leaf[512] }      (grids in the .vqvdb's order)
# record_index: the leaf's position among that grid's records, ascending.
RES_MAGIC = b"VQRES"
RES_VERSION = 1
RES_ENTRY = np.dtype([("record_index", "<u4"), ("leaf", "<f4", (512,))])
assert RES_ENTRY.itemsize == 2052


def dumps_residual(tol: float, grids) -> bytes:
    """grids: one (record_index [m], leaves float32 [m,512]) pair per grid of the .vqvdb, in its order."""
    if not 1 <= len(grids) <= 255:
        raise ValueError("a .vqres file holds 1..255 grids")
    out = [RES_MAGIC + struct.pack("<BB", RES_VERSION, len(grids)) + np.float32(tol).astype("<f4").tobytes()]
    for ids, leaves in grids:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        leaves = np.asarray(leaves, dtype=np.float32).reshape(-1, 512)
        if len(ids) != len(leaves):
            raise ValueError(f"{len(ids)} record indices but {len(leaves)} leaves")
        if len(ids) and (ids.min() < 0 or ids.max() >= 1 << 32 or (np.diff(ids) <= 0).any()):
            raise ValueError("record indices must be ascending, unique and below 2^32")
        ent = np.empty(len(ids), dtype=RES_ENTRY)
        ent["record_index"] = ids
        ent["leaf"] = leaves
        out.append(struct.pack("<I", len(ids)) + ent.tobytes())
    return b"".join(out)


def loads_residual(buf: bytes):
    """-> (tol, [(record_index int64 [m], leaves float32 [m,512]) per grid])."""
    if len(buf) < 11:
        raise ValueError("Failed to read residual file header.")
    if buf[:5] != RES_MAGIC:
        raise ValueError("Invalid residual file magic; not a .vqres file.")
    version, n_grids = struct.unpack_from("<BB", buf, 5)
    if version != RES_VERSION:
        raise ValueError(f"Unsupported .vqres version {version} (expected {RES_VERSION}).")
    tol = float(np.frombuffer(buf, dtype="<f4", count=1, offset=7)[0])
    off, grids = 11, []
    for _ in range(n_grids):
        if off + 4 > len(buf):
            raise ValueError("Residual file truncated: no outlier count.")
        (m,) = struct.unpack_from("<I", buf, off); off += 4
        if off + m * RES_ENTRY.itemsize > len(buf):
            raise ValueError("Residual file truncated: incomplete leaf entry.")
        ent = np.frombuffer(buf, dtype=RES_ENTRY, count=m, offset=off); off += m * RES_ENTRY.itemsize
        ids = ent["record_index"].astype(np.int64)
        if (np.diff(ids) <= 0).any():
            raise ValueError("residual file: record indices are not ascending")
        grids.append((ids, ent["leaf"].copy()))
    if off != len(buf):
        raise ValueError("Residual file holds bytes past its last grid.")
    return tol, grids


def save_residual(path, tol: float, grids) -> None:
    with open(path, "wb") as f:
        f.write(dumps_residual(tol, grids))


def load_residual(path):
    with open(path, "rb") as f:
        return loads_residual(f.read())


# ---- `.vqres` v2: quantised or raw records of the leaves over the tolerance (include/vqvdb_hip_residual.h) ----
#     file : "VQRES" | u8 version=2 | u8 numGrids | f32 tol
#     grid : u32 nRecords | nRecords x { u32 record_index | u8 class | u8 bytes[class==255 ? 2048 : 64*class] }
# record_index ascending within the grid; class 0 .. 16 (bit planes) or 255 (the leaf's 2048 bytes).
RES_VERSION_2 = 2
RES_CLASS_RAW = 255
RES_CLASS_MAX_BITS = 16


def residual_record_bytes(cls: int) -> int:
    if cls == RES_CLASS_RAW:
        return 2048
    if 0 <= cls <= RES_CLASS_MAX_BITS:
        return 64 * cls
    raise ValueError(f"residual file: class {cls} is not 0..16 or 255")


def dumps_residual_v2(tol: float, grids) -> bytes:
    """grids: one (record_index [m], class [m], list of m record bytes) triple per grid of the .vqvdb, in its order."""
    if not 1 <= len(grids) <= 255:
        raise ValueError("a .vqres file holds 1..255 grids")
    out = [RES_MAGIC + struct.pack("<BB", RES_VERSION_2, len(grids)) + np.float32(tol).astype("<f4").tobytes()]
    for ids, classes, recs in grids:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        classes = np.asarray(classes, dtype=np.int64).reshape(-1)
        if not len(ids) == len(classes) == len(recs):
            raise ValueError(f"{len(ids)} record indices, {len(classes)} classes and {len(recs)} records")
        if len(ids) and (ids.min() < 0 or ids.max() >= 1 << 32 or (np.diff(ids) <= 0).any()):
            raise ValueError("record indices must be ascending, unique and below 2^32")
        out.append(struct.pack("<I", len(ids)))
        for ri, cls, rec in zip(ids, classes, recs):
            if len(rec) != residual_record_bytes(int(cls)):
                raise ValueError(f"a record of class {int(cls)} holds {residual_record_bytes(int(cls))} bytes, not {len(rec)}")
            out.append(struct.pack("<IB", int(ri), int(cls)) + bytes(rec))
    return b"".join(out)


def loads_residual_v2(buf: bytes):
    """-> (tol, [(record_index int64 [m], class uint8 [m], list of m record bytes) per grid])."""
    if len(buf) < 11:
        raise ValueError("Failed to read residual file header.")
    if buf[:5] != RES_MAGIC:
        raise ValueError("Invalid residual file magic; not a .vqres file.")
    version, n_grids = struct.unpack_from("<BB", buf, 5)
    if version != RES_VERSION_2:
        raise ValueError(f"Unsupported .vqres version {version} (expected {RES_VERSION_2}).")
    tol = float(np.frombuffer(buf, dtype="<f4", count=1, offset=7)[0])
    off, grids = 11, []
    for _ in range(n_grids):
        if off + 4 > len(buf):
            raise ValueError("Residual file truncated: no record count.")
        (m,) = struct.unpack_from("<I", buf, off); off += 4
        if off + 5 * m > len(buf):
            raise ValueError("Residual file truncated: incomplete leaf entry.")
        ids, classes, recs = np.empty(m, np.int64), np.empty(m, np.uint8), []
        for i in range(m):
            if off + 5 > len(buf):
                raise ValueError("Residual file truncated: incomplete leaf entry.")
            ri, cls = struct.unpack_from("<IB", buf, off); off += 5
            if i and ri <= ids[i - 1]:
                raise ValueError("residual file: record indices are not ascending")
            size = residual_record_bytes(cls)
            if off + size > len(buf):
                raise ValueError("Residual file truncated: incomplete leaf entry.")
            ids[i], classes[i] = ri, cls
            recs.append(bytes(buf[off:off + size])); off += size
        grids.append((ids, classes, recs))
    if off != len(buf):
        raise ValueError("Residual file holds bytes past its last grid.")
    return tol, grids


def save_residual_v2(path, tol: float, grids) -> None:
    with open(path, "wb") as f:
        f.write(dumps_residual_v2(tol, grids))


def load_residual_v2(path):
    with open(path, "rb") as f:
        return loads_residual_v2(f.read())
