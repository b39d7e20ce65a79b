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


# ---- `.vqv3` v1: the Vec3 codec's container (include/vqvdb_hip_vec3_file.h) ----
#     file : "VQVEC3" | u8 version=1 | u8 numGrids (1..255) | u32 numCodes | u8 kind | u8 mode | u16 zero | f32 tol | u32 zero
#     grid : u32 nameLength | name | f32 transform[16] | u16 latentShape[3]={4,4,4} | u32 totalBlocks (n) | u8 hasBackground | u8 zero[3]
#            f32 background[3] | u64 payloadBytes | i32 origins[n][3] | u16 indices[n][64]
#            kind 1 only: u64 masks[n][8] | u16 codes[n] | u8 payload[payloadBytes]
# kind 0: indices only (mode 0, tol +0.0, payloadBytes 0).  kind 1: masks and the compact records of include/vqvdb_hip_vec3_active.h;
# mode is the decoder mode the records belong to (0 fp32, 1 bf16).  A leaf's record starts at the exclusive sum of the sizes before it.
VEC3_MAGIC = b"VQVEC3"
VEC3_VERSION = 1
VEC3_HEADER_BYTES = 24
VEC3_KIND_INDICES, VEC3_KIND_ACTIVE = 0, 1
VEC3_CODE_KEPT, VEC3_CODE_RAW = 0xFFFE, 0xFFFF


def vec3_record_bytes(codes, active) -> np.ndarray:
    """int64 [n]: the bytes of every leaf's compact record from its code and its count of active voxels: 0 kept, 8 ceil(3 A / 2) raw,
    8 ceil(A / 64) (b0 + b1 + b2) quantised.  A code that is neither a sentinel nor three widths of 0..16 raises."""
    c = np.asarray(codes).astype(np.int64).reshape(-1)
    a = np.asarray(active).astype(np.int64).reshape(-1)
    if len(c) != len(a):
        raise ValueError(f"{len(c)} codes but {len(a)} active counts")
    if len(a) and (a.min() < 0 or a.max() > 512):
        raise ValueError("an active count is outside 0..512")
    kept, raw = c == VEC3_CODE_KEPT, c == VEC3_CODE_RAW
    b = [(c >> s) & 31 for s in (0, 5, 10)]
    bad = ~(kept | raw) & ((c < 0) | ((c >> 15) != 0) | (b[0] > 16) | (b[1] > 16) | (b[2] > 16))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f".vqv3: code 0x{int(c[i]) & 0xFFFF:04X} of leaf {i} is neither 0xFFFE, 0xFFFF nor three widths of 0..16")
    return np.where(kept, 0, np.where(raw, 8 * ((3 * a + 1) // 2), 8 * ((a + 63) // 64) * (b[0] + b[1] + b[2])))


def _vec3_popcounts(masks) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(len(masks), 64), axis=1).sum(axis=1, dtype=np.int64)


def dumps_vec3(header: dict, grids) -> bytes:
    """header: {"num_codes", "kind", and for kind 1 "mode" (0 / 1) and "tol"}.  grids: dicts with "name", "origins" int32 [n,3],
    "indices" uint16 [n,64], optional "transform" (16 floats, default identity) and "background" (three floats or None), and for
    kind 1 "masks" uint64 [n,8], "codes" uint16 [n] and "payload" (bytes or uint8 array)."""
    kind, num_codes = int(header["kind"]), int(header["num_codes"])
    if kind not in (VEC3_KIND_INDICES, VEC3_KIND_ACTIVE):
        raise ValueError(f".vqv3: kind {kind} is neither 0 nor 1")
    mode = int(header.get("mode", 0)) if kind else 0
    if mode not in (0, 1):
        raise ValueError(f".vqv3: mode {mode} is neither 0 (fp32) nor 1 (bf16)")
    if not 1 <= num_codes <= 65536:
        raise ValueError(f".vqv3: numCodes {num_codes} is not in 1..65536")
    if not 1 <= len(grids) <= 255:
        raise ValueError("a .vqv3 file holds 1..255 grids")
    with np.errstate(over="ignore"):
        tol = np.float32(header.get("tol", 0.0)) if kind else np.float32(0.0)
    out = [VEC3_MAGIC + struct.pack("<BBIBBH", VEC3_VERSION, len(grids), num_codes, kind, mode, 0) + np.array([tol], "<f4").tobytes() + struct.pack("<I", 0)]
    for g in grids:
        origins = np.ascontiguousarray(g["origins"], dtype="<i4").reshape(-1, 3)
        n = len(origins)
        if n >= 1 << 32:
            raise ValueError("more than 2^32-1 leaves in one grid")
        indices = np.ascontiguousarray(g["indices"], dtype="<u2").reshape(n, 64)
        name = g["name"].encode() if isinstance(g["name"], str) else bytes(g["name"])
        transform = IDENTITY if g.get("transform") is None else np.asarray(g["transform"], dtype="<f4").reshape(16)
        bg = g.get("background")
        bg_bytes = b"\0" * 12 if bg is None else np.ascontiguousarray(bg, dtype="<f4").reshape(3).tobytes()
        payload = b""
        if kind:
            masks = np.ascontiguousarray(g["masks"], dtype="<u8").reshape(n, 8)
            codes = np.ascontiguousarray(g["codes"], dtype="<u2").reshape(n)
            payload = np.ascontiguousarray(g["payload"], dtype=np.uint8).tobytes() if isinstance(g["payload"], np.ndarray) else bytes(g["payload"])
            need = int(vec3_record_bytes(codes, _vec3_popcounts(masks)).sum())
            if need != len(payload):
                raise ValueError(f".vqv3: grid '{name.decode(errors='replace')}': the codes and masks need {need} payload bytes, got {len(payload)}")
        out.append(struct.pack("<I", len(name)) + name + transform.tobytes() + struct.pack("<3HIB3x", 4, 4, 4, n, 0 if bg is None else 1) + bg_bytes +
                   struct.pack("<Q", len(payload)))
        out += [origins.tobytes(), indices.tobytes()]
        if kind:
            out += [masks.tobytes(), codes.tobytes(), payload]
    return b"".join(out)


def loads_vec3(buf):
    """-> (header dict, [grid dict]) with the keys of dumps_vec3 ("background" None where absent; kind 0: "masks", "codes" and
    "payload" None).  Refuses whatever the C reader refuses: wrong magic, version, kind, mode, reserved fields, a length that is not
    what the headers imply, an index >= numCodes, an illegal code, record sizes that do not sum to payloadBytes."""
    buf = bytes(buf)
    if len(buf) < VEC3_HEADER_BYTES:
        raise ValueError("Failed to read file header.")
    if buf[:6] != VEC3_MAGIC:
        raise ValueError("Invalid file magic; not a .vqv3 file.")
    version, n_grids, num_codes, kind, mode, zero16 = struct.unpack_from("<BBIBBH", buf, 6)
    tol_bits, zero32 = struct.unpack_from("<II", buf, 16)
    if version != VEC3_VERSION:
        raise ValueError(f"Unsupported .vqv3 version {version} (expected 1).")
    if n_grids < 1:
        raise ValueError(".vqv3: a file holds 1..255 grids, the header says 0")
    if not 1 <= num_codes <= 65536:
        raise ValueError(f".vqv3: numCodes {num_codes} is not in 1..65536")
    if kind not in (VEC3_KIND_INDICES, VEC3_KIND_ACTIVE):
        raise ValueError(f".vqv3: kind {kind} is neither 0 nor 1")
    if mode > 1:
        raise ValueError(f".vqv3: mode {mode} is neither 0 (fp32) nor 1 (bf16)")
    if zero16 or zero32:
        raise ValueError(".vqv3: a reserved field of the file header is not zero")
    if kind == VEC3_KIND_INDICES and (mode or tol_bits):
        raise ValueError(".vqv3: a file of kind 0 carries mode 0 and tol +0.0")
    header = {"num_codes": num_codes, "kind": kind, "mode": mode, "tol": float(np.frombuffer(buf, "<f4", 1, 16)[0])}
    off, grids = VEC3_HEADER_BYTES, []
    trunc = ".vqv3: file truncated inside the metadata of a grid"
    for _ in range(n_grids):
        if off + 4 > len(buf):
            raise ValueError(trunc)
        (name_len,) = struct.unpack_from("<I", buf, off); off += 4
        if off + name_len + 98 > len(buf):
            raise ValueError(trunc)
        name = buf[off:off + name_len].decode(); off += name_len
        transform = np.frombuffer(buf, "<f4", 16, off).copy(); off += 64
        s0, s1, s2, n, has_bg, z0, z1, z2 = struct.unpack_from("<3HI4B", buf, off); off += 14
        bg_raw = buf[off:off + 12]; off += 12
        (payload_bytes,) = struct.unpack_from("<Q", buf, off); off += 8
        who = f".vqv3: grid '{name}' "
        if (s0, s1, s2) != (4, 4, 4):
            raise ValueError(who + f"has latent shape [{s0},{s1},{s2}], not [4,4,4]")
        if has_bg > 1 or z0 or z1 or z2:
            raise ValueError(who + "has a hasBackground byte above 1 or a reserved byte that is not zero")
        if not has_bg and bg_raw != b"\0" * 12:
            raise ValueError(who + "has no background but background values that are not +0.0")
        if kind == VEC3_KIND_INDICES and payload_bytes:
            raise ValueError(who + f"belongs to a file of kind 0 but has payloadBytes {payload_bytes}")
        fixed = n * (12 + 128 + (64 + 2 if kind else 0))
        if off + fixed + payload_bytes > len(buf):
            raise ValueError(who + f"needs more bytes than the file holds ({n} leaves, {payload_bytes} payload bytes)")
        g = {"name": name, "transform": transform, "background": np.frombuffer(bg_raw, "<f4").copy() if has_bg else None,
             "masks": None, "codes": None, "payload": None}
        g["origins"] = np.frombuffer(buf, "<i4", n * 3, off).reshape(n, 3).copy(); off += 12 * n
        g["indices"] = np.frombuffer(buf, "<u2", n * 64, off).reshape(n, 64).copy(); off += 128 * n
        if n and int(g["indices"].max()) >= num_codes:
            raise ValueError(who + f"holds index {int(g['indices'].max())}, out of range (num_codes {num_codes})")
        if kind:
            g["masks"] = np.frombuffer(buf, "<u8", n * 8, off).reshape(n, 8).copy(); off += 64 * n
            g["codes"] = np.frombuffer(buf, "<u2", n, off).copy(); off += 2 * n
            need = int(vec3_record_bytes(g["codes"], _vec3_popcounts(g["masks"])).sum())
            if need != payload_bytes:
                raise ValueError(who + f": the codes and masks need {need} payload bytes, the grid's header says {payload_bytes}")
            g["payload"] = np.frombuffer(buf, np.uint8, payload_bytes, off).copy(); off += payload_bytes
        grids.append(g)
    if off != len(buf):
        raise ValueError(f".vqv3: the headers imply {off} bytes, the file holds {len(buf)}")
    return header, grids


def vec3_file_bytes(grids, kind: int, payload_bytes=None) -> int:
    """len(dumps_vec3(...)) without the data: 24 + sum_g (102 + nameLength_g + n_g (12 + 128 + (64 + 2 if kind 1))) + sum_g
    payload_bytes[g].  grids: dicts with "name" and "origins" [n,3] (or "n_leaves"); payload_bytes: one integer per grid for kind 1,
    None (or zeros) for kind 0.  Restates vqhip_vec3_budget_file_bytes of include/vqvdb_hip_vec3_budget.h."""
    if kind not in (VEC3_KIND_INDICES, VEC3_KIND_ACTIVE):
        raise ValueError(f".vqv3: kind {kind} is neither 0 nor 1")
    if not 1 <= len(grids) <= 255:
        raise ValueError("a .vqv3 file holds 1..255 grids")
    if payload_bytes is None:
        if kind:
            raise ValueError(".vqv3: a file of kind 1 needs every grid's payload bytes")
        payload_bytes = [0] * len(grids)
    if len(payload_bytes) != len(grids):
        raise ValueError(f"{len(grids)} grids but {len(payload_bytes)} payload sizes")
    total = VEC3_HEADER_BYTES
    for g, payload in zip(grids, payload_bytes):
        n = int(g["n_leaves"]) if "n_leaves" in g else len(np.asarray(g["origins"]).reshape(-1, 3))
        name = g["name"].encode() if isinstance(g["name"], str) else bytes(g["name"])
        if not 0 <= n < 1 << 32:
            raise ValueError("more than 2^32-1 leaves in one grid")
        if int(payload) < 0 or (not kind and int(payload)):
            raise ValueError(".vqv3: a payload size is negative, or not zero in a file of kind 0")
        total += 102 + len(name) + n * (12 + 128 + (64 + 2 if kind else 0)) + int(payload)
    if total >= 1 << 63:
        raise ValueError(".vqv3: the file's size passes 2^63 - 1")
    return total


def write_vec3(path_or_buf, header: dict, grids) -> None:
    """dumps_vec3 into a path or into an object with write()."""
    data = dumps_vec3(header, grids)
    if hasattr(path_or_buf, "write"):
        path_or_buf.write(data)
        return
    with open(path_or_buf, "wb") as f:
        f.write(data)


def read_vec3(path_or_buf):
    """loads_vec3 of a path, of bytes or of an object with read()."""
    if isinstance(path_or_buf, (bytes, bytearray, memoryview)):
        return loads_vec3(path_or_buf)
    if hasattr(path_or_buf, "read"):
        return loads_vec3(path_or_buf.read())
    with open(path_or_buf, "rb") as f:
        return loads_vec3(f.read())
