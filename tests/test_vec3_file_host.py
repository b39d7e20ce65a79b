"""The .vqv3 container without a GPU: write_vec3 / read_vec3 of vqvdb_amd/vqvdbfile.py round trip both kinds, match a
file assembled here with struct.pack byte for byte, and refuse what the format forbids; record sizes equal tests/torch_ref_active.py
on the count edges; names, arity and constants of include/vqvdb_hip_vec3_file.h, in the header text and in the library."""
import ctypes
import io
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_active as tra  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from vqvdb_amd import codec, vqvdbfile as vf  # noqa: E402

F = np.float32
NAMES = ["vqhip_vec3_encode_leaves", "vqhip_vec3_decode_leaves", "vqhip_vec3_file_compress", "vqhip_vec3_file_compress_active",
         "vqhip_vec3_file_decompress", "vqhip_vec3_file_info"]
ARITY = dict(zip(NAMES, (4, 4, 6, 8, 7, 8)))
BACKGROUND = np.array([-0.0, np.nan, 1e30], F)
EDGES = (0, 1, 63, 64, 65, 511, 512)
CODES = [t3r.KEPT, t3r.RAW, 0, t3r.make_code(1, 0, 0), t3r.make_code(0, 7, 0), t3r.make_code(3, 0, 16), t3r.make_code(16, 16, 16)]


def masks_with_counts(counts, seed=5):
    rng = np.random.default_rng(seed)
    active = np.zeros((len(counts), 512), bool)
    for i, a in enumerate(counts):
        active[i, rng.permutation(512)[:a]] = True
    return codec.pack_masks(active)


def make_grid(name, n, kind, seed, background=None, num_codes=4096):
    rng = np.random.default_rng(seed)
    g = {"name": name, "origins": rng.integers(-4096, 4096, (n, 3)).astype(np.int32) * 8, "indices": rng.integers(0, num_codes, (n, 64)).astype(np.uint16),
         "transform": rng.standard_normal(16).astype(F), "background": background}
    if kind:
        counts = [EDGES[i % len(EDGES)] for i in range(n)]
        g["masks"] = masks_with_counts(counts, seed)
        g["codes"] = np.array([CODES[(i // len(EDGES) + i) % len(CODES)] for i in range(n)], np.uint16)
        g["payload"] = rng.integers(0, 256, int(tra.record_size(g["codes"], np.array(counts)).sum())).astype(np.uint8)
    return g


def same_grid(a, b, kind):
    assert a["name"] == b["name"] and np.array_equal(a["origins"], b["origins"]) and np.array_equal(a["indices"], b["indices"])
    assert np.asarray(a["transform"], F).tobytes() == b["transform"].tobytes()
    assert (a.get("background") is None) == (b["background"] is None)
    if a.get("background") is not None:
        assert np.asarray(a["background"], F).tobytes() == b["background"].tobytes()      # -0.0, NaN and 1e30 to the bit
    if kind:
        assert np.array_equal(a["masks"], b["masks"]) and np.array_equal(a["codes"], b["codes"]) and bytes(a["payload"]) == bytes(b["payload"])
    else:
        assert b["masks"] is None and b["codes"] is None and b["payload"] is None


@pytest.mark.parametrize("kind", (0, 1))
def test_round_trip_of_two_grids_and_an_empty_one(kind, tmp_path):
    header = {"num_codes": 4096, "kind": kind, "mode": kind, "tol": 0.0625 if kind else 0.0}
    grids = [make_grid("", 23, kind, 1, BACKGROUND), make_grid("empty", 0, kind, 2), make_grid("n" * 300, 9, kind, 3)]
    data = vf.dumps_vec3(header, grids)
    per_leaf = 12 + 128 + (64 + 2 if kind else 0)
    assert len(data) == 24 + sum(102 + len(g["name"]) + per_leaf * len(g["origins"]) + (len(g["payload"]) if kind else 0) for g in grids)
    path = tmp_path / "t.vqv3"
    vf.write_vec3(path, header, grids)
    buf = io.BytesIO()
    vf.write_vec3(buf, header, grids)
    assert path.read_bytes() == data == buf.getvalue()
    for source in (path, data, io.BytesIO(data)):
        h, got = vf.read_vec3(source)
        assert h == header and len(got) == 3
        for a, b in zip(grids, got):
            same_grid(a, b, kind)
        assert vf.dumps_vec3(h, got) == data
    with np.errstate(over="ignore"):
        for tol in (float("nan"), float("inf"), -1.0, 1e300) if kind else ():
            h, _ = vf.read_vec3(vf.dumps_vec3(dict(header, tol=tol), grids))
            assert F(h["tol"]).tobytes() == F(tol).tobytes()


def hand_assembled():
    """a kind-1 file of one grid with two leaves and a background, and of one grid without either, field by field"""
    m0 = [0x8000000000000001, 0, 0, 0, 0, 0, 0, 1 << 63]        # 3 active voxels: 0, 63, 511
    m1 = [0xFFFFFFFFFFFFFFFF] * 8                               # 512
    code0, code1 = 0xFFFF, 2 | 0 << 5 | 1 << 10                 # raw: 8 ceil(9 / 2) = 40 B; quantised, 3 planes of 8 words: 192 B
    payload = bytes(range(40)) + bytes(255 - (i % 200) for i in range(192))
    b = b"VQVEC3" + struct.pack("<BBIBBHfI", 1, 2, 4096, 1, 1, 0, 0.25, 0)
    assert len(b) == 24
    b += struct.pack("<I", 3) + b"vel" + struct.pack("<16f", *range(16)) + struct.pack("<3H", 4, 4, 4) + struct.pack("<IB3x", 2, 1)
    b += struct.pack("<I", 0x80000000) + struct.pack("<I", 0x7FC00000) + struct.pack("<f", 1e30) + struct.pack("<Q", 232)
    b += struct.pack("<6i", -8, 0, 8, 16, -24, 2147483640) + struct.pack("<64H", *range(64)) + struct.pack("<64H", *([4095] * 64))
    b += struct.pack("<8Q", *m0) + struct.pack("<8Q", *m1) + struct.pack("<2H", code0, code1) + payload
    b += struct.pack("<I", 0) + struct.pack("<16f", 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1) + struct.pack("<3H", 4, 4, 4) + struct.pack("<IB3x", 0, 0)
    b += bytes(12) + struct.pack("<Q", 0)
    header = {"num_codes": 4096, "kind": 1, "mode": 1, "tol": 0.25}
    grids = [{"name": "vel", "transform": np.arange(16, dtype=F), "origins": np.array([[-8, 0, 8], [16, -24, 2147483640]], np.int32),
              "indices": np.stack([np.arange(64), np.full(64, 4095)]).astype(np.uint16), "background": np.array([0x80000000, 0x7FC00000, 0x7149F2CA], np.uint32).view(F),
              "masks": np.array([m0, m1], np.uint64), "codes": np.array([code0, code1], np.uint16), "payload": np.frombuffer(payload, np.uint8)},
             {"name": "", "origins": np.zeros((0, 3), np.int32), "indices": np.zeros((0, 64), np.uint16), "masks": np.zeros((0, 8), np.uint64),
              "codes": np.zeros(0, np.uint16), "payload": b""}]
    assert struct.pack("<f", 1e30) == struct.pack("<I", 0x7149F2CA)
    return b, header, grids


def test_a_hand_assembled_file_pins_the_layout():
    want, header, grids = hand_assembled()
    assert len(want) == 24 + (102 + 3) + 2 * (12 + 128 + 64 + 2) + 232 + 102
    assert vf.dumps_vec3(header, grids) == want
    h, got = vf.read_vec3(want)
    assert h == header
    for a, b in zip(grids, got):
        same_grid(dict(a, transform=a.get("transform", vf.IDENTITY)), b, 1)
    # kind 0: the same grid without masks, codes and payload; mode and tol are zero whatever the header dict says
    k0 = vf.dumps_vec3({"num_codes": 4096, "kind": 0, "mode": 1, "tol": 0.25}, grids[:1])
    assert k0[:24] == b"VQVEC3" + struct.pack("<BBIBBHfI", 1, 1, 4096, 0, 0, 0, 0.0, 0)
    assert k0[24:24 + 105 - 8] == want[24:24 + 105 - 8] and k0[24 + 97:24 + 105] == bytes(8) and k0[24 + 105:] == want[24 + 105:24 + 105 + 2 * 140]


def test_read_vec3_refuses_what_the_format_forbids():
    good, _, _ = hand_assembled()
    vf.read_vec3(good)

    def patched(at, fmt, *v):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)

    payload_field = 24 + 105 - 8
    codes_at = 24 + 105 + 2 * (12 + 128 + 64)
    cases = {
        "magic": (patched(0, "<c", b"X"), "magic"), "version": (patched(6, "<B", 2), "version"), "kind 2": (patched(12, "<B", 2), "kind"),
        "mode 2": (patched(13, "<B", 2), "mode"), "reserved u16": (patched(14, "<H", 256), "reserved"), "reserved u32": (patched(20, "<I", 1), "reserved"),
        "grid reserved": (patched(24 + 7 + 64 + 6 + 4 + 2, "<B", 1), "reserved"), "hasBackground 2": (patched(24 + 7 + 64 + 6 + 4, "<B", 2), "hasBackground"),
        "latent shape": (patched(24 + 7 + 64, "<H", 8), "latent shape"), "no grids": (patched(7, "<B", 0), "grids"),
        "one byte short": (good[:-1], "truncated|bytes"), "one byte long": (good + b"\0", "imply"),
        "payloadBytes + 8": (patched(payload_field, "<Q", 240), "bytes"), "payloadBytes - 8": (patched(payload_field, "<Q", 224), "bytes|truncated"),
        "payloadBytes + 8, file grown": (patched(payload_field, "<Q", 240)[:-102] + bytes(8) + good[-102:], "payload bytes"),
        "illegal code": (patched(codes_at + 2, "<H", 17), "0x0011"), "code above the widths": (patched(codes_at + 2, "<H", 0x8000), "0x8000"),
        "index >= numCodes": (patched(8, "<I", 4095), "out of range"), "mask bit": (patched(24 + 105 + 2 * 140, "<B", 3), "payload bytes"),
        "total 2^32 - 1": (patched(24 + 7 + 64 + 6, "<I", 0xFFFFFFFF), "more bytes"), "name length": (patched(24, "<I", 0xFFFFFFFF), "truncated"),
        "empty": (b"", "header"), "header only": (good[:24], "truncated"),
    }
    for name, (data, message) in cases.items():
        with pytest.raises(ValueError, match=message):
            vf.read_vec3(data)
        assert data != good, name
    for cut in (24, 28, 24 + 105 - 8, 24 + 105, 24 + 105 + 24, 24 + 105 + 24 + 256, codes_at, codes_at + 4, len(good) - 102, len(good) - 1):
        with pytest.raises(ValueError):
            vf.read_vec3(good[:cut])
    k0 = vf.dumps_vec3({"num_codes": 16, "kind": 0}, [make_grid("g", 3, 0, 4, num_codes=16)])
    vf.read_vec3(k0)
    for at, fmt, v in ((13, "<B", 1), (16, "<f", 0.5), (16, "<I", 0x80000000), (24 + 5 + 64 + 6 + 4 + 4 + 12, "<Q", 8)):
        b = bytearray(k0)
        struct.pack_into(fmt, b, at, v)
        with pytest.raises(ValueError):
            vf.read_vec3(bytes(b))
    # the writer refuses what the reader would
    _, header, grids = hand_assembled()
    for bad_header in (dict(header, kind=2), dict(header, mode=2), dict(header, num_codes=0)):
        with pytest.raises(ValueError):
            vf.dumps_vec3(bad_header, grids)
    with pytest.raises(ValueError, match="payload bytes"):
        vf.dumps_vec3(header, [dict(grids[0], payload=bytes(224))])
    with pytest.raises(ValueError, match="0x0011"):
        vf.dumps_vec3(header, [dict(grids[0], codes=np.array([0xFFFF, 17], np.uint16))])
    with pytest.raises(ValueError, match="1..255"):
        vf.dumps_vec3(header, [])


def test_record_sizes_equal_the_restatement_on_the_count_edges():
    lib = codec.load_library() if os.path.exists(codec.LIB_PATH) else None
    for code in CODES:
        want = tra.record_size(np.full(len(EDGES), code), np.array(EDGES))
        assert np.array_equal(vf.vec3_record_bytes(np.full(len(EDGES), code, np.uint16), np.array(EDGES)), want), code
        assert (want % 8 == 0).all()
        for a, w in zip(EDGES, want):
            assert lib is None or lib.vqhip_vec3_active_record_bytes(int(code), a) == w
    masks = masks_with_counts(EDGES)
    assert np.array_equal(vf._vec3_popcounts(masks), np.array(EDGES)) and np.array_equal(codec.HipVec3Codec.active_counts(masks), np.array(EDGES))
    for bad in (17, 17 << 5, 17 << 10, 0x8000, 0xFFFD):
        with pytest.raises(ValueError, match="neither"):
            vf.vec3_record_bytes(np.array([bad]), np.array([5]))
    with pytest.raises(ValueError, match="0..512"):
        vf.vec3_record_bytes(np.array([0]), np.array([513]))


def test_header_library_and_bindings_hold_exactly_the_six_names():
    assert codec.VEC3_FILE_SYMBOLS == NAMES
    raw = open(os.path.join(ROOT, "include", "vqvdb_hip_vec3_file.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(NAMES)
    assert all("precision" not in n and not n.startswith(("vqhip_vec3_mask_", "vqhip_vec3_active_", "vqhip_vec3_compress")) for n in NAMES)
    assert re.search(r'#include\s+"vqvdb_hip_vec3_active.h"', text)
    for macro, value in (("VERSION", 1), ("HEADER_BYTES", 24), ("KIND_INDICES", 0), ("KIND_ACTIVE", 1)):
        assert re.search(r"#define\s+VQHIP_VEC3_FILE_" + macro + r"\s+" + str(value) + r"\b", text), macro
    assert (vf.VEC3_VERSION, vf.VEC3_HEADER_BYTES, vf.VEC3_KIND_INDICES, vf.VEC3_KIND_ACTIVE, vf.VEC3_MAGIC) == (1, 24, 0, 1, b"VQVEC3")
    assert '"VQVEC3"' in raw and "precision" not in text.replace("vqvdb_hip_vec3_precision.h", "")      # the field is called mode
    for name in NAMES:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert params.count(",") + 1 == ARITY[name], name
    for struct_name, fields in (("vqhip_vec3_grid_source", ("name", "transform", "leaf_ptrs", "origins", "n_leaves", "masks", "background")),
                                ("vqhip_vec3_grid_info", ("name", "transform", "num_codes", "total_blocks", "grid_index", "kind", "mode", "tol",
                                                          "has_background", "background"))):
        body = re.search(r"typedef struct " + struct_name + r"\s*\{(.*?)\}\s*" + struct_name + ";", text, flags=re.S).group(1)
        assert tuple(re.findall(r"(\w+)(?:\[\d+\])?\s*;", body)) == fields, struct_name
    assert tuple(n for n, _ in codec._Vec3GridSource._fields_) == ("name", "transform", "leaf_ptrs", "origins", "n_leaves", "masks", "background")
    assert tuple(n for n, _ in codec._Vec3GridInfo._fields_) == ("name", "transform", "num_codes", "total_blocks", "grid_index", "kind", "mode", "tol",
                                                                  "has_background", "background")
    # the older headers point here instead of saying that nothing reaches the disk
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        assert "no Vec3 file container" not in open(os.path.join(ROOT, "include", h)).read(), h
    others = [v for k, v in vars(codec).items() if k.endswith("_SYMBOLS") and k != "VEC3_FILE_SYMBOLS"]
    assert len(others) >= 11 and not any(set(NAMES) & set(o) for o in others)
    for m in ("encode_leaves", "decode_leaves", "compress_file", "compress_file_active", "decompress_file"):
        assert callable(getattr(codec.HipVec3Codec, m)), m
    if not os.path.exists(codec.LIB_PATH):                         # the checks below need the built library
        return
    lib = codec.load_library()
    for name in NAMES:
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == ARITY[name] and f.restype == ctypes.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_\w+)\b", out))
    assert {n for n in exported if n.startswith("vqhip_vec3_file_") or n.endswith("_leaves") and n.startswith("vqhip_vec3_")} == set(NAMES) | \
        {"vqhip_vec3_set_chunk_leaves", "vqhip_vec3_chunk_leaves"}


def test_a_null_handle_is_refused_and_file_info_needs_no_device(tmp_path):
    if not os.path.exists(codec.LIB_PATH):                         # nothing to call before the library is built
        return
    lib = codec.load_library()
    out = os.fspath(tmp_path / "never.vqv3").encode()
    assert lib.vqhip_vec3_encode_leaves(None, None, 1, None) == -1 and lib.vqhip_vec3_decode_leaves(None, None, 1, None) == -1
    assert lib.vqhip_vec3_file_compress(None, out, None, 1, 0, None) == -1
    assert lib.vqhip_vec3_file_compress_active(None, out, None, 1, 0.5, 0, None, None) == -1
    assert lib.vqhip_vec3_file_decompress(None, out, 0, codec.VEC3_GRID_BEGIN_FN(), codec.VEC3_LEAF_ALLOC_FN(), None, None) == -1
    assert not (tmp_path / "never.vqv3").exists()
    data, header, grids = hand_assembled()
    path = tmp_path / "h.vqv3"
    path.write_bytes(data)
    assert codec.vec3_file_info(path) == {"n_grids": 2, "num_codes": 4096, "kind": 1, "mode": 1, "tol": 0.25, "total_blocks": 2, "payload_bytes": 232}
    for bad, message in ((data[:-1], "truncated|bytes"), (data + b"\0", "imply"), (b"VQVDB" + data[5:], "magic"), (data[:6] + b"\2" + data[7:], "version")):
        path.write_bytes(bad)
        with pytest.raises(RuntimeError, match=message):
            codec.vec3_file_info(path)
    with pytest.raises(RuntimeError, match="Cannot open"):
        codec.vec3_file_info(tmp_path / "missing.vqv3")
    assert lib.vqhip_vec3_file_info(None, None, None, None, None, None, None, None) == -1


def test_wrapper_checks_its_arguments_before_any_device():
    V = codec.HipVec3Codec
    leaf = np.zeros((512, 3), F)
    assert V._leaf_ptrs([leaf, leaf], 2, writable=False).dtype == np.uint64
    for bad in (np.zeros((512, 3), np.float64), np.zeros(512, F), np.zeros((512, 6), F)[:, ::2]):
        with pytest.raises(ValueError, match="leaf buffer 1"):
            V._leaf_ptrs([leaf, bad], 2, writable=False)
    ro = leaf.copy()
    ro.setflags(write=False)
    V._leaf_ptrs([ro], 1, writable=False)
    with pytest.raises(ValueError, match="writable"):
        V._leaf_ptrs([ro], 1, writable=True)
    with pytest.raises(ValueError, match="expected 2"):
        V._leaf_ptrs([leaf], 2, writable=False)
    self = object.__new__(V)                                       # no handle: _grid_sources touches none
    g = {"name": "g", "origins": np.zeros((2, 3), np.int32), "leaves": np.zeros((2, 512, 3), F)}
    src, n_g, _keep = V._grid_sources(self, [g], need_masks=False)
    assert n_g == 1 and src[0].n_leaves == 2 and src[0].masks is None and src[0].background is None and src[0].name == b"g"
    with pytest.raises(ValueError, match="needs masks"):
        V._grid_sources(self, [g], need_masks=True)
    src, _, _keep = V._grid_sources(self, [dict(g, masks=np.ones((2, 512), bool), background=[1, 2, 3])], need_masks=True)
    assert src[0].masks and src[0].background
    with pytest.raises(ValueError, match="masks"):
        V._grid_sources(self, [dict(g, masks=np.zeros((3, 8), np.uint64))], need_masks=True)
    with pytest.raises(ValueError, match="background"):
        V._grid_sources(self, [dict(g, background=[1, 2])], need_masks=False)
    with pytest.raises(ValueError, match="origins but"):
        V._grid_sources(self, [dict(g, leaves=np.zeros((3, 512, 3), F))], need_masks=False)
    self._h = None
