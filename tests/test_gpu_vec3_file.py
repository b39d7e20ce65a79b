"""The Vec3 handle on leaf pointers and on disk (include/vqvdb_hip_vec3_file.h): encode_leaves / decode_leaves against
encode / decode, files of kind 0 and kind 1 against write_vec3 of the in-memory calls' results for every batch size, decompress_file
against decode and decompress_active, and the refusals, all to the bit, in both precision modes.  Leaves, masks and tolerances are
those of tests/test_gpu_vec3_active.py; the handle's chunk is 32 leaves, so that every call runs several chunks."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import masked_gpu_common as mg  # noqa: E402
import torch_ref_masked as trm  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from test_gpu_vec3_active import count_edges  # noqa: E402
from vqvdb_amd import codec as vc, synth_vec3, vqvdbfile as vf, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec, pack_masks  # noqa: E402

pytestmark = pytest.mark.gpu

C = 3
F = np.float32
N0, SPLIT = 136, 97
BATCHES = (32, 33, 4096)
BACKGROUND = np.array([-0.0, np.nan, 1e30], F)
NAMES = ("velocity", "rest", "empty")
MODES = {"fp32": 0, "bf16": 1}


@pytest.fixture(scope="module")
def pack():
    return weightpack.dumps(synth_vec3.make_weights(0))


@pytest.fixture(scope="module")
def codecs(pack):
    cs = {m: HipVec3Codec(pack, precision=m) for m in MODES}
    for c in cs.values():
        c.set_chunk_leaves(32)
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def base(codecs):
    """x [145,512,3] (the 136 leaves and the designed input), origins, transform, the three masks, the three tolerances; computed
    once and left unchanged"""
    leaves = np.concatenate([synth_vec3.make_leaves(128, 4321), synth_vec3.edge_leaves()])
    assert len(leaves) == N0
    dx, _, dact, _ = trm.designed(C)
    x = np.ascontiguousarray(np.concatenate([leaves, dx]))
    _, uerr = codecs["fp32"].roundtrip(leaves)
    variants = mg.mask_variants(x, C, dact)
    variants["count_edges"] = count_edges(len(x))
    rng = np.random.default_rng(9)
    origins = (rng.integers(-1000, 1000, (len(x), 3)) * 8).astype(np.int32)
    transform = rng.standard_normal(16).astype(F)
    masks = {k: pack_masks(variants[k]) for k in ("ones", "sparse", "count_edges", "designed")}
    for a in (x, origins, transform, *variants.values(), *masks.values()):
        a.setflags(write=False)
    return {"x": x, "origins": origins, "transform": transform, "active": variants, "masks": masks, "tols": [mg.tolerances(uerr)[2], float("inf"), 0.0]}


def parts(n):
    return (slice(0, SPLIT), slice(SPLIT, n), slice(0, 0))


def sources(base, masks=None, background=None, as_pointers=False):
    """the grid dicts of the file calls: 97 leaves, the rest, none"""
    x, out = base["x"], []
    for name, s in zip(NAMES, parts(len(x))):
        g = {"name": name, "origins": base["origins"][s], "leaves": [x[i] for i in range(s.start, s.stop)] if as_pointers else x[s],
             "transform": base["transform"] if name == "velocity" else None, "background": background if name != "rest" else None}
        if masks is not None:
            g["masks"] = masks[s]
        out.append(g)
    return out


def expected_bytes(base, header, per_grid, background=None):
    """write_vec3 of the in-memory calls' results: per_grid[i] = (indices, masks, codes, payload) or (indices,)"""
    grids = []
    for name, s, r in zip(NAMES, parts(len(base["x"])), per_grid):
        g = {"name": name, "origins": base["origins"][s], "indices": r[0], "transform": base["transform"] if name == "velocity" else None,
             "background": background if name != "rest" else None}
        if len(r) > 1:
            g.update(masks=r[1], codes=r[2], payload=r[3])
        grids.append(g)
    return vf.dumps_vec3(header, grids)


def shuffled_buffers(x, seed, writable=False):
    """one separately allocated buffer per leaf, allocated in a shuffled order, each holding its leaf"""
    bufs = [None] * len(x)
    for i in np.random.default_rng(seed).permutation(len(x)):
        bufs[i] = np.array(x[i], dtype=F, order="C")
        bufs[i].setflags(write=writable)
    return bufs


@pytest.mark.parametrize("mode", MODES)
def test_leaf_pointer_calls_equal_the_packed_calls(codecs, base, mode):
    c = codecs[mode]
    for n in (1, 33, 97):
        x = base["x"][:n]
        bufs = shuffled_buffers(x, n)
        want = c.encode(x)
        got = c.encode_leaves(bufs)
        assert got.dtype == np.uint16 and np.array_equal(got, want), n
        assert all(mg.same(b, x[i]) for i, b in enumerate(bufs))                         # read-only inputs stay as they were
        dec = c.decode(want)
        outs = shuffled_buffers(np.full((n, 512, 3), 7.0, F), n + 1, writable=True)
        idx = want.copy()
        idx.setflags(write=False)
        c.decode_leaves(idx, outs)
        assert all(mg.same(o, dec[i]) for i, o in enumerate(outs)), n
    lib, h = c._lib, c._h
    assert lib.vqhip_vec3_encode_leaves(h, None, 0, None) == 0 and lib.vqhip_vec3_decode_leaves(h, None, 0, None) == 0
    idx = np.zeros((1, 64), np.uint16)
    assert lib.vqhip_vec3_encode_leaves(h, None, 1, idx.ctypes.data) == -1 and "null pointer" in lib.vqhip_vec3_last_error(h).decode()
    null = np.zeros(1, np.uint64)
    assert lib.vqhip_vec3_encode_leaves(h, null.ctypes.data, 1, idx.ctypes.data) == -1 and "is NULL" in lib.vqhip_vec3_last_error(h).decode()
    out = [np.full((512, 3), 7.0, F)]
    bad = np.full((1, 64), 4096, np.uint16)
    with pytest.raises(RuntimeError, match="out of range"):
        c.decode_leaves(bad, out)
    assert (out[0] == 7.0).all()


@pytest.mark.parametrize("mode", MODES)
def test_kind_0_file_is_write_vec3_of_encode(codecs, base, mode, tmp_path):
    c, x = codecs[mode], base["x"]
    idx = c.encode(x)
    want = expected_bytes(base, {"num_codes": 4096, "kind": 0}, [(idx[s],) for s in parts(len(x))], BACKGROUND)
    for batch in BATCHES:
        path = tmp_path / f"k0_{batch}.vqv3"
        st = c.compress_file(path, sources(base, masks=base["masks"]["sparse"], background=BACKGROUND, as_pointers=batch == 33), batch)   # masks are ignored
        assert path.read_bytes() == want, batch
        assert st["leaves"] == len(x) and st["grids"] == 3
    assert vc.vec3_file_info(path) == {"n_grids": 3, "num_codes": 4096, "kind": 0, "mode": 0, "tol": 0.0, "total_blocks": len(x), "payload_bytes": 0}
    dec = c.decode(idx)
    for batch in BATCHES:
        grids, st = c.decompress_file(path, batch, return_stats=True)
        assert [g["name"] for g in grids] == list(NAMES) and st["leaves"] == len(x)
        for g, s in zip(grids, parts(len(x))):
            n = s.stop - s.start
            assert g["kind"] == 0 and g["masks"] is None and g["num_codes"] == 4096 and g["total_blocks"] == n
            assert np.array_equal(g["origins"], base["origins"][s]) and mg.same(g["leaves"], dec[s]), (batch, g["name"])
            assert sum(g["batches"]) == n and all(b <= min(batch, 32) for b in g["batches"]) and len(g["batches"]) == -(-n // min(batch, 32))
            assert mg.same(g["transform"], base["transform"] if g["name"] == "velocity" else vf.IDENTITY)
            assert (g["background"] is None) == (g["name"] == "rest") and (g["background"] is None or mg.same(g["background"], BACKGROUND))


@pytest.mark.parametrize("variant", ("ones", "sparse", "count_edges"))
@pytest.mark.parametrize("mode", MODES)
def test_kind_1_file_is_write_vec3_of_compress_active(codecs, base, mode, variant, tmp_path):
    c, x, masks, active = codecs[mode], base["x"], base["masks"][variant], base["active"][variant]
    act3 = np.repeat(active[:, :, None], 3, axis=2)
    finite = np.isfinite(x).all(axis=(1, 2))
    assert (~finite).any() and finite.sum() >= N0 - 8
    for tol in base["tols"]:
        res = [c.compress_active(x[s], masks[s], tol) for s in parts(len(x))]
        header = {"num_codes": 4096, "kind": 1, "mode": MODES[mode], "tol": HipVec3Codec.check_tol(tol)}
        for background in (None, BACKGROUND):
            want = expected_bytes(base, header, [(r[0], masks[s], r[1], r[2]) for r, s in zip(res, parts(len(x)))], background)
            assert want[13] == MODES[mode]
            for batch in BATCHES if background is None else BATCHES[1:2]:
                path = tmp_path / f"k1_{batch}.vqv3"
                st = c.compress_file_active(path, sources(base, masks, background, as_pointers=batch == 33), tol, batch)
                assert path.read_bytes() == want, (tol, batch)
                assert st["payload_bytes"] == [len(r[2]) for r in res] and st["leaves"] == len(x)
            info = vc.vec3_file_info(path)
            assert info["mode"] == MODES[mode] and info["kind"] == 1 and info["payload_bytes"] == sum(len(r[2]) for r in res)
            for batch in BATCHES[:2]:
                grids = c.decompress_file(path, batch)
                for g, s, r in zip(grids, parts(len(x)), res):
                    bg = background if g["name"] != "rest" else None
                    ref = c.decompress_active(r[0], masks[s], tol, r[1], r[2], background=bg)
                    assert mg.same(g["leaves"], ref) and np.array_equal(g["masks"], masks[s]) and np.array_equal(g["origins"], base["origins"][s])
                    assert g["mode"] == MODES[mode] and F(g["tol"]).tobytes() == F(header["tol"]).tobytes() and sum(g["batches"]) == s.stop - s.start
                    out, xs, a3 = g["leaves"], x[s], act3[s]
                    if bg is not None:
                        assert out[~a3].reshape(-1, 3).tobytes() == np.tile(BACKGROUND, ((~active[s]).sum(), 1)).tobytes()
                    fin = finite[s]
                    assert (np.abs(xs[fin] - out[fin])[a3[fin]] <= F(header["tol"])).all(), (tol, g["name"])
                    raw = r[1] == t3r.RAW
                    assert out[raw][a3[raw]].tobytes() == xs[raw][a3[raw]].tobytes()
                    nan = np.isnan(np.where(a3, xs, 0)).any(axis=(1, 2))
                    assert raw[nan].all()                                                # a NaN at an active voxel: raw, hence the bits above


def test_the_designed_input_through_a_file(codecs, base, tmp_path):
    c, x = codecs["fp32"], base["x"]
    masks = base["masks"]["designed"]
    s = slice(N0, len(x))
    path = tmp_path / "designed.vqv3"
    g = {"name": "designed", "origins": base["origins"][s], "leaves": x[s], "masks": base["active"]["designed"][s], "background": BACKGROUND}
    c.compress_file_active(path, [g], trm.TOL_D, 4)
    idx, code, payload = c.compress_active(x[s], masks[s], trm.TOL_D)
    h, (got,) = vf.read_vec3(path)
    assert h == {"num_codes": 4096, "kind": 1, "mode": 0, "tol": trm.TOL_D}
    assert np.array_equal(got["indices"], idx) and np.array_equal(got["codes"], code) and np.array_equal(got["payload"], payload)
    assert np.array_equal(got["masks"], masks[s])
    (out,) = c.decompress_file(path, 5)
    assert out["batches"] == [5, 4] and mg.same(out["leaves"], c.decompress_active(idx, masks[s], trm.TOL_D, code, payload, background=BACKGROUND))


def test_refusals_happen_on_the_host_and_leave_the_handle_usable(codecs, base, pack, tmp_path):
    c, b16, x = codecs["fp32"], codecs["bf16"], base["x"]
    masks = base["masks"]["count_edges"]
    tol = base["tols"][0]
    first = c.encode(x[:4])
    lib, h = c._lib, c._h
    good, k0 = tmp_path / "good.vqv3", tmp_path / "k0.vqv3"
    c.compress_file_active(good, sources(base, masks, BACKGROUND), tol, 0)
    c.compress_file(k0, sources(base), 0)
    data = good.read_bytes()
    _, grids = vf.read_vec3(data)
    assert len(grids[0]["payload"]) > 8 and len(grids[1]["payload"]) > 8

    earlier = {id(c): first}

    def usable(codec=c):
        """one encode of 4 leaves gives what it gave before the refusal"""
        assert np.array_equal(codec.encode(x[:4]), earlier[id(codec)])

    def refused(codec, path, message, allowed_allocs=()):
        """VQHIP_ERR_INVALID with a message; leaf_alloc ran for the grids in allowed_allocs only; the handle works as before"""
        seen = []
        if id(codec) not in earlier:
            earlier[id(codec)] = codec.encode(x[:4])

        def on_alloc(_user, gidx, _origins, _masks, n, out_ptrs):
            seen.append(gidx)
            buf = np.empty((n, 512, 3), F)
            keep.append(buf)
            for i in range(n):
                out_ptrs[i] = buf[i].ctypes.data
            return 0

        keep = []
        rc = codec._lib.vqhip_vec3_file_decompress(codec._h, os.fspath(path).encode(), 33, vc.VEC3_GRID_BEGIN_FN(), vc.VEC3_LEAF_ALLOC_FN(on_alloc), None, None)
        text = codec._lib.vqhip_vec3_last_error(codec._h).decode()
        assert rc == -1 and message in text, (rc, text)
        assert set(seen) <= set(allowed_allocs), seen
        usable(codec)

    def patched(at, value, name):
        p = tmp_path / name
        buf = bytearray(data)
        buf[at:at + len(value)] = value
        p.write_bytes(bytes(buf))
        return p

    # the offsets of the second grid's sections, from the layout
    meta0 = 24
    end0 = meta0 + 102 + len(NAMES[0]) + SPLIT * 206 + len(grids[0]["payload"])
    n1 = len(x) - SPLIT
    org1 = end0 + 102 + len(NAMES[1])
    idx1, msk1, cod1 = org1 + 12 * n1, org1 + 140 * n1, org1 + 204 * n1
    # mode mismatch in both directions, before any callback; a kind-0 file carries no mode and opens in either
    refused(b16, good, "fp32 decoder, the handle is in bf16 mode")
    other = tmp_path / "bf16.vqv3"
    b16.compress_file_active(other, sources(base, masks), tol, 0)
    refused(c, other, "bf16 decoder, the handle is in fp32 mode")
    assert mg.same(b16.decompress_file(k0)[0]["leaves"], b16.decode(c.encode(x[:SPLIT])))
    # another K
    small = HipVec3Codec(weightpack.dumps(synth_vec3.make_weights(0, k_codes=512)))
    try:
        refused(small, good, "4096 codes, this model has 512")
        refused(small, k0, "4096 codes, this model has 512")
    finally:
        small.close()
    # damaged bytes of the second grid: the first grid may have been decoded, the refused one sees no leaf_alloc
    refused(c, patched(idx1 + 128 * 40 + 2 * 63, np.uint16(4096).tobytes(), "index.vqv3"), "out of range", allowed_allocs=(0,))
    refused(c, patched(cod1 + 2 * (n1 - 1), np.uint16(17).tobytes(), "code.vqv3"), "0x0011", allowed_allocs=(0,))
    # one mask bit flipped: a leaf whose record grows with one more active voxel (a raw leaf: 8 ceil(3 A / 2) bytes; a quantised one
    # with A a multiple of 64: one more word per plane), the first voxel of its first word with room switched on
    codes1, counts1 = grids[1]["codes"], HipVec3Codec.active_counts(grids[1]["masks"])
    grows = (counts1 < 512) & (vf.vec3_record_bytes(codes1, np.minimum(counts1 + 1, 512)) != vf.vec3_record_bytes(codes1, counts1))
    assert grows.any()
    edge = int(np.flatnonzero(grows)[0])
    words = grids[1]["masks"][edge]
    j = int(np.flatnonzero(words != np.uint64(0xFFFFFFFFFFFFFFFF))[0])
    bit = next(b for b in range(64) if not (int(words[j]) >> b) & 1)
    at = msk1 + 64 * edge + 8 * j + bit // 8
    refused(c, patched(at, bytes([data[at] | 1 << (bit % 8)]), "mask.vqv3"), "payload bytes", allowed_allocs=(0,))
    for cut, name in ((len(data) - 1, "short.vqv3"), (org1 + 5, "cut.vqv3"), (30, "head.vqv3")):
        p = tmp_path / name
        p.write_bytes(data[:cut])
        refused(c, p, ".vqv3")
    p = tmp_path / "long.vqv3"
    p.write_bytes(data + b"\0")
    refused(c, p, "imply")
    refused(c, tmp_path / "missing.vqv3", "Cannot open input file")

    # a callback that returns 1: the call stops at that grid
    calls = []

    def failing(_user, gidx, _origins, _masks, n, _out):
        calls.append((gidx, n))
        return 1

    rc = lib.vqhip_vec3_file_decompress(h, os.fspath(good).encode(), 33, vc.VEC3_GRID_BEGIN_FN(), vc.VEC3_LEAF_ALLOC_FN(failing), None, None)
    assert rc == -1 and "leaf_alloc callback failed (1)" in lib.vqhip_vec3_last_error(h).decode() and calls == [(0, 32)]
    usable()
    begun = []

    def no_grid(_user, gi):
        begun.append(gi.contents.grid_index)
        return 1

    rc = lib.vqhip_vec3_file_decompress(h, os.fspath(good).encode(), 33, vc.VEC3_GRID_BEGIN_FN(no_grid), vc.VEC3_LEAF_ALLOC_FN(failing), None, None)
    assert rc == -1 and "grid_begin callback failed" in lib.vqhip_vec3_last_error(h).decode() and begun == [0] and calls == [(0, 32)]
    usable()
    null_alloc = lib.vqhip_vec3_file_decompress(h, os.fspath(good).encode(), 33, vc.VEC3_GRID_BEGIN_FN(), vc.VEC3_LEAF_ALLOC_FN(), None, None)
    assert null_alloc == -1 and "null path or leaf allocator" in lib.vqhip_vec3_last_error(h).decode()

    # compress: NULL masks for kind 1, an unwritable path, a NULL leaf pointer in the second grid; no output file is left
    src, n_g, _keep = c._grid_sources(sources(base, masks), need_masks=True)
    out = tmp_path / "refused.vqv3"
    src[1].masks = None
    assert lib.vqhip_vec3_file_compress_active(h, os.fspath(out).encode(), src, n_g, tol, 33, None, None) == -1
    assert "has no masks" in lib.vqhip_vec3_last_error(h).decode() and not out.exists()
    usable()
    src, n_g, _keep = c._grid_sources(sources(base, masks, as_pointers=True), need_masks=True)
    nowhere = tmp_path / "no_such_directory" / "f.vqv3"
    assert lib.vqhip_vec3_file_compress_active(h, os.fspath(nowhere).encode(), src, n_g, tol, 33, None, None) == -1
    assert "Cannot open output file" in lib.vqhip_vec3_last_error(h).decode() and not nowhere.parent.exists()
    assert lib.vqhip_vec3_file_compress(h, os.fspath(nowhere).encode(), src, n_g, 33, None) == -1
    usable()
    ptrs = _keep[9]                                                                      # the second grid's leaf addresses
    assert ptrs.dtype == np.uint64 and len(ptrs) == n1
    ptrs[n1 - 1] = 0
    assert lib.vqhip_vec3_file_compress_active(h, os.fspath(out).encode(), src, n_g, tol, 33, None, None) == -1
    assert "is NULL" in lib.vqhip_vec3_last_error(h).decode() and not out.exists()       # the first grid was written, the file is gone
    usable()
    for bad_n in (0, 256):
        assert lib.vqhip_vec3_file_compress(h, os.fspath(out).encode(), src, bad_n, 33, None) == -1 and not out.exists()
    with pytest.raises(ValueError, match="needs masks"):
        c.compress_file_active(out, sources(base), tol)
    with pytest.raises(TypeError):
        c.compress_file_active(out, sources(base, masks), "0.5")
    # the handles still work, and give what they gave
    usable()
    usable(b16)
    assert mg.same(c.decompress_file(good, 33)[1]["leaves"][-9:], c.decompress_file(good, 32)[1]["leaves"][-9:])


@pytest.mark.parametrize("mode", MODES)
def test_the_in_memory_calls_are_unchanged_by_file_calls(pack, base, mode, tmp_path):
    x, masks, tol = base["x"], base["masks"]["sparse"], base["tols"][0]
    c = HipVec3Codec(pack, precision=mode)
    try:
        c.set_chunk_leaves(32)

        def snapshot():
            idx = c.encode(x)
            ci, cc, cp = c.compress_active(x, masks, tol)
            return [idx, c.decode(idx), ci, cc, cp, c.decompress_active(ci, masks, tol, cc, cp, background=BACKGROUND)]

        before = snapshot()
        path = tmp_path / "f.vqv3"
        c.compress_file(path, sources(base), 33)
        c.decompress_file(path, 4096)
        c.compress_file_active(path, sources(base, masks, BACKGROUND, as_pointers=True), tol, 33)
        c.decompress_file(path, 7)
        c.encode_leaves([x[i] for i in range(33)])
        assert c.chunk_leaves() == 32 and c.precision == mode
        assert all(mg.same(a, b) for a, b in zip(before, snapshot()))
    finally:
        c.close()
