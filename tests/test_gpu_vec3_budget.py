"""The Vec3 handle's compress into a byte budget on compact records (include/vqvdb_hip_vec3_budget.h), in memory and
into a .vqv3 file, in both precision modes, all to the bit: the sizes against rate_sweep_active, the chosen rung against the pick
restated in tests/test_vec3_budget_host.py, every output against compress_active / compress_file_active at that rung, the file's
size against the formula, and the refusals.  Leaves, masks and tolerances are those of tests/test_gpu_vec3_active.py; the handle's
chunk is 32 leaves, so that every call runs several chunks and pass 2 meets chunks with all, some, one and none of their leaves
selected.

"A mode switch between two calls" is read as §26 reads it: a file written in one mode is refused by a handle in the other, whether
that is a second handle or the writing handle after vqhip_vec3_set_precision."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import masked_gpu_common as mg  # noqa: E402
import torch_ref_active as tra  # noqa: E402,F401  (the restatement the compared calls are held against in test_gpu_vec3_active.py)
import torch_ref_masked as trm  # noqa: E402
import torch_ref_vec3_residual as t3r  # noqa: E402
from test_gpu_vec3_active import count_edges  # noqa: E402
from test_vec3_budget_host import ref_file_bytes, ref_pick  # noqa: E402
from vqvdb_amd import codec as vc, synth_vec3, vqvdbfile as vf, weightpack  # noqa: E402
from vqvdb_amd.codec import HipVec3Codec, pack_masks  # noqa: E402

pytestmark = pytest.mark.gpu

C = 3
F = np.float32
N0, SPLIT = 136, 97
BATCHES = (32, 33, 4096)
NAMES = ("velocity", "rest", "empty")
MODES = {"fp32": 0, "bf16": 1}
BACKGROUND = np.array([-0.0, np.nan, 1e30], F)
FILL = 0xA5


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
    """x [145,512,3] (the 136 leaves and the designed input), origins, the masks, and the rungs: the seven tolerances of
    tests/test_gpu_vec3_active.py plus TOL_D, NaN and +inf, shuffled; computed once and left unchanged"""
    leaves = np.concatenate([synth_vec3.make_leaves(128, 4321), synth_vec3.edge_leaves()])
    assert len(leaves) == N0
    dx, _, dact, _ = trm.designed(C)
    x = np.ascontiguousarray(np.concatenate([leaves, dx]))
    _, uerr = codecs["fp32"].roundtrip(leaves)
    variants = mg.mask_variants(x, C, dact)
    variants["count_edges"] = count_edges(len(x))
    rungs = mg.tolerances(uerr) + [trm.TOL_D, float("nan"), float("inf")]
    rungs = [rungs[i] for i in np.random.default_rng(11).permutation(len(rungs))]
    assert len(rungs) == 10 and sum(np.isnan(rungs)) == 2 and sum(np.isinf(rungs)) == 2
    origins = (np.random.default_rng(9).integers(-1000, 1000, (len(x), 3)) * 8).astype(np.int32)
    masks = {k: pack_masks(variants[k]) for k in ("ones", "sparse", "count_edges", "designed")}
    for a in (x, origins, *variants.values(), *masks.values()):
        a.setflags(write=False)
    return {"x": x, "origins": origins, "active": variants, "masks": masks, "rungs": rungs, "median": mg.tolerances(uerr)[2]}


def parts(n):
    return (slice(0, SPLIT), slice(SPLIT, n), slice(0, 0))


def sources(base, masks, background=None, as_pointers=False):
    """the grid dicts of the file calls: 97 leaves, the rest, none"""
    x, out = base["x"], []
    for name, s in zip(NAMES, parts(len(x))):
        out.append({"name": name, "origins": base["origins"][s], "leaves": [x[i] for i in range(s.start, s.stop)] if as_pointers else x[s],
                    "background": background if name != "rest" else None, "masks": masks[s]})
    return out


def same_tol(a, b):
    return F(a).tobytes() == F(b).tobytes() or (np.isnan(a) and np.isnan(b))


def budgets_of(sizes):
    """each distinct size, that size minus 1, and 0"""
    return sorted({0} | {int(s) for s in sizes} | {int(s) - 1 for s in sizes if s > 0})


def raw_budget_compress(c, x, masks, rungs, budget):
    """the C call on buffers filled with FILL -> (rc, message, tol_used, bytes, indices, leaf_code, payload, payload_bytes)"""
    n, t = len(x), np.asarray(rungs, F)
    sizes, idx, err = np.full(len(t), -7, np.int64), np.zeros((n, 64), np.uint16), np.zeros((n, 2), F)
    lc, payload = np.full(n, FILL * 257, np.uint16), np.full(n * 6144, FILL, np.uint8)
    used, nbytes = ctypes.c_float(-3.0), ctypes.c_int64(-3)
    rc = c._lib.vqhip_vec3_budget_compress(c._h, x.ctypes.data, masks.ctypes.data, n, t.ctypes.data, len(t), budget, ctypes.byref(used), sizes.ctypes.data,
                                           idx.ctypes.data, err.ctypes.data, lc.ctypes.data, payload.ctypes.data, ctypes.byref(nbytes))
    return rc, c._lib.vqhip_vec3_last_error(c._h).decode(), used.value, sizes, idx, lc, payload, nbytes.value


@pytest.mark.parametrize("variant", ("ones", "sparse", "count_edges", "designed"))
@pytest.mark.parametrize("mode", MODES)
def test_in_memory_budget_compress_equals_compress_active_at_the_picked_rung(codecs, base, mode, variant):
    c, x, masks, rungs = codecs[mode], base["x"], base["masks"][variant], base["rungs"]
    sweep = c.rate_sweep_active(x, masks, rungs)
    finite = [s for s, t in zip(sweep, rungs) if not np.isnan(t)]
    assert len(set(int(s) for s in sweep)) >= 3, sweep
    refs, refused, chosen = {}, 0, set()
    for budget in budgets_of(sweep):
        want = ref_pick([int(s) for s in sweep], rungs, budget)
        if want < 0:
            rc, text, used, sizes, idx, lc, payload, nbytes = raw_budget_compress(c, x, masks, rungs, budget)
            assert rc == -1 and nbytes == 0 and used == -3.0, (budget, rc, text)
            assert (lc == FILL * 257).all() and (payload == FILL).all(), "leaf_code or payload touched although nothing fits"
            assert f"has {min(finite)} bytes" in text and f"the budget is {budget} bytes" in text, text
            assert np.array_equal(sizes, sweep) and np.array_equal(idx, c.compress_active(x, masks, 0.5)[0])   # pass 1's values
            with pytest.raises(RuntimeError, match="the budget is"):
                c.rate_compress_active(x, masks, rungs, budget)
            refused += 1
            continue
        used, sizes, idx, lc, payload, err = c.rate_compress_active(x, masks, rungs, budget, return_leaf_err=True)
        assert same_tol(used, rungs[want]), (budget, used, rungs[want])
        assert np.array_equal(sizes, sweep), budget
        key = F(used).tobytes()
        if key not in refs:
            refs[key] = c.compress_active(x, masks, used, return_leaf_err=True)
        ridx, rlc, rpayload, rerr = refs[key]
        assert mg.same(idx, ridx) and mg.same(lc, rlc) and mg.same(payload, rpayload) and mg.same(err, rerr), (budget, used)
        assert len(payload) == sweep[want] <= budget
        chosen.add(want)
    assert len(chosen) >= 3, chosen                                                          # the budgets walk the ladder
    if variant == "ones":
        assert refused >= 1                                                                  # the leaves with NaN are raw at every rung: 0 bytes never fit
    # without the optional outputs, and the fill of the payload beyond its bytes
    budget = int(max(finite))
    rc, text, used, sizes, idx, lc, payload, nbytes = raw_budget_compress(c, x, masks, rungs, budget)
    want = ref_pick([int(s) for s in sweep], rungs, budget)
    assert rc == 0 and same_tol(used, rungs[want]) and nbytes == sweep[want], text
    assert (payload[nbytes:] == FILL).all(), "bytes written beyond the payload"
    n, t = len(x), np.asarray(rungs, F)
    lc2, p2, used2, nb2 = np.zeros(n, np.uint16), np.full(n * 6144, FILL, np.uint8), ctypes.c_float(), ctypes.c_int64()
    idx2 = np.zeros((n, 64), np.uint16)
    rc = c._lib.vqhip_vec3_budget_compress(c._h, x.ctypes.data, masks.ctypes.data, n, t.ctypes.data, len(t), budget, ctypes.byref(used2), None,
                                           idx2.ctypes.data, None, lc2.ctypes.data, p2.ctypes.data, ctypes.byref(nb2))
    assert rc == 0 and mg.same(lc2, lc) and mg.same(p2, payload) and mg.same(idx2, idx) and nb2.value == nbytes


@pytest.mark.parametrize("variant", ("ones", "sparse", "count_edges"))
@pytest.mark.parametrize("mode", MODES)
def test_file_budget_compress_equals_compress_file_active_at_the_picked_rung(codecs, base, mode, variant, tmp_path):
    c, x, masks, rungs = codecs[mode], base["x"], base["masks"][variant], base["rungs"]
    active = base["active"][variant]
    src = sources(base, masks, BACKGROUND)
    per_grid = np.stack([c.rate_sweep_active(x[s], masks[s], rungs) for s in parts(len(x))])
    assert not per_grid[2].any() and per_grid[0].any() and per_grid[1].any()
    for batch in BATCHES:
        got = c.rate_sweep_file(sources(base, masks, as_pointers=batch == 33), rungs, batch)
        assert got.dtype == np.int64 and np.array_equal(got, per_grid), batch
    file_sizes = [vc.vec3_file_bytes(src, 1, per_grid[:, t]) for t in range(len(rungs))]
    counts = [s.stop - s.start for s in parts(len(x))]
    assert file_sizes == [ref_file_bytes(NAMES, counts, 1, [int(b) for b in per_grid[:, t]]) for t in range(len(rungs))]
    target = file_sizes[rungs.index(base["median"])]
    refs = {}
    for budget in (target, target - 1):
        want = ref_pick(file_sizes, rungs, budget)
        assert want >= 0
        for batch in BATCHES:
            path = tmp_path / f"b_{budget}_{batch}.vqv3"
            st = c.compress_file_budget(path, sources(base, masks, BACKGROUND, as_pointers=batch == 33), rungs, budget, batch)
            assert same_tol(st["tol_used"], rungs[want]), (budget, batch, st["tol_used"])
            key = F(st["tol_used"]).tobytes()
            if key not in refs:
                ref_path = tmp_path / f"ref_{len(refs)}.vqv3"
                rst = c.compress_file_active(ref_path, src, st["tol_used"], 32)
                refs[key] = (ref_path.read_bytes(), rst["payload_bytes"])
            assert path.read_bytes() == refs[key][0], (budget, batch)
            assert st["payload_bytes"] == refs[key][1] == [int(b) for b in per_grid[:, want]]
            assert st["file_bytes"] == os.path.getsize(path) == vc.vec3_file_bytes(src, 1, st["payload_bytes"]) == file_sizes[want] <= budget
            assert st["leaves"] == len(x) and st["grids"] == 3 and st["wall_s"] > 0
    assert len(refs) == 2                                                                    # one byte below the size: the next rung
    # the bound at every active value of every finite leaf, through decompress_file
    info = vc.vec3_file_info(path)
    assert info["kind"] == 1 and info["mode"] == MODES[mode] and same_tol(info["tol"], st["tol_used"])
    finite = np.isfinite(x).all(axis=(1, 2))
    act3 = np.repeat(active[:, :, None], 3, axis=2)
    for g, s in zip(c.decompress_file(path, 33), parts(len(x))):
        out, xs, a3, fin = g["leaves"], x[s], act3[s], finite[s]
        assert np.array_equal(g["masks"], masks[s]) and np.array_equal(g["origins"], base["origins"][s])
        assert (np.abs(xs[fin] - out[fin])[a3[fin]] <= F(st["tol_used"])).all(), g["name"]
    # no rung fits: the output is not created, a file planted at the path keeps its bytes
    least = min(f for f, t in zip(file_sizes, rungs) if not np.isnan(t))
    missing, planted = tmp_path / "never.vqv3", tmp_path / "planted.vqv3"
    planted.write_bytes(b"the bytes that were here before")
    for p in (missing, planted):
        with pytest.raises(RuntimeError) as e:
            c.compress_file_budget(p, src, rungs, least - 1, 33)
        assert f"has {least} bytes" in str(e.value) and f"the budget is {least - 1} bytes" in str(e.value)
    assert not missing.exists() and planted.read_bytes() == b"the bytes that were here before"
    st = c.compress_file_budget(planted, src, rungs, least, 33)
    assert st["file_bytes"] == least == os.path.getsize(planted)


@pytest.mark.parametrize("mode", MODES)
def test_pass_2_works_on_the_selected_leaves_only(codecs, base, mode, tmp_path):
    c = codecs[mode]
    x = np.array(base["x"][:128])                                                            # NaN-free
    assert np.isfinite(x).all()
    masks = pack_masks(np.ones((128, 512), bool))
    inf, nan = float("inf"), float("nan")
    # every leaf is kept under +inf: no chunk has a selected leaf and the payload is empty
    used, sizes, idx, lc, payload = c.rate_compress_active(x, masks, [inf], 0)
    ridx, rlc, rpayload = c.compress_active(x, masks, inf)
    assert used == inf and sizes.tolist() == [0] and (lc == t3r.KEPT).all() and len(payload) == 0
    assert mg.same(idx, ridx) and mg.same(lc, rlc) and len(rpayload) == 0
    # one NaN planted: a chunk with a single selected leaf alongside chunks with none
    x[40, 17, 1] = nan
    ridx, rlc, rpayload = c.compress_active(x, masks, inf)
    assert (rlc != t3r.KEPT).sum() == 1 and rlc[40] == t3r.RAW and len(rpayload) == 6144
    used, sizes, idx, lc, payload = c.rate_compress_active(x, masks, [nan, inf], 6144)
    assert used == inf and sizes.tolist() == [128 * 6144, 6144]
    assert mg.same(idx, ridx) and mg.same(lc, rlc) and mg.same(payload, rpayload)
    with pytest.raises(RuntimeError, match="has 6144 bytes, the budget is 6143 bytes"):
        c.rate_compress_active(x, masks, [nan, inf], 6143)
    # the same through a file, the selected leaf in the second grid, in a batch of its own kind (the last of 33 + 33 + 31 + ...)
    grids = [{"name": "a", "origins": base["origins"][:30], "leaves": x[:30], "masks": masks[:30]},
             {"name": "b", "origins": base["origins"][30:128], "leaves": [x[i] for i in range(30, 128)], "masks": masks[30:128]}]
    ref, out = tmp_path / "ref.vqv3", tmp_path / "out.vqv3"
    c.compress_file_active(ref, grids, inf, 32)
    size = os.path.getsize(ref)
    for batch in (7, 32, 4096):
        st = c.compress_file_budget(out, grids, [nan, inf], size, batch)
        assert out.read_bytes() == ref.read_bytes() and st["payload_bytes"] == [0, 6144] and st["file_bytes"] == size and st["tol_used"] == inf
    # some of a chunk's leaves selected, at a tolerance between the leaves' errors: pass 2 gathers them
    _, err = c.roundtrip(x[:64])
    tol = float(np.sort(err[np.isfinite(err[:, 0]), 0])[30])
    ridx, rlc, rpayload = c.compress_active(x[:64], masks[:64], tol)
    kept = (rlc == t3r.KEPT).sum()
    assert 0 < kept < 64 and 0 < (rlc[:32] == t3r.KEPT).sum() < 32
    used, sizes, idx, lc, payload = c.rate_compress_active(x[:64], masks[:64], [tol], len(rpayload))
    assert same_tol(used, tol) and mg.same(idx, ridx) and mg.same(lc, rlc) and mg.same(payload, rpayload)


def test_refusals_leave_no_output_and_a_usable_handle(codecs, base, tmp_path):
    c, b16, x, rungs = codecs["fp32"], codecs["bf16"], base["x"], base["rungs"]
    masks = base["masks"]["count_edges"]
    lib, h = c._lib, c._h
    earlier = {id(k): (k.encode(x[:4]), k.compress_active(x[:40], masks[:40], base["median"])) for k in (c, b16)}

    def usable(k=c):
        """the handle gives the bits it gave before the refusal"""
        assert np.array_equal(k.encode(x[:4]), earlier[id(k)][0])
        assert all(mg.same(a, b) for a, b in zip(k.compress_active(x[:40], masks[:40], base["median"]), earlier[id(k)][1]))

    t = np.asarray(rungs, F)
    used, size = ctypes.c_float(-3.0), ctypes.c_int64(-3)
    out = tmp_path / "refused.vqv3"
    big = 1 << 40

    def file_call(src, n_g, path=out, tols=t, n_tols=len(t), budget=big, used_p=ctypes.byref(used), size_p=ctypes.byref(size)):
        rc = lib.vqhip_vec3_budget_file_compress(h, os.fspath(path).encode(), src, n_g, tols.ctypes.data if tols is not None else None, n_tols, budget, 33,
                                                 None, used_p, None, size_p)
        return rc, lib.vqhip_vec3_last_error(h).decode()

    def sweep_call(src, n_g, n_tols=len(t)):
        sizes = np.full((3, len(t)), -7, np.int64)
        rc = lib.vqhip_vec3_budget_file_sweep(h, src, n_g, t.ctypes.data, n_tols, 33, sizes.ctypes.data)
        return rc, lib.vqhip_vec3_last_error(h).decode()

    # a mode switch between two calls: the file belongs to the mode that wrote it
    good = tmp_path / "good.vqv3"
    st = c.compress_file_budget(good, sources(base, masks), rungs, big, 33)
    assert st["tol_used"] == min(r for r in rungs if not np.isnan(r)) == 0.0
    with pytest.raises(RuntimeError, match="fp32 decoder, the handle is in bf16 mode"):
        b16.decompress_file(good)
    usable(b16)
    first = c.decompress_file(good)[0]["leaves"]
    c.precision = "bf16"
    try:
        with pytest.raises(RuntimeError, match="fp32 decoder, the handle is in bf16 mode"):
            c.decompress_file(good)
        other = tmp_path / "bf16.vqv3"
        assert vc.vec3_file_info(good)["mode"] == 0
        c.compress_file_budget(other, sources(base, masks), rungs, big, 33)
        assert vc.vec3_file_info(other)["mode"] == 1 and other.read_bytes() != good.read_bytes()
    finally:
        c.precision = "fp32"
    with pytest.raises(RuntimeError, match="bf16 decoder, the handle is in fp32 mode"):
        c.decompress_file(other)
    assert mg.same(c.decompress_file(good)[0]["leaves"], first)
    usable()
    # NULL masks in the second grid
    src, n_g, _keep = c._grid_sources(sources(base, masks), need_masks=True)
    src[1].masks = None
    for rc, text in (file_call(src, n_g), sweep_call(src, n_g)):
        assert rc == -1 and "has no masks" in text, text
    assert not out.exists() and used.value == -3.0 and size.value == -3
    usable()
    # an unwritable path
    src, n_g, _keep = c._grid_sources(sources(base, masks, as_pointers=True), need_masks=True)
    nowhere = tmp_path / "no_such_directory" / "f.vqv3"
    rc, text = file_call(src, n_g, path=nowhere)
    assert rc == -1 and "Cannot open output file" in text and not nowhere.parent.exists() and used.value == -3.0
    usable()
    # arguments
    for bad in (0, 65, -1):
        rc, text = file_call(src, n_g, n_tols=bad)
        assert rc == -1 and "n_tols" in text
        rc, text = sweep_call(src, n_g, n_tols=bad)
        assert rc == -1 and "n_tols" in text
    assert file_call(src, n_g, budget=-1) == (-1, "vec3 compress_file_budget: file_budget < 0")
    assert file_call(src, n_g, tols=None)[0] == -1 and file_call(src, n_g, used_p=None)[0] == -1 and file_call(src, n_g, size_p=None)[0] == -1
    for bad_n in (0, 256):
        assert file_call(src, bad_n)[0] == -1 and sweep_call(src, bad_n)[0] == -1
    assert lib.vqhip_vec3_budget_file_sweep(h, src, n_g, t.ctypes.data, len(t), 33, None) == -1
    assert not out.exists()
    # a NULL leaf pointer in the second grid: found in pass 1, before the output is opened
    planted = tmp_path / "planted.vqv3"
    planted.write_bytes(b"still here")
    ptrs = _keep[9]                                                                          # the second grid's leaf addresses
    n1 = len(x) - SPLIT
    assert ptrs.dtype == np.uint64 and len(ptrs) == n1
    ptrs[n1 - 1] = 0
    for rc, text in (file_call(src, n_g), file_call(src, n_g, path=planted), sweep_call(src, n_g)):
        assert rc == -1 and "is NULL" in text, text
    assert not out.exists() and planted.read_bytes() == b"still here" and used.value == -3.0 and size.value == -3
    usable()
    # the in-memory call: the refusals of the byte-budget call without masks, and NULL masks
    n = 8
    xs, ms = np.ascontiguousarray(x[:n]), np.ascontiguousarray(masks[:n])
    idx, lc, payload, nbytes = np.zeros((n, 64), np.uint16), np.zeros(n, np.uint16), np.zeros(n * 6144, np.uint8), ctypes.c_int64(-3)

    def mem_call(leaves=xs, m=ms, count=n, n_tols=len(t), budget=big, used_p=ctypes.byref(used), nbytes_p=ctypes.byref(nbytes), indices=idx):
        rc = lib.vqhip_vec3_budget_compress(h, None if leaves is None else leaves.ctypes.data, None if m is None else m.ctypes.data, count, t.ctypes.data,
                                            n_tols, budget, used_p, None, None if indices is None else indices.ctypes.data, None, lc.ctypes.data,
                                            payload.ctypes.data, nbytes_p)
        return rc, lib.vqhip_vec3_last_error(h).decode()

    assert mem_call(m=None) == (-1, "vec3 rate_compress_active: null pointer") and nbytes.value == 0
    assert mem_call(leaves=None)[0] == -1 and mem_call(indices=None)[0] == -1
    assert mem_call(count=-1)[0] == -1 and mem_call(budget=-1)[0] == -1 and mem_call(used_p=None)[0] == -1 and mem_call(nbytes_p=None)[0] == -1
    for bad in (0, 65):
        assert "n_tols" in mem_call(n_tols=bad)[1]
    used.value, nbytes.value = -3.0, -3
    assert mem_call(leaves=None, m=None, count=0, budget=0) == (0, lib.vqhip_vec3_last_error(h).decode()) and nbytes.value == 0 and used.value == 0.0
    with pytest.raises(ValueError, match="needs masks"):
        c.compress_file_budget(out, [{k: v for k, v in g.items() if k != "masks"} for g in sources(base, masks)], rungs, big)
    assert not out.exists()
    usable()
    usable(b16)
