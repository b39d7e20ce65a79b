"""The host arithmetic and the interface of include/vqvdb_hip_vec3_budget.h without a GPU: a numpy restatement of the
pick and of the .vqv3 file size held against vqhip_vec3_budget_pick and vqhip_vec3_budget_file_bytes, the file size against
len(dumps_vec3(...)) for both kinds, and names, arities and lists of the header, the library and the bindings."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from vqvdb_amd import codec, vqvdbfile as vf  # noqa: E402

F = np.float32
NAMES = ["vqhip_vec3_budget_pick", "vqhip_vec3_budget_file_bytes", "vqhip_vec3_budget_compress", "vqhip_vec3_budget_file_sweep",
         "vqhip_vec3_budget_file_compress"]
ARITY = dict(zip(NAMES, (4, 4, 14, 7, 12)))
NAN, INF = float("nan"), float("inf")


def have_library():
    return os.path.exists(codec.LIB_PATH)


def ref_pick(sizes, tols, budget):
    """the index of the smallest tolerance by value whose size fits; NaN never; of equal tolerances the first; -1 if none"""
    if not 1 <= len(tols) <= 64 or len(sizes) != len(tols) or budget < 0 or any(s < 0 for s in sizes):
        return -1
    best = -1
    for t, (s, tol) in enumerate(zip(sizes, np.asarray(tols, F))):
        if tol == tol and s <= budget and (best < 0 or tol < F(tols[best])):
            best = t
    return best


def ref_file_bytes(names, counts, kind, payloads):
    return 24 + sum(102 + len(n.encode()) + c * (12 + 128 + (66 if kind == 1 else 0)) for n, c in zip(names, counts)) + sum(payloads)


def c_pick(sizes, tols, budget, n_tols=None):
    s, t = np.asarray(sizes, np.int64), np.asarray(tols, F)
    return int(codec.load_library().vqhip_vec3_budget_pick(s.ctypes.data, t.ctypes.data, len(t) if n_tols is None else n_tols, budget))


PICK_CASES = {
    "sizes fall": ([900, 500, 100, 0], [0.1, 0.2, 0.4, 0.8]),
    "sizes rise with the tolerance": ([100, 500, 900, 2000], [0.1, 0.2, 0.4, 0.8]),
    "sizes rise and fall": ([700, 300, 900, 200, 650], [0.1, 0.2, 0.4, 0.8, 1.6]),
    "shuffled rungs": ([200, 900, 300, 700], [0.8, 0.4, 0.2, 0.1]),
    "a NaN rung with the smallest size": ([0, 700, 300], [NAN, 0.1, 0.2]),
    "duplicates: the first wins": ([300, 300, 800, 300], [0.2, 0.2, 0.1, 0.2]),
    "negative, zero and +inf rungs": ([6144, 6000, 5000, 0], [-1.0, 0.0, 0.5, INF]),
    "-0 and +0 are one value: the first": ([10, 10], [0.0, -0.0]),
    "every rung NaN": ([0, 0], [NAN, NAN]),
    "one rung": ([512], [0.25]),
}


@pytest.mark.parametrize("name", PICK_CASES)
def test_the_pick_equals_the_restatement(name):
    sizes, tols = PICK_CASES[name]
    budgets = sorted({0, 2**62} | {s + d for s in sizes for d in (-1, 0, 1) if s + d >= 0})   # every size, one byte below and above it
    want = [ref_pick(sizes, tols, b) for b in budgets]
    if name == "sizes rise with the tolerance":
        assert want[budgets.index(100)] == 0 and want[budgets.index(99)] == -1
    if name == "sizes rise and fall":
        assert want[budgets.index(300)] == 1 and want[budgets.index(299)] == 3 and want[budgets.index(199)] == -1
    if name == "a NaN rung with the smallest size":
        assert want[budgets.index(0)] == -1 and want[budgets.index(300)] == 2
    if name == "duplicates: the first wins":
        assert want[budgets.index(300)] == 0 and want[budgets.index(800)] == 2
    if name == "negative, zero and +inf rungs":
        assert want[budgets.index(0)] == 3 and want[budgets.index(5000)] == 2 and want[budgets.index(6144)] == 0
    if name == "every rung NaN":
        assert set(want) == {-1}
    if not have_library():
        return
    for b, w in zip(budgets, want):
        assert c_pick(sizes, tols, b) == w, (name, b)
        if any(t < 0 for t in tols):                                  # the wrapper refuses the negative rungs that the C call takes
            with pytest.raises(ValueError, match="tol must be >= 0"):
                codec.vec3_active_rate_pick(sizes, tols, b)
        elif w >= 0:
            assert codec.vec3_active_rate_pick(sizes, tols, b) == w
        else:
            with pytest.raises(ValueError, match="no rung fits"):
                codec.vec3_active_rate_pick(sizes, tols, b)


def test_the_pick_refuses_bad_arguments():
    assert ref_pick([1], [0.5], -1) == -1 and ref_pick([], [], 5) == -1 and ref_pick([0] * 65, [0.5] * 65, 5) == -1 and ref_pick([1, -1], [0.5, 0.6], 5) == -1
    assert ref_pick([7] * 64, list(np.linspace(1, 2, 64)), 7) == 0
    if not have_library():
        return
    lib = codec.load_library()
    s, t = np.array([1, 2], np.int64), np.array([0.5, 0.25], F)
    assert c_pick(s, t, 5) == 1
    assert c_pick(s, t, -1) == -1 and c_pick(s, t, 5, n_tols=0) == -1 and c_pick(np.zeros(65, np.int64), np.ones(65, F), 5) == -1
    assert c_pick([1, -1], [0.5, 0.6], 5) == -1 and c_pick([-1, 1], [NAN, 0.6], 5) == -1       # a negative size, even on a NaN rung
    assert c_pick([7] * 64, np.linspace(1, 2, 64), 7) == 0
    assert lib.vqhip_vec3_budget_pick(None, t.ctypes.data, 2, 5) == -1 and lib.vqhip_vec3_budget_pick(s.ctypes.data, None, 2, 5) == -1
    with pytest.raises(ValueError, match="1..64"):
        codec.vec3_active_rate_pick([], [], 5)
    with pytest.raises(ValueError, match="1..64"):
        codec.vec3_active_rate_pick([0] * 65, [0.5] * 65, 5)
    with pytest.raises(ValueError, match="sizes"):
        codec.vec3_active_rate_pick([1, 2, 3], [0.5, 0.6], 5)
    with pytest.raises(ValueError, match="negative"):
        codec.vec3_active_rate_pick([1, -2], [0.5, 0.6], 5)
    with pytest.raises(ValueError, match="budget"):
        codec.vec3_active_rate_pick([1, 2], [0.5, 0.6], -1)
    with pytest.raises(TypeError):
        codec.vec3_active_rate_pick([1, 2], [0.5, 0.6], 5.0)


def file_grids(kind, background):
    """two grids and an empty one, names of 0 and 300 bytes, as dumps_vec3 takes them"""
    rng = np.random.default_rng(3)
    out = []
    for name, n in (("", 23), ("empty", 0), ("n" * 300, 9)):
        g = {"name": name, "origins": rng.integers(-99, 99, (n, 3)).astype(np.int32) * 8, "indices": rng.integers(0, 4096, (n, 64)).astype(np.uint16),
             "background": background if name != "empty" else None}
        if kind:
            active = rng.random((n, 512)) < 0.3
            g["masks"] = codec.pack_masks(active)
            g["codes"] = np.array([(0xFFFE, 0xFFFF, 0, 3 | 2 << 5 | 16 << 10)[i % 4] for i in range(n)], np.uint16)
            g["payload"] = rng.integers(0, 256, int(vf.vec3_record_bytes(g["codes"], active.sum(axis=1)).sum())).astype(np.uint8)
        out.append(g)
    return out


@pytest.mark.parametrize("background", (None, [1.0, -0.0, 3.5]))
@pytest.mark.parametrize("kind", (0, 1))
def test_the_file_size_equals_the_length_of_dumps_vec3(kind, background):
    grids = file_grids(kind, background)
    data = vf.dumps_vec3({"num_codes": 4096, "kind": kind, "mode": 0, "tol": 0.5}, grids)
    payloads = [len(g["payload"]) if kind else 0 for g in grids]
    assert not kind or (payloads[0] > 0 and payloads[1] == 0 and payloads[2] > 0)
    want = ref_file_bytes([g["name"] for g in grids], [len(g["origins"]) for g in grids], kind, payloads)
    assert len(data) == want
    assert vf.vec3_file_bytes(grids, kind, payloads if kind else None) == want
    assert vf.vec3_file_bytes([{"name": g["name"], "n_leaves": len(g["origins"])} for g in grids], kind, payloads) == want
    assert vf.vec3_file_bytes(grids, kind, payloads) - vf.vec3_file_bytes(grids[:1], kind, payloads[:1]) == want - 24 - 102 - 23 * (206 if kind else 140) - payloads[0]
    with pytest.raises(ValueError):
        vf.vec3_file_bytes(grids, 2, payloads)
    with pytest.raises(ValueError):
        vf.vec3_file_bytes(grids, kind, [0, 0])
    with pytest.raises(ValueError):
        vf.vec3_file_bytes(grids, kind, [0, -1, 0])
    with pytest.raises(ValueError):
        vf.vec3_file_bytes([], kind, [])
    with pytest.raises(ValueError, match="2\\^63"):
        vf.vec3_file_bytes(grids, 1, [2**62, 2**62, 0])
    if not kind:
        with pytest.raises(ValueError):
            vf.vec3_file_bytes(grids, 0, [0, 8, 0])
    else:
        with pytest.raises(ValueError):
            vf.vec3_file_bytes(grids, 1, None)
    if not have_library():
        return
    sources = [dict(g, leaves=np.zeros((len(g["origins"]), 512, 3), F)) for g in grids]
    assert codec.vec3_file_bytes(sources, kind, payloads if kind else None) == want
    assert codec.vec3_file_bytes(sources, kind, payloads) == want
    lists = [dict(g, leaves=[np.zeros((512, 3), F) for _ in range(len(g["origins"]))]) for g in grids]
    assert codec.vec3_file_bytes(lists, kind, payloads) == want
    with pytest.raises(ValueError, match="payload sizes"):
        codec.vec3_file_bytes(sources, kind, payloads[:2])
    with pytest.raises(ValueError, match="refuse"):
        codec.vec3_file_bytes(sources, kind, [0, -1, 0])
    with pytest.raises(ValueError, match="refuse"):
        codec.vec3_file_bytes(sources, 1 if kind else 0, [2**63 - 1, 0, 0] if kind else [0, 8, 0])
    with pytest.raises(ValueError, match="kind"):
        codec.vec3_file_bytes(sources, 2, payloads)
    if kind:
        with pytest.raises(ValueError, match="needs masks"):
            codec.vec3_file_bytes([{k: v for k, v in g.items() if k != "masks"} for g in sources], 1, payloads)
    # what the writer refuses of the grid list, through the C call
    lib = codec.load_library()
    src, n_g, _keep = codec._vec3_grid_sources(sources, need_masks=bool(kind))
    pb = np.array(payloads, np.int64)
    call = lib.vqhip_vec3_budget_file_bytes
    assert call(src, n_g, kind, pb.ctypes.data) == want
    assert call(None, n_g, kind, pb.ctypes.data) == -1 and call(src, 0, kind, pb.ctypes.data) == -1 and call(src, 256, kind, pb.ctypes.data) == -1
    assert call(src, n_g, 2, pb.ctypes.data) == -1 and call(src, n_g, -1, pb.ctypes.data) == -1
    assert call(src, n_g, kind, None) == (-1 if kind else want)
    for field, value in (("name", None), ("leaf_ptrs", None), ("origins", None), ("n_leaves", -1), ("n_leaves", 1 << 32)) + ((("masks", None),) if kind else ()):
        old = getattr(src[2], field)
        setattr(src[2], field, value)
        assert call(src, n_g, kind, pb.ctypes.data) == -1, field
        setattr(src[2], field, old)
    src[2].n_leaves = (1 << 32) - 1                                  # the pointers are never followed
    assert call(src, n_g, kind, pb.ctypes.data) == want + ((1 << 32) - 1 - 9) * (206 if kind else 140)
    src[2].n_leaves = 9
    assert call(src, n_g, kind, pb.ctypes.data) == want


def test_header_library_and_bindings_hold_exactly_the_five_names():
    assert codec.VEC3_BUDGET_SYMBOLS == NAMES
    raw = open(os.path.join(ROOT, "include", "vqvdb_hip_vec3_budget.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(vqhip_\w+)\s*\(", text))) == sorted(NAMES)
    assert not [n for n in NAMES if n.startswith("vqhip_vec3_compress")]          # tests/test_vec3_bounded_host.py reserves that prefix
    assert all(n.startswith("vqhip_vec3_budget_") for n in NAMES)                  # ... and the older headers' tests reserve theirs
    assert re.search(r'#include\s+"vqvdb_hip_vec3_file.h"', text)
    assert "136 bytes per leaf" in raw                                              # what the file call keeps on the host is said
    for name in NAMES:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert params.count(",") + 1 == ARITY[name], name
    others = [v for k, v in vars(codec).items() if k.endswith("_SYMBOLS") and k != "VEC3_BUDGET_SYMBOLS"]
    assert len(others) >= 12 and codec.VEC3_FILE_SYMBOLS in others and codec.VEC3_ACTIVE_SYMBOLS in others
    assert not any(set(NAMES) & set(o) for o in others)
    for m in ("rate_compress_active", "rate_sweep_file", "compress_file_budget", "check_budget"):
        assert callable(getattr(codec.HipVec3Codec, m)), m
    assert callable(codec.vec3_active_rate_pick) and callable(codec.vec3_file_bytes) and callable(vf.vec3_file_bytes)
    fmt = open(os.path.join(ROOT, "vqvdb_amd", "csrc", "vq_vec3_budget_format.h")).read()
    assert "vqv3f::layout(" in fmt and not re.search(r"\b(206|140|102)\b", re.sub(r"//[^\n]*", "", fmt))   # the layout's constants, not a copy
    if not have_library():
        return
    lib = codec.load_library()
    for name in NAMES:
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == ARITY[name], name
        assert f.restype == (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int), name
    out = subprocess.run(["nm", "-D", "--defined-only", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vqhip_\w+)\b", out))
    assert {n for n in exported if "budget" in n} == set(NAMES)
    assert not {n for n in exported if n.startswith("vqhip_vec3_compress")} - {"vqhip_vec3_compress_bounded"}


def test_a_null_handle_is_refused(tmp_path):
    if not have_library():
        return
    lib = codec.load_library()
    out = tmp_path / "never.vqv3"
    t = np.array([0.5], F)
    used, nbytes = ctypes.c_float(-3.0), ctypes.c_int64(-3)
    assert lib.vqhip_vec3_budget_compress(None, None, None, 1, t.ctypes.data, 1, 0, ctypes.byref(used), None, None, None, None, None, ctypes.byref(nbytes)) == -1
    assert lib.vqhip_vec3_budget_file_sweep(None, None, 1, t.ctypes.data, 1, 0, None) == -1
    assert lib.vqhip_vec3_budget_file_compress(None, os.fspath(out).encode(), None, 1, t.ctypes.data, 1, 0, 0, None, ctypes.byref(used), None,
                                               ctypes.byref(nbytes)) == -1
    assert used.value == -3.0 and nbytes.value == -3 and not out.exists()


def test_wrappers_check_their_arguments_before_any_device():
    V = codec.HipVec3Codec
    assert V.check_budget(0, "b") == 0 and V.check_budget(np.int64(7), "b") == 7 and V.check_budget(2**63 - 1, "b") == 2**63 - 1
    for bad in (-1, 2**63):
        with pytest.raises(ValueError, match="file_budget"):
            V.check_budget(bad, "file_budget")
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError, match="payload_budget"):
            V.check_budget(bad, "payload_budget")
    self = object.__new__(V)                                          # no handle: the checks come first
    try:
        x, m = np.zeros((2, 512, 3), F), np.zeros((2, 8), np.uint64)
        with pytest.raises(ValueError, match="1..64"):
            V.rate_compress_active(self, x, m, [], 5)
        with pytest.raises(ValueError):
            V.rate_compress_active(self, x, m[:1], [0.5], 5)
        with pytest.raises(TypeError, match="payload_budget"):
            V.rate_compress_active(self, x, m, [0.5], 5.0)
        g = {"name": "g", "origins": np.zeros((2, 3), np.int32), "leaves": x}
        with pytest.raises(ValueError, match="needs masks"):
            V.rate_sweep_file(self, [g], [0.5])
        with pytest.raises(ValueError, match="file_budget"):
            V.compress_file_budget(self, "never.vqv3", [dict(g, masks=m)], [0.5], -1)
        with pytest.raises(ValueError, match="tol"):
            V.compress_file_budget(self, "never.vqv3", [dict(g, masks=m)], [-0.5], 10)
    finally:
        self._h = None
