"""The handles' lazily grown buffers on the GPU (vqvdb_amd/csrc/vq_buffers.h): a handle that has seen batches of 32,
96, 32 and 160 leaves returns at every size, byte for byte, what a fresh handle given only that size returns, for every call family;
families interleave on one handle; the training buffers grow from 32 to 96 leaves; and twenty create / exercise / destroy rounds in
a child process lose no device memory (profiles/buffers_leak.json has the parent commit's drift of the same loop).

Both handles cut a call into chunks and size their buffers per chunk, and a chunk is a multiple of 32 leaves.  A chunk of 32 would
make every chunk 32 leaves and nothing would ever be replaced, so the cases run at two chunks: 64 (the calls see chunks of 32, then
64 + 32, then 32, then 64 + 64 + 32: one regrow, then multi-chunk loops over grown buffers that hold a smaller last chunk) and 256
(one chunk per call of 32, 96, 32, 160 leaves: two regrows with a smaller call between them).  PEAKS states that arithmetic, and
the scalar handle's workspace_bytes() must rise exactly where it says (the Vec3 handle has no such accessor).  A training batch may
not exceed the chunk, so the training cases keep the default chunk."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from vqvdb_amd import full_training, synth, synth_vec3, weightpack  # noqa: E402
from vqvdb_amd.codec import HipCodec, HipVec3Codec, pack_masks  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (32, 96, 32, 160)
CHUNKS = (64, 256)
LEAK_CHUNK = 32   # the leak loop only counts bytes: the chunk at which profiles/buffers_leak.json measured the parent
NMAX = max(SIZES)
# the largest chunk a handle has been given up to and including each step: where it rises, buffers are replaced by larger ones
PEAKS = {chunk: [max(min(n, chunk) for n in SIZES[:k + 1]) for k in range(len(SIZES))] for chunk in CHUNKS}
assert PEAKS == {64: [32, 64, 64, 64], 256: [32, 96, 96, 160]}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Model:
    """One handle type: how to make it, its leaves (with masks for Vec3), and tolerances around the median leaf error."""

    def __init__(self, name):
        self.name = name
        if name == "scalar":
            self.pack = weightpack.dumps(synth.make_weights(0))
            self.leaves = np.ascontiguousarray(synth.make_leaves(NMAX, seed=2201))
            self.idx_t, self.leaf_shape = torch.uint8, (512,)
        else:
            self.pack = weightpack.dumps(synth_vec3.make_weights(0))
            self.leaves = np.ascontiguousarray(synth_vec3.make_leaves(NMAX, 2201))
            self.idx_t, self.leaf_shape = torch.int16, (512, 3)
            self.masks = pack_masks(np.random.default_rng(5).random((NMAX, 512)) < 0.5)
        c = self.new()
        err = c.roundtrip(self.leaves)[1]
        c.close()
        self.tol = float(np.float32(np.median(err[:, 0])))
        self.tols = [2 * self.tol, self.tol, self.tol / 2]
        self.fresh = {}   # (mode, chunk, family, n) -> what a fresh handle returns: computed once, shared by the cases

    def new(self, mode="fp32", chunk=CHUNKS[0]):
        c = HipCodec(self.pack) if self.name == "scalar" else HipVec3Codec(self.pack, precision=mode)
        if chunk:
            c.set_chunk_leaves(chunk)
        return c


@pytest.fixture(scope="module")
def models():
    return {name: Model(name) for name in ("scalar", "vec3")}


# ---- the call families: (model, codec, n) -> tuple of numpy arrays ----
def last_chunk(c, n):
    chunk = c.chunk_leaves()
    return n - (n - 1) // chunk * chunk


def fam_encode_decode(m, c, n):
    idx = c.encode(m.leaves[:n])
    return idx, c.decode(idx)


def fam_device(m, c, n):
    s = torch.cuda.Stream()
    x = torch.from_numpy(m.leaves[:n]).cuda()
    idx = torch.zeros((n, 64), dtype=m.idx_t, device="cuda")
    out = torch.zeros((n,) + m.leaf_shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    c.encode_device(x.data_ptr(), n, idx.data_ptr(), s.cuda_stream)
    c.decode_device(idx.data_ptr(), n, out.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), out.cpu().numpy()


def fam_roundtrip(m, c, n):
    return tuple(c.roundtrip(m.leaves[:n], return_recon=True))


def fam_bounded(m, c, n):
    idx, ids, raw, err = c.compress_bounded(m.leaves[:n], m.tol, return_leaf_err=True)
    return idx, ids, raw, err, c.decompress_bounded(idx, ids, raw)


def fam_residual(m, c, n):
    idx, code, payload, err = c.compress_residual(m.leaves[:n], m.tol, return_leaf_err=True)
    return idx, code, payload, err, c.decompress_residual(idx, m.tol, code, payload)


def fam_rate_sweep(m, c, n):
    return (c.rate_sweep(m.leaves[:n], m.tols),)


def fam_rate_compress(m, c, n):
    used, hist, idx, code, payload, err = c.rate_compress(m.leaves[:n], m.tols, n * 3072, return_leaf_err=True)
    return np.float32(used), hist, idx, code, payload, err


def fam_residual_masked(m, c, n):
    idx, code, payload, err = c.compress_residual_masked(m.leaves[:n], m.masks[:n], m.tol, return_leaf_err=True)
    return idx, code, payload, err, c.decompress_residual(idx, m.tol, code, payload)


def fam_rate_sweep_masked(m, c, n):
    return (c.rate_sweep_masked(m.leaves[:n], m.masks[:n], m.tols),)


def fam_debug(m, c, n):
    """The debug copies (one buffer per layer, sized to the largest chunk kept so far) of the last chunk of an encode and a decode."""
    c.debug_enable(True)
    try:
        c.decode(c.encode(m.leaves[:n]))
        return tuple(c.debug_fetch(k, last_chunk(c, n)) for k in ("encoder.pre.0", "encoder.down1", "encoder.proj", "decoder.stem", "decoder.up_conv"))
    finally:
        c.debug_enable(False)


BOTH = (fam_encode_decode, fam_device, fam_roundtrip, fam_bounded, fam_residual, fam_rate_sweep)
VEC3_ONLY = (fam_rate_compress, fam_residual_masked, fam_rate_sweep_masked, fam_debug)
CASES = [(name, mode, chunk, f) for chunk in CHUNKS for name, mode, fams in
         (("scalar", "fp32", BOTH), ("vec3", "fp32", BOTH + VEC3_ONLY), ("vec3", "bf16", BOTH + VEC3_ONLY)) for f in fams]


def fresh_result(m, mode, chunk, fam, n):
    key = (mode, chunk, fam.__name__, n)
    if key not in m.fresh:
        c = m.new(mode, chunk)
        try:
            m.fresh[key] = fam(m, c, n)
        finally:
            c.close()
    return m.fresh[key]


@pytest.mark.parametrize("name,mode,chunk,fam", CASES, ids=[f"{a}-{b}-chunk{ch}-{f.__name__[4:]}" for a, b, ch, f in CASES])
def test_grow_shrink_grow_matches_a_fresh_handle(models, name, mode, chunk, fam):
    m = models[name]
    c = m.new(mode, chunk)
    assert c.chunk_leaves() == chunk   # (the handle may lower a chunk that does not fit the free memory: PEAKS would not hold)
    held = []
    try:
        for step, n in enumerate(SIZES):
            got, want = fam(m, c, n), fresh_result(m, mode, chunk, fam, n)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert same(g, w), (step, n, k)
            if name == "scalar":   # the workspace was replaced by a larger one exactly where the peak chunk rose, and kept elsewhere
                held.append(c.workspace_bytes())
                assert held[0] > 0
                if step:
                    assert (held[step] > held[step - 1]) == (PEAKS[chunk][step] > PEAKS[chunk][step - 1]), (step, held)
                    assert held[step] >= held[step - 1], (step, held)
    finally:
        c.close()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", ["scalar", "vec3"])
def test_interleaved_families_on_one_handle(models, name, chunk):
    """A residual compress at 160 leaves, a plain encode at 32, a size sweep at 96, the residual compress again: at chunk 256 the
    sweep's buffers grow between two users of the residual set, and the encode and the sweep see buffers larger than they need."""
    m = models[name]
    c = m.new("fp32", chunk)
    try:
        first = fam_residual(m, c, 160)
        idx = c.encode(m.leaves[:32])
        hist = c.rate_sweep(m.leaves[:96], m.tols)
        last = fam_residual(m, c, 160)
        for k, (a, b) in enumerate(zip(first, last)):
            assert same(a, b), k
        assert same(idx, fresh_result(m, "fp32", chunk, fam_encode_decode, 32)[0])
        assert same(hist, fresh_result(m, "fp32", chunk, fam_rate_sweep, 96)[0])
    finally:
        c.close()


# ---- training buffers: one statistics call and one forward / backward at 32 leaves, then at 96, against a fresh handle at 96 ----
def train_scalar(m, c, n):
    x = torch.from_numpy(m.leaves[:n]).cuda()
    st = torch.zeros(full_training.STATS_FLOATS, device="cuda")
    torch.cuda.synchronize()
    c.train_vq_stats_device(x.data_ptr(), n, st.data_ptr())   # the handle's own latent and index scratch
    g = torch.zeros(c.fulltrain_param_count(), device="cuda")
    aux = torch.zeros(full_training.AUX_FLOATS, device="cuda")
    torch.cuda.synchronize()
    c.fulltrain_fwdbwd_device(x.data_ptr(), n, n, g.data_ptr(), aux.data_ptr())
    torch.cuda.synchronize()
    return st.cpu().numpy(), g.cpu().numpy(), aux.cpu().numpy()


def train_vec3(m, c, n):
    x = torch.from_numpy(m.leaves[:n]).cuda()
    st = torch.zeros(c.train_stats_floats(), device="cuda")
    torch.cuda.synchronize()
    c.train_vq_stats_device(x.data_ptr(), n, st.data_ptr())
    g = torch.zeros(c.fulltrain_param_count(), device="cuda")
    aux = torch.zeros(c.fulltrain_aux_floats(), device="cuda")
    torch.cuda.synchronize()
    c.fulltrain_fwdbwd_device(x.data_ptr(), n, n, g.data_ptr(), aux.data_ptr())
    torch.cuda.synchronize()
    return st.cpu().numpy(), g.cpu().numpy(), aux.cpu().numpy()


@pytest.mark.parametrize("name", ["scalar", "vec3"])
def test_training_buffers_grow(models, name):
    m = models[name]
    run = train_scalar if name == "scalar" else train_vec3

    def handle():
        c = m.new(chunk=0)
        c.train_begin()
        c.fulltrain_begin()
        return c

    grown, fresh = handle(), handle()
    try:
        run(m, grown, 32)
        got, want = run(m, grown, 96), run(m, fresh, 96)
        for k, (g, w) in enumerate(zip(got, want)):
            assert same(g, w), k
    finally:
        grown.close()
        fresh.close()


# ---- no leak: twenty create / exercise / destroy rounds in a child process ----
LEAK_SCRIPT = r"""
import json, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
import torch
import test_gpu_buffers as t
ms = {{name: t.Model(name) for name in ("scalar", "vec3")}}
free = []
for r in range(20):
    for name, m in ms.items():
        c = m.new(chunk=t.LEAK_CHUNK)
        for fam in t.BOTH + (t.VEC3_ONLY if name == "vec3" else ()):
            fam(m, c, 96)
        c.close()
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info()[0])
c = ms["scalar"].new(chunk=t.LEAK_CHUNK)
c.encode(ms["scalar"].leaves[:32])
ws32 = c.workspace_bytes()
c.close()
print(json.dumps({{"free_after_first": free[0], "free_after_twentieth": free[-1], "drift_bytes": free[0] - free[-1], "workspace_32_leaves": ws32}}))
"""


def test_twenty_handles_leak_no_device_memory(tmp_path):
    """hipMemGetInfo's free memory after the first destroy and after the twentieth.  The parent commit's drift over the same loop is in
    profiles/buffers_leak.json (measured on one MI355X); this change's drift may exceed it by at most one 32-leaf workspace."""
    script = tmp_path / "leak.py"
    script.write_text(LEAK_SCRIPT.format(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print("leak loop:", got)
    parent = json.load(open(os.path.join(ROOT, "profiles", "buffers_leak.json")))["parent"]["drift_bytes"]
    assert got["drift_bytes"] <= parent + got["workspace_32_leaves"], (got, parent)
