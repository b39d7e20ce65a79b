"""Which launches a call makes, at the sizes where the launch code of vq_runtime.hip changes its choice.

A plan is the list of (name, launches) pairs that profile_read() returns after ONE call on a fresh handle (so that no earlier call
can have changed the choice), compared with tests/golden/launch_plan.json.  The fixture was recorded with

    python tests/test_gpu_launch_plan.py --record > tests/golden/launch_plan.json

on an MI355X at the commit before the encoder and the decoder became one list of layer stages each; it stores the compute_units()
it was recorded with, and a device with another count fails here (the nt >= n_cus choice of the decoder front depends on it).

Sizes in leaves, each the last before a selection flips and the first after it:
  encode  1 | 64 | 1024, 1056: cout-split x2 kernels | 8160, 8192: nt >= 256, first conv twice and 8 tiles per VQ workgroup |
          51200, 51232: position-split path / one wave per tile
  decode  64 | 1536, 1568: tail16_tiles | 2048, 2080: cout-split x4 kernels, sixteen-wave small front | 8160, 8192: nt >= n_cus,
          the front on stem_taps_k | 55296, 55328: position-split path / one wave per tile
  65 leaves with the small-batch policy off under every environment of test_gpu_parity.py::test_large_path_kernel_variants_agree;
  decode of 64 and 2080 leaves under VQHIP_STEM_SMALL=split, VQHIP_R64S=stream, VQHIP_TAIL16_TILES=0 and the three together;
  bf16 encode and bf16 decode at 64 and 55328 leaves;
  train_vq_stats_device at 224, 256 (8 tiles) and 32768 leaves (1024 tiles): the limits of the latent assignment;
  fulltrain_fwdbwd_device at 64 leaves, the names up to train_latent_assign.

The last test is about what a call leaves behind on the handle: a plain encode after a full-training forward gives the bits of a
fresh handle's and does not touch the training latents."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vqvdb_amd import synth, weightpack  # noqa: E402
from vqvdb_amd.codebook_training import STATS_FLOATS  # noqa: E402
from vqvdb_amd.codec import HipCodec  # noqa: E402
from vqvdb_amd.full_training import AUX_FLOATS  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_plan.json")
SWITCHES = ("VQHIP_CONV8", "VQHIP_STEM", "VQHIP_CONV4", "VQHIP_DOWN", "VQHIP_FIRST", "VQHIP_TAIL", "VQHIP_FIRST_SRC", "VQHIP_STEM_SMALL",
            "VQHIP_R64S", "VQHIP_TAIL16_TILES")
LARGE_PATH_ENVS = ({}, {"VQHIP_CONV8": "w8"}, {"VQHIP_CONV8": "rows"}, {"VQHIP_STEM": "split"}, {"VQHIP_STEM": "gather"}, {"VQHIP_FIRST": "steps"},
                   {"VQHIP_FIRST": "roll0"}, {"VQHIP_CONV4": "rows"}, {"VQHIP_DOWN": "rows"}, {"VQHIP_CONV4": "rows", "VQHIP_DOWN": "rows"},
                   {"VQHIP_TAIL": "slab"}, {"VQHIP_TAIL": "groups"}, {"VQHIP_TAIL": "rows32"}, {"VQHIP_FIRST_SRC": "raw"},
                   {"VQHIP_FIRST_SRC": "raw", "VQHIP_FIRST": "roll0"})
SMALL_PATH_ENVS = ({"VQHIP_STEM_SMALL": "split"}, {"VQHIP_R64S": "stream"}, {"VQHIP_TAIL16_TILES": "0"},
                   {"VQHIP_STEM_SMALL": "split", "VQHIP_R64S": "stream", "VQHIP_TAIL16_TILES": "0"})
N_MAX = 55328

# (call, leaves, small-batch policy, environment)
CASES = [("encode", n, -1, {}) for n in (1, 64, 1024, 1056, 8160, 8192, 51200, 51232)]
CASES += [("decode", n, -1, {}) for n in (64, 1536, 1568, 2048, 2080, 8160, 8192, 55296, 55328)]
CASES += [("both", 65, 0, env) for env in LARGE_PATH_ENVS]
CASES += [("decode", n, -1, env) for env in SMALL_PATH_ENVS for n in (64, 2080)]
CASES += [(call, n, -1, {}) for call in ("encode_bf16", "decode_bf16") for n in (64, 55328)]
CASES += [("train_vq_stats", n, -1, {}) for n in (224, 256, 32768)]
CASES += [("fulltrain_fwdbwd", 64, -1, {})]


def case_id(call, n, tiles, env):
    return f"{call}-{n}" + ("-nosplit" if tiles == 0 else "") + "".join(f"-{k[6:]}={v}" for k, v in env.items())


@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def device_inputs():
    g = torch.Generator(device="cuda").manual_seed(4100)
    leaves = torch.rand(N_MAX, 512, device="cuda", generator=g)
    idx = torch.randint(0, 256, (N_MAX, 64), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    return leaves, idx


def plan(pack, inputs, call, n, tiles, env):
    """[[name, launches], ...] of one call on a fresh handle."""
    leaves, idx = inputs
    with environment(env):
        c = HipCodec(pack, encode_precision="bf16" if call == "encode_bf16" else "fp32", decode_precision="bf16" if call == "decode_bf16" else "fp32")
    try:
        c.set_small_batch_tiles(tiles)
        if call == "train_vq_stats":
            c.train_begin()
        if call == "fulltrain_fwdbwd":
            c.fulltrain_begin()
        torch.cuda.synchronize()
        c.profile_enable(True)
        if call in ("encode", "encode_bf16", "both"):
            out = torch.empty(n, 64, dtype=torch.uint8, device="cuda")
            c.encode_device(leaves.data_ptr(), n, out.data_ptr())
        if call in ("decode", "decode_bf16", "both"):
            out = torch.empty(n, 512, device="cuda")
            c.decode_device(idx.data_ptr(), n, out.data_ptr())
        if call == "train_vq_stats":
            stats = torch.zeros(STATS_FLOATS, device="cuda")
            c.train_vq_stats_device(leaves.data_ptr(), n, stats.data_ptr())
        if call == "fulltrain_fwdbwd":
            grads = torch.zeros(c.fulltrain_param_count(), device="cuda")
            aux = torch.zeros(AUX_FLOATS, device="cuda")
            c.fulltrain_fwdbwd_device(leaves.data_ptr(), n, n, grads.data_ptr(), aux.data_ptr())
        torch.cuda.synchronize()
        got = [[s["name"], s["launches"]] for s in c.profile_read()]
    finally:
        c.close()
    if call == "fulltrain_fwdbwd":
        names = [name for name, _ in got]
        got = got[:names.index("train_latent_assign") + 1]
    return got


@pytest.fixture(scope="module")
def pack(weights):
    return weightpack.dumps(weights)


@pytest.fixture(scope="module")
def inputs():
    return device_inputs()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_compute_units_are_those_of_the_recording(pack, recorded):
    c = HipCodec(pack)
    try:
        assert list(c.compute_units()) == recorded["compute_units"]
    finally:
        c.close()


@pytest.mark.parametrize("call,n,tiles,env", CASES, ids=[case_id(*case) for case in CASES])
def test_launch_plan(pack, inputs, recorded, call, n, tiles, env):
    got = plan(pack, inputs, call, n, tiles, env)
    print(got)
    assert got == recorded["cases"][case_id(call, n, tiles, env)]


def test_plain_encode_after_a_training_forward(pack, inputs):
    """The training forward hands its extra outputs to the encoder as arguments: nothing of them stays on the handle."""
    leaves = inputs[0]
    idx = torch.empty(51232, 64, dtype=torch.uint8, device="cuda")

    def encode(c, n):
        idx.zero_()
        c.encode_device(leaves.data_ptr(), n, idx.data_ptr())
        torch.cuda.synchronize()
        return idx[:n].cpu().numpy()

    fresh = HipCodec(pack)
    try:
        want = {n: encode(fresh, n) for n in (64, 51232)}
    finally:
        fresh.close()
    c = HipCodec(pack)
    try:
        c.fulltrain_begin()
        c.fulltrain_forward_device(leaves.data_ptr(), 64)
        torch.cuda.synchronize()
        latent = c.fetch("t_z", 64, 128, 64)
        assert np.isfinite(latent).all() and np.abs(latent).max() > 0.0
        for n in (64, 51232):
            assert np.array_equal(encode(c, n), want[n]), n
        assert np.array_equal(c.fetch("t_z", 64, 128, 64).view(np.uint32), latent.view(np.uint32))
    finally:
        c.close()


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    the_pack = weightpack.dumps(synth.make_weights(seed=0))
    the_inputs = device_inputs()
    handle = HipCodec(the_pack)
    units = list(handle.compute_units())
    handle.close()
    cases = {case_id(*case): plan(the_pack, the_inputs, *case) for case in CASES}
    print(json.dumps({"compute_units": units, "cases": cases}, indent=1))
