#!/usr/bin/env python3
"""Generate tests/golden/golden_vec3_v1.npz by IMPORTING the reference model VQVAE(3, 64, 4096, 0.25)
(python/VQVAE_v2.py EncoderVec3 / DecoderVec3) with synth_vec3.make_weights(0) loaded strict.

Runs only where a reference checkout and CPU torch are present; the file holds the reference's OUTPUTS only (inputs are
regenerated from synth_vec3).  No reference source is copied.

    python tests/golden/make_golden_vec3.py [--check]

  idx        u16 [520,64]   VQVAE.encode of synth_vec3.make_leaves(512, 4321) + edge_leaves()
  second     u16 [520,64]   the second-nearest code of every position
  gap        f32 [520,64]   relative top-2 gap (d2 - d1) / max(|d1|, |z|^2, 1e-30) of every position
  rec        f32 [72,512,3] VQVAE.decode of idx[:64] and of the edge leaves' indices
  act_<name> f32 [C, P]     per-layer activations of mixed leaf 0 (encoder) and of decode(idx[0]) (decoder), module outputs
--check regenerates everything and compares it bit for bit with the committed file instead of writing it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("VQVDB_REFERENCE_PYTHON", "/root/reference/python"))

from vqvdb_amd import synth_vec3  # noqa: E402
from VQVAE_v2 import VQVAE  # noqa: E402  (the reference model, imported, not copied)

OUT = os.path.join(HERE, "golden_vec3_v1.npz")
N_MIX, SEED, N_REC = 512, 4321, 64
ACT_LAYERS = ["encoder.pre.0", "encoder.pre.2", "encoder.pre", "encoder.down1", "encoder.res_stack.0", "encoder.res_stack.1",
              "encoder.proj", "decoder.stem.0", "decoder.stem", "decoder.res_stack.0", "decoder.res_stack.1", "decoder.up_conv"]


def build_model():
    torch.manual_seed(0)
    w = synth_vec3.make_weights(0)
    m = VQVAE(3, synth_vec3.D_EMBED, synth_vec3.K_CODES, 0.25).eval()
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd["quantizer.cluster_size"] = torch.ones(synth_vec3.K_CODES)
    sd["quantizer.embed_avg"] = sd["quantizer.embedding"].clone()
    m.load_state_dict(sd, strict=True)
    return m


def to_model(leaves):
    return torch.from_numpy(leaves).reshape(-1, 8, 8, 8, 3).permute(0, 4, 1, 2, 3).contiguous()


@torch.no_grad()
def generate():
    torch.set_num_threads(8)
    m = build_model()
    leaves = np.concatenate([synth_vec3.make_leaves(N_MIX, SEED), synth_vec3.edge_leaves()])
    x = to_model(leaves)
    idx = m.encode(x).reshape(-1, 64)
    z = m.encoder(x)
    flat = z.permute(0, 2, 3, 4, 1).reshape(-1, 64)
    e = m.quantizer.embedding
    dist = (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * flat @ e.t()
    top = torch.topk(dist, 2, dim=1, largest=False)
    d1 = dist.gather(1, idx.reshape(-1, 1))[:, 0]
    assert torch.equal(d1, top.values[:, 0]), "VQVAE.encode did not pick a minimum of the distances restated here"
    second = torch.where(top.indices[:, 0] == idx.reshape(-1), top.indices[:, 1], top.indices[:, 0])
    d2 = dist.gather(1, second.reshape(-1, 1))[:, 0]
    scale = torch.maximum(torch.maximum(d1.abs(), (flat ** 2).sum(1)), torch.full_like(d1, 1e-30))
    gap = ((d2 - d1) / scale).reshape(-1, 64)
    rec_idx = torch.cat([idx[:N_REC], idx[N_MIX:]])
    rec = m.decode(rec_idx.reshape(-1, 4, 4, 4)).permute(0, 2, 3, 4, 1).reshape(-1, 512, 3)

    acts = {}
    hooks = []
    for name, mod in m.named_modules():
        if name in ACT_LAYERS:
            hooks.append(mod.register_forward_hook(lambda _m, _i, o, name=name: acts.__setitem__(name, o[0].detach().clone().reshape(o.shape[1], -1))))
    m.encoder(x[:1])
    m.decode(idx[:1].reshape(-1, 4, 4, 4))
    for h in hooks:
        h.remove()
    out = {"idx": idx.numpy().astype(np.uint16), "second": second.reshape(-1, 64).numpy().astype(np.uint16),
           "gap": gap.numpy().astype(np.float32), "rec": rec.numpy().astype(np.float32)}
    for k in ACT_LAYERS:
        out["act_" + k] = acts[k].numpy().astype(np.float32)
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    n_codes = len(np.unique(out["idx"]))
    print(f"distinct codes in use: {n_codes} of {synth_vec3.K_CODES}; positions with gap < 1e-4: {int((out['gap'] < 1e-4).sum())}")
    assert n_codes >= 200, "synthetic codebook too collapsed for a meaningful fixture"
    return out


if __name__ == "__main__":
    data = generate()
    if "--check" in sys.argv:
        ref = np.load(OUT)
        assert sorted(ref.files) == sorted(data), "fixture keys differ"
        for k, v in data.items():
            assert ref[k].dtype == v.dtype and np.array_equal(ref[k].view(np.uint8), v.view(np.uint8)), f"{k} differs"
        print("golden_vec3_v1.npz reproduced bit for bit")
    else:
        np.savez_compressed(OUT, **data)
        print(f"{OUT}: {os.path.getsize(OUT)} bytes")
