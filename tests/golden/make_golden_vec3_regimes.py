#!/usr/bin/env python3
"""Generate tests/golden/golden_vec3_regimes_v1.npz and golden_vec3_regimes_v1_part2.npz by IMPORTING the reference model VQVAE(3, 64, 4096, 0.25)
(python/VQVAE_v2.py EncoderVec3 / DecoderVec3) with each file-free weight regime of tests/vec3_regimes.py loaded strict.

Runs only where a reference checkout and CPU torch are present; the file holds the reference's OUTPUTS only (weights and
leaves are regenerated from numpy).  No reference source is copied.

    python tests/golden/make_golden_vec3_regimes.py [--check]

per regime (seed1, seed2, default_like, deadcodes, wide, saturated), on synth_vec3.make_leaves(24, seed=777) + edge_leaves():
  <regime>/idx     u16 [32,64]    VQVAE.encode
  <regime>/second  u16 [32,64]    the second-nearest code of every position
  <regime>/gap     f32 [32,64]    relative top-2 gap (d2 - d1) / max(|d1|, |z|^2, 1e-30) of every position
  <regime>/rec     f32 [32,512,3] VQVAE.decode of idx
The first file holds seed1, seed2 and default_like, the second deadcodes, wide and saturated: 1.17 MB of decoded float32 voxels
do not fit one committed file of at most 1 MiB.  vec3_regimes.load_fixture() reads both.
--check regenerates everything and compares it bit for bit with the committed files instead of writing them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("VQVDB_REFERENCE_PYTHON", "/root/reference/python"))

import vec3_regimes as vr  # noqa: E402
from vqvdb_amd import synth_vec3  # noqa: E402
from VQVAE_v2 import VQVAE  # noqa: E402  (the reference model, imported, not copied)


def build_model(w):
    torch.manual_seed(0)
    m = VQVAE(3, synth_vec3.D_EMBED, synth_vec3.K_CODES, 0.25).eval()
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd["quantizer.cluster_size"] = torch.ones(synth_vec3.K_CODES)
    sd["quantizer.embed_avg"] = sd["quantizer.embedding"].clone()
    m.load_state_dict(sd, strict=True)
    return m


@torch.no_grad()
def generate():
    torch.set_num_threads(8)
    leaves = vr.fixture_leaves()
    x = torch.from_numpy(leaves).reshape(-1, 8, 8, 8, 3).permute(0, 4, 1, 2, 3).contiguous()
    out = {}
    for name, w in vr.regimes().items():
        m = build_model(w)
        idx = m.encode(x).reshape(-1, 64)
        flat = m.encoder(x).permute(0, 2, 3, 4, 1).reshape(-1, 64)
        e = m.quantizer.embedding
        dist = (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * flat @ e.t()
        top = torch.topk(dist, 2, dim=1, largest=False)
        d1 = dist.gather(1, idx.reshape(-1, 1))[:, 0]
        assert torch.equal(d1, top.values[:, 0]), "VQVAE.encode did not pick a minimum of the distances restated here"
        second = torch.where(top.indices[:, 0] == idx.reshape(-1), top.indices[:, 1], top.indices[:, 0])
        d2 = dist.gather(1, second.reshape(-1, 1))[:, 0]
        scale = torch.maximum(torch.maximum(d1.abs(), (flat ** 2).sum(1)), torch.full_like(d1, 1e-30))
        gap = ((d2 - d1) / scale).reshape(-1, 64)
        rec = m.decode(idx.reshape(-1, 4, 4, 4)).permute(0, 2, 3, 4, 1).reshape(-1, 512, 3)
        out[name + "/idx"] = idx.numpy().astype(np.uint16)
        out[name + "/second"] = second.reshape(-1, 64).numpy().astype(np.uint16)
        out[name + "/gap"] = gap.numpy().astype(np.float32)
        out[name + "/rec"] = rec.numpy().astype(np.float32)
        n_codes = len(np.unique(out[name + "/idx"]))
        print(f"{name}: distinct codes in use {n_codes}; positions with gap < 1e-4: {int((out[name + '/gap'] < 1e-4).sum())}; "
              f"largest |rec| {float(np.abs(out[name + '/rec']).max()):.7f}")
        assert n_codes >= 200, "codebook too collapsed for a meaningful fixture"
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


if __name__ == "__main__":
    data = generate()
    for path, names in vr.FIXTURE_FILES:
        part = {k: v for k, v in data.items() if k.split("/")[0] in names}
        if "--check" in sys.argv:
            ref = np.load(path)
            assert sorted(ref.files) == sorted(part), "fixture keys differ"
            for k, v in part.items():
                assert ref[k].dtype == v.dtype and np.array_equal(ref[k].view(np.uint8), v.view(np.uint8)), f"{k} differs"
            print(f"{os.path.basename(path)} reproduced bit for bit")
        else:
            np.savez_compressed(path, **part)
            print(f"{path}: {os.path.getsize(path)} bytes")
