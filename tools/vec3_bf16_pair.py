#!/usr/bin/env python3
"""CPU measurement behind the constants of tests/test_gpu_vec3_bf16.py and tests/test_vec3_bf16_host.py: the four end-to-end
closeness quantities between the two torch restatements (tests/torch_ref_vec3_bf16.py against tests/torch_ref_vec3.py, both
with float64 weights) on the 520 fixture leaves.  No GPU.

    python tools/vec3_bf16_pair.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3 as tr  # noqa: E402
import torch_ref_vec3_bf16 as tb  # noqa: E402
from vqvdb_amd import synth_vec3  # noqa: E402


def pair(leaves, w):
    with torch.no_grad():
        return tb.closeness(leaves, w, lambda x: tb.encode(x, w)[0].numpy(), lambda i: tb.decode(i, w).numpy(),
                            lambda x: tr.encode(x, w)[0].numpy(), lambda i: tr.decode(i, w).numpy())


if __name__ == "__main__":
    w = tr.weights_to_torch(synth_vec3.make_weights(0), torch.float64)
    leaves = np.concatenate([synth_vec3.make_leaves(512, 4321), synth_vec3.edge_leaves()])
    print(json.dumps(pair(leaves, w)))
