"""The helpers of tests/test_gpu_vec3_fulltrain.py and tests/test_gpu_vec3_fulltrain_edges.py — TEST INFRASTRUCTURE: a handle in
full-training mode, the device calls of include/vqvdb_hip_vec3_fulltrain.h on numpy arrays, the flat vector split into its 60
tensors, and the screening of leaves at which the loss is differentiable with a margin."""
import numpy as np
import torch

import torch_ref_vec3 as tr
import torch_ref_vec3_fulltrain as tf
from vqvdb_amd import vec3_full_training, weightpack
from vqvdb_amd.codec import HipVec3Codec


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_codec(W):
    c = HipVec3Codec(weightpack.dumps(W))
    c.fulltrain_begin()
    return c


def fwdbwd(c, leaves, n_global=None, stream=0):
    n = len(leaves)
    x = dev(leaves)
    g = torch.zeros(c.fulltrain_param_count(), dtype=torch.float32, device="cuda")
    a = torch.zeros(c.fulltrain_aux_floats(), dtype=torch.float32, device="cuda")
    c.fulltrain_fwdbwd_device(x.data_ptr(), n, n_global or n, g.data_ptr(), a.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return g.cpu().numpy(), a.cpu().numpy()


def forward(c, leaves):
    n = len(leaves)
    x = dev(leaves)
    idx = torch.zeros((n, 64), dtype=torch.int16, device="cuda")
    rec = torch.zeros((n, 512, 3), dtype=torch.float32, device="cuda")
    c.fulltrain_forward_device(x.data_ptr(), n, idx.data_ptr(), rec.data_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(np.uint16), rec.cpu().numpy()


def split(vec):
    out, off = {}, 0
    for name, shape in vec3_full_training.PARAM_SPECS:
        size = int(np.prod(shape))
        out[name] = vec[off:off + size]
        off += size
    return out


def _screen(leaves, W, idx, n_keep=32):
    """Indices of all leaves whose ReLU inputs are all >= 2e-6 from zero and whose |recon - x| are all >= 1e-6 (fp64) at the
    weights W with the assignment idx; at least n_keep must pass."""
    w = tr.weights_to_torch(W)
    mins = []
    orig = tr._gn_relu

    def rec_gn(x, ww, prefix, eps=1e-5):
        pre = torch.nn.functional.group_norm(x, 8, ww[prefix + ".weight"], ww[prefix + ".bias"], eps=eps)
        mins.append(pre.abs().flatten(1).min(1).values)
        return torch.relu(pre)

    tr._gn_relu = rec_gn
    try:
        with torch.no_grad():
            e = w["quantizer.embedding"]
            out = tf.loss(leaves, w, e, torch.as_tensor(idx.reshape(-1).astype(np.int64)))
    finally:
        tr._gn_relu = orig
    relu_min = torch.stack(mins).min(0).values.numpy()
    x = np.asarray(leaves, np.float64).reshape(len(leaves), -1)
    diff_min = np.abs(out["rec"].numpy().reshape(len(leaves), -1) - x).min(1)
    ok = np.where((relu_min >= 2e-6) & (diff_min >= 1e-6))[0]
    assert len(ok) >= n_keep, f"only {len(ok)} of {len(leaves)} leaves pass the screening"
    return ok
