"""The helpers of tests/test_gpu_fulltrain_edges.py and tests/test_fulltrain_ref_host.py — TEST INFRASTRUCTURE: the scalar
model's training loss per leaf on top of tests/torch_ref.py, its gradient for a batch given as distinct leaves with
multiplicities, the screening of leaves at which that loss is differentiable with a margin (decided in fp64 alone), and the
device calls of the full-training handle on numpy arrays."""
import numpy as np
import torch
import torch.nn.functional as F

import torch_ref
from vqvdb_amd import synth
from vqvdb_amd.codebook_training import STATS_FLOATS, metrics_from_stats
from vqvdb_amd.full_training import AUX_FLOATS, TRAINABLE
from vqvdb_amd.training_common import recon_metrics

NAMES = [name for name, _ in TRAINABLE]
RELU_MARGIN = 2e-6     # the margin of test_parameter_gradients_against_fp64_autograd
L1_MARGIN = 1e-6       # |recon - x|: the kink of the L1 term
GAP_MARGIN = 1e-5      # (second-best - best) / second-best distance of the code assignment


# ---- the reference ----
def to_torch(W, dtype, grad=False) -> dict:
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=grad and not k.startswith("quantizer.")) for k, v in W.items()}


def _leaves(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).view(-1, 1, 8, 8, 8)


def per_leaf_loss(x, w, idx, dtype):
    """[n]: 0.8 mean_512 (r - x)^2 + 0.2 mean_512 |r - x| + 0.25 mean_(64*128) (z - q)^2 of every leaf, with the assignment idx
    (int64 [n*64], row = leaf * 64 + position) and the straight-through decoder input; w: tensors of `dtype`.  The mean of
    these over the batch is torch_ref.training_loss."""
    x = _leaves(x, dtype)
    n = x.shape[0]
    z = torch_ref.encoder(x, w)
    q = w["quantizer.embedding"][torch.as_tensor(np.asarray(idx, np.int64).reshape(-1))].view(n, 4, 4, 4, z.shape[1]).permute(0, 4, 1, 2, 3)
    r = torch_ref.decoder(z + (q - z).detach(), w)
    d = (r - x).flatten(1)
    return 0.8 * (d * d).mean(1) + 0.2 * d.abs().mean(1) + 0.25 * ((z - q.detach()) ** 2).flatten(1).mean(1)


def weighted_gradients(x, counts, n_global, W, idx, dtype=torch.float64) -> tuple:
    """Autograd of sum_i counts_i L_i / n_global in `dtype` -> ({"loss": the batch's mean loss}, {name: gradient}).  GroupNorm and
    every loss term are per leaf, so this is exactly the gradient of the batch in which leaf i occurs counts_i times, scaled by
    n / n_global (n = sum of the counts)."""
    w = to_torch(W, dtype, grad=True)
    L = per_leaf_loss(x, w, idx, dtype)
    cnt = torch.as_tensor(np.asarray(counts, np.float64)).to(dtype)
    total = (cnt * L).sum()
    (total / n_global).backward()
    return {"loss": float(total.detach() / cnt.sum())}, {k: w[k].grad.numpy() for k in NAMES}


def screen(cand, W) -> tuple:
    """(indices of the kept candidates, the fp64 assignment [len(cand), 64]) at the weights W, from the fp64 forward alone.  A
    leaf is kept if every ReLU input (GroupNorm outputs and the two attention layers) is at least RELU_MARGIN from zero, every
    |recon - x| at least L1_MARGIN, and at all 64 positions the best and the second-best code distance differ by at least
    GAP_MARGIN of the latter."""
    w = to_torch(W, torch.float64)
    real_relu, mins = F.relu, []

    def spy(t, *a, **k):
        mins.append(t.detach().abs().flatten(1).min(1).values)
        return real_relu(t, *a, **k)
    x = _leaves(cand, torch.float64)
    F.relu = spy
    try:
        with torch.no_grad():
            _, pieces = torch_ref.training_loss(x, w)
    finally:
        F.relu = real_relu
    n = x.shape[0]
    relu_min = torch.stack(mins).min(0).values
    diff_min = (pieces["recon"] - x).abs().flatten(1).min(1).values
    flat = pieces["z"].permute(0, 2, 3, 4, 1).reshape(-1, pieces["z"].shape[1])
    e = w["quantizer.embedding"]
    d = (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * flat @ e.t()
    two = torch.topk(d, 2, dim=1, largest=False).values
    gap_min = ((two[:, 1] - two[:, 0]) / two[:, 1]).view(n, 64).min(1).values
    ok = (relu_min >= RELU_MARGIN) & (diff_min >= L1_MARGIN) & (gap_min >= GAP_MARGIN)
    return np.flatnonzero(ok.numpy()), pieces["idx"].numpy().reshape(n, 64)


def pool() -> np.ndarray:
    """The 152 candidates: white noise, leaves shaped like VDB content, the edge leaves."""
    return np.ascontiguousarray(np.concatenate([synth.make_leaves(96, seed=9300), synth.sparse_leaves(48, seed=9301), synth.edge_leaves()]))


def pick(keep, n, seed=9302) -> np.ndarray:
    """n of the kept candidates in a fixed shuffled order of the pool (so every batch size mixes the three kinds); fails rather
    than shrink the batch."""
    assert len(keep) >= n, f"only {len(keep)} candidates pass the screening, {n} are needed"
    order = np.random.default_rng(seed).permutation(152)
    kept = set(int(k) for k in keep)
    return np.array([int(i) for i in order if int(i) in kept][:n])


# ---- the device ----
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_codec(W):
    from vqvdb_amd import weightpack
    from vqvdb_amd.codec import HipCodec
    c = HipCodec(weightpack.dumps(W))
    c.fulltrain_begin()
    return c


def fwdbwd(c, leaves, n_global=None) -> tuple:
    """(flat gradient, aux) of one forward + backward pass."""
    n = len(leaves)
    x = dev(leaves)
    g = torch.zeros(c.fulltrain_param_count(), dtype=torch.float32, device="cuda")
    a = torch.zeros(AUX_FLOATS, dtype=torch.float32, device="cuda")
    c.fulltrain_fwdbwd_device(x.data_ptr(), n, n_global or n, g.data_ptr(), a.data_ptr())
    torch.cuda.synchronize()
    return g.cpu().numpy(), a.cpu().numpy()


def loss_from_aux(aux) -> float:
    """The total loss as FullTrainer.step reads it from the auxiliary sums."""
    aux = np.asarray(aux, np.float64)
    return recon_metrics(aux[STATS_FLOATS:])[2] + metrics_from_stats(aux[:STATS_FLOATS])["vq_loss"]


def split(flat) -> dict:
    out, off = {}, 0
    for name, shape, _ in synth.TENSORS:
        if name.startswith("quantizer."):
            continue
        size = int(np.prod(shape))
        out[name] = flat[off:off + size]
        off += size
    assert off == len(flat)
    return out


def handle_idx(c, leaves) -> np.ndarray:
    """The training forward's assignment [n, 64]: the rows it gathered (t_q) matched to the rows of the handle's codebook bit for
    bit."""
    n = len(leaves)
    x = dev(leaves)
    c.fulltrain_forward_device(x.data_ptr(), n)
    torch.cuda.synchronize()
    E = c.train_get_state()["embedding"]
    row_of = {E[k].tobytes(): k for k in range(len(E))}
    assert len(row_of) == len(E), "two codebook rows are equal"
    rows = np.ascontiguousarray(c.fetch("t_q", n, 128, 64).transpose(0, 2, 1)).reshape(-1, 128)
    return np.array([row_of[r.tobytes()] for r in rows], dtype=np.int64).reshape(n, 64)
