"""The reference helpers of tests/test_gpu_fulltrain_edges.py without a GPU, all in fp64: the per-leaf loss with multiplicities
against torch_ref.training_loss on the batch written out, the forced assignment against the default path, and the number of
candidates the screening keeps."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref  # noqa: E402
from fulltrain_common import NAMES, per_leaf_loss, pick, pool, screen, to_torch, weighted_gradients  # noqa: E402
from vqvdb_amd import synth  # noqa: E402

TOL = 1e-12     # of each tensor's largest value: two fp64 evaluations of the same sums in another order


@pytest.fixture(scope="module")
def W0():
    return synth.make_weights(0)


def autograd(x, W, n_global=None, idx=None):
    """torch_ref.training_loss(...).backward() in fp64, the loss scaled by n / n_global -> (loss, gradients, assignment)."""
    w = to_torch(W, torch.float64, grad=True)
    xs = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).view(-1, 1, 8, 8, 8)
    loss, pieces = torch_ref.training_loss(xs, w, idx=idx)
    (loss * (len(x) / (n_global or len(x)))).backward()
    return float(loss.detach()), {k: w[k].grad.numpy() for k in NAMES}, pieces["idx"]


def assert_same(got, want):
    for k in NAMES:
        top = float(np.abs(want[k]).max())
        assert top > 0.0, k
        assert float(np.abs(got[k] - want[k]).max()) <= TOL * top, k


def test_all_counts_one_is_the_batch_loss(W0):
    x = synth.make_leaves(6, seed=9310)
    loss, g, idx = autograd(x, W0)
    vals, gw = weighted_gradients(x, np.ones(6), 6, W0, idx.numpy(), torch.float64)
    assert abs(vals["loss"] - loss) <= TOL * loss
    assert_same(gw, g)


@pytest.mark.parametrize("n_global", [11, 20])
def test_counts_are_repeated_leaves(W0, n_global):
    x = np.concatenate([synth.make_leaves(3, seed=9311), synth.sparse_leaves(2, seed=9312)])
    counts = np.array([3, 1, 2, 1, 4])
    rows = np.repeat(np.arange(5), counts)[np.random.default_rng(5).permutation(11)]
    loss, g, idx = autograd(x[rows], W0, n_global)
    first = [int(np.flatnonzero(rows == i)[0]) for i in range(5)]
    idx5 = idx.numpy().reshape(11, 64)[first]
    vals, gw = weighted_gradients(x, counts, n_global, W0, idx5, torch.float64)
    assert abs(vals["loss"] - loss) <= TOL * loss
    assert_same(gw, g)


def test_forced_argmin_is_the_default_path(W0):
    x = synth.make_leaves(5, seed=9313)
    loss, g, idx = autograd(x, W0)
    loss_f, g_f, idx_f = autograd(x, W0, idx=idx.clone())
    assert loss_f == loss and torch.equal(idx_f, idx)
    for k in NAMES:
        assert np.array_equal(g_f[k], g[k]), k
    w = to_torch(W0, torch.float64)
    with torch.no_grad():
        per_leaf = per_leaf_loss(x, w, idx.numpy(), torch.float64)
    assert per_leaf.shape == (5,) and abs(float(per_leaf.mean()) - loss) <= TOL * loss


@pytest.mark.parametrize("seed", [0, 1])
def test_the_screening_keeps_enough_of_the_pool(seed):
    cand = pool()
    assert cand.shape == (152, 512)
    keep, idx = screen(cand, synth.make_weights(seed))
    kinds = [int(((keep >= lo) & (keep < hi)).sum()) for lo, hi in ((0, 96), (96, 144), (144, 152))]
    print(f"weight seed {seed}: kept {len(keep)} of 152 (dense {kinds[0]}/96, sparse {kinds[1]}/48, edge {kinds[2]}/8)")
    assert len(keep) >= 65 and idx.shape == (152, 64)
    chosen = pick(keep, 65)
    assert len(set(chosen.tolist())) == 65 and set(chosen.tolist()) <= set(keep.tolist())
    assert (chosen >= 96).any() and (chosen < 96).any()
