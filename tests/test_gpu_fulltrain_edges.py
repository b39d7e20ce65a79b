"""Scalar full training at its edges: all 44 parameter gradients and the loss against fp64 autograd where the launch code of
vq_train_full.inc changes shape with the batch — one ragged tile (1, 7, 31 leaves), a tile of one leaf behind full ones (33,
65), two tiles per weight-gradient group (1025), two planes per workgroup and the shared reduction stream (2049) — on a handle
whose buffers hold an earlier, larger batch, with n_global != n, with the unfolded tail, with the fallback weight-gradient
family, at weights that reached the handle through set_params and through apply (with the EMA moving the codebook), after a
batch with NaN and Inf leaves, and through the overlap entry point.

The inputs are chosen by the fp64 reference alone (fulltrain_common.screen) and the handle's code assignment must equal the
fp64 argmin on every leaf.  Bars: 5e-6 of each tensor's largest fp64 gradient (GRAD_VS_FP64 of test_gpu_fulltrain.py); a tensor
whose gradient PyTorch's own fp32 autograd misses by more than 2.5e-6 gets twice that error.  The loss: 2e-5 relative.

Measured on the MI355X (worst GPU error / torch fp32's worst error / widened bars; loss error 1.7e-9 .. 3.1e-8):
  1 leaf                9.23e-7 / 8.21e-7 / none        7 leaves              7.74e-7 / 1.07e-6 / none
  31 leaves             5.21e-7 / 1.81e-6 / none        33 leaves             4.90e-7 / 1.61e-6 / none
  65 leaves             5.29e-7 / 1.82e-6 / none        33, n_global 80       3.14e-7 / 1.61e-6 / none
  1, unfolded tail      9.87e-7 / 8.21e-7 / none        33, unfolded tail     5.66e-7 / 1.61e-6 / none
  1025 leaves           6.53e-7 / 1.03e-5 / 18 of 44 tensors, largest encoder.pre.3.conv1.bias 2.06e-5
  2049 leaves           9.51e-7 / 3.57e-5 / 28 of 44 tensors, largest encoder.pre.3.conv1.bias 7.13e-5
  1025, pair kernels    2.23e-6 / 1.03e-5 / the same 18
  set_params            4.52e-7 / 1.53e-6 / none        apply                 1.17e-6 / 1.57e-6 / none
No GPU error reaches the unwidened bar: the widened bars are torch's fp32 sums over the whole batch.  The 33-leaf gradient and aux
are the bits of a fresh handle after the 96-leaf batch, after the NaN / Inf batch and through the overlap entry point.  No bug found.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fulltrain_common import (NAMES, dev, fwdbwd, handle_idx, loss_from_aux, new_codec, pick, pool, screen, split,  # noqa: E402
                              weighted_gradients)
from vqvdb_amd import synth  # noqa: E402
from vqvdb_amd.full_training import AUX_FLOATS, dict_to_flat, flat_to_dict  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 5e-6                 # GRAD_VS_FP64: of the tensor's largest fp64 gradient
LOSS_BAR = 2e-5            # relative, the bar of test_five_steps_against_the_references_own_optimizer_loop
N_DISTINCT = 65            # coprime to the 32 leaves of a tile: every tile of a tiled batch holds another set
RAGGED = (1, 7, 31, 33, 65)
LR_APPLY = 2e-3
U = 2.0 ** -24             # unit roundoff of float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_gradients(label, g, g64, g32, factor=1.0):
    """Every tensor of the flat gradient g against factor * g64, relative to that tensor's largest value.  The bar is BAR; on a
    tensor where torch's own fp32 gradient is more than BAR / 2 from fp64 it is max(BAR, twice that error), since two fp32 sums in
    different orders may differ from each other by as much as each differs from fp64.  No bar comes from the GPU's number."""
    gpu = split(g)
    worst, worst32, widened, failed = 0.0, 0.0, [], []
    for k in NAMES:
        ref = g64[k].reshape(-1) * factor
        top = float(np.abs(ref).max())
        assert top > 0.0, f"{label} {k}: the fp64 gradient is all zero"
        err = float(np.abs(gpu[k] - ref).max()) / top
        err32 = float(np.abs(g32[k].reshape(-1).astype(np.float64) * factor - ref).max()) / top
        bar = max(BAR, 2.0 * err32) if err32 > BAR / 2 else BAR
        print(f"{label} {k:36s} gpu {err:.2e}  torch fp32 {err32:.2e}  bar {bar:.2e}")
        worst, worst32 = max(worst, err), max(worst32, err32)
        if bar > BAR:
            widened.append((k, f"{bar:.1e}"))
        if not err < bar:
            failed.append((k, err, bar))
    print(f"{label}: worst parameter-gradient error {worst:.2e}, torch fp32's worst {worst32:.2e}, widened bars: {widened}")
    assert not failed, (label, failed)


def check_loss(label, aux, vals):
    got = loss_from_aux(aux)
    print(f"{label}: loss {got:.9g}, fp64 {vals['loss']:.9g}, relative error {abs(got - vals['loss']) / vals['loss']:.2e}")
    assert abs(got - vals["loss"]) < LOSS_BAR * vals["loss"], (label, got, vals["loss"])


def references(leaves, counts, W, idx, materialised=None):
    """fp64 autograd of the weighted batch, and torch's fp32 autograd of the same batch (written out, if given) -> (vals, g64, g32)"""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n = int(np.sum(counts))
    vals, g64 = weighted_gradients(leaves, counts, n, W, idx, torch.float64)
    if materialised is None:
        _, g32 = weighted_gradients(leaves, counts, n, W, idx, torch.float32)
    else:
        rows = materialised
        _, g32 = weighted_gradients(leaves[rows], np.ones(len(rows)), n, W, idx[rows], torch.float32)
    return vals, g64, g32


@pytest.fixture(scope="module")
def W0():
    return synth.make_weights(0)


@pytest.fixture(scope="module")
def cand():
    return pool()


# ---- a, b, c: the created weights ----
@pytest.fixture(scope="module")
def created(W0, cand):
    """One handle at the weights it was created with, after a 96-leaf batch; the 65 screened leaves with their fp64 assignment,
    which the handle must reproduce; the references by batch size (computed once)."""
    keep, idx64 = screen(cand, W0)
    chosen = pick(keep, N_DISTINCT)
    c = new_codec(W0)
    state = {"c": c, "leaves": np.ascontiguousarray(cand[chosen]), "idx": idx64[chosen], "ref": {}}
    fwdbwd(c, cand[:96])       # every buffer past the batches below holds this batch's values, not fresh memory
    assert np.array_equal(handle_idx(c, state["leaves"]), state["idx"]), "the handle's assignment is not the fp64 argmin"
    yield state
    c.close()


def tiling(n):
    """Row j of the n-leaf batch is screened leaf PERM[j % 65]."""
    perm = np.random.default_rng(9303).permutation(N_DISTINCT)
    return perm[np.arange(n) % N_DISTINCT]


def ref_created(created, W0, n):
    if n not in created["ref"]:
        if n <= N_DISTINCT:
            created["ref"][n] = references(created["leaves"][:n], np.ones(n), W0, created["idx"][:n])
        else:
            rows = tiling(n)
            created["ref"][n] = references(created["leaves"], np.bincount(rows, minlength=N_DISTINCT), W0, created["idx"], materialised=rows)
    return created["ref"][n]


@pytest.fixture(scope="module")
def fresh33(W0, created):
    """The 33-leaf batch on a handle that has run nothing else."""
    c = new_codec(W0)
    g, aux = fwdbwd(c, created["leaves"][:33])
    c.close()
    assert np.isfinite(g).all() and np.isfinite(aux).all()
    return g, aux


@pytest.mark.parametrize("n", RAGGED)
def test_gradients_at_ragged_batch_sizes(created, fresh33, W0, n):
    c, leaves = created["c"], np.ascontiguousarray(created["leaves"][:n])
    g, aux = fwdbwd(c, leaves)
    vals, g64, g32 = ref_created(created, W0, n)
    check_gradients(f"n={n}", g, g64, g32)
    check_loss(f"n={n}", aux, vals)
    if n == 33:
        assert np.array_equal(bits(g), bits(fresh33[0])), "what an earlier, larger batch left in the buffers changed the gradient"
        assert np.array_equal(bits(aux), bits(fresh33[1]))


@pytest.mark.parametrize("n", (1, 33))
def test_gradients_with_the_unfolded_tail(created, W0, n):
    c, leaves = created["c"], np.ascontiguousarray(created["leaves"][:n])
    c.fulltrain_set_folded_tail(False)
    try:
        g, aux = fwdbwd(c, leaves)
    finally:
        c.fulltrain_set_folded_tail(True)
    vals, g64, g32 = ref_created(created, W0, n)
    check_gradients(f"unfolded n={n}", g, g64, g32)
    check_loss(f"unfolded n={n}", aux, vals)


def test_gradients_with_a_larger_global_batch(created, W0):
    """n_global = 80 on 33 leaves: every term of the loss is a mean over leaves and GroupNorm is per leaf, so the gradient is the
    33-leaf mean loss's times 33 / 80 exactly."""
    n, n_global = 33, 80
    g, _ = fwdbwd(created["c"], np.ascontiguousarray(created["leaves"][:n]), n_global)
    _, g64, g32 = ref_created(created, W0, n)
    check_gradients(f"n={n} n_global={n_global}", g, g64, g32, factor=n / n_global)


def tiled_batch(created, n):
    rows = tiling(n)
    counts = np.bincount(rows, minlength=N_DISTINCT)
    assert counts.min() >= 1 and len({tuple(sorted(rows[t:t + 32])) for t in range(0, n - 31, 32)}) == n // 32
    return np.ascontiguousarray(created["leaves"][rows]), rows


@pytest.mark.parametrize("n", (1025, 2049))
def test_gradients_over_many_tiles(created, W0, n):
    c = created["c"]
    leaves, rows = tiled_batch(created, n)
    assert np.array_equal(handle_idx(c, leaves), created["idx"][rows]), "the assignment of a leaf depends on its place in the batch"
    g, aux = fwdbwd(c, leaves)
    vals, g64, g32 = ref_created(created, W0, n)
    check_gradients(f"n={n}", g, g64, g32)
    check_loss(f"n={n}", aux, vals)


def test_gradients_over_many_tiles_with_the_pair_kernels(created, W0, monkeypatch):
    """VQHIP_TRAIN_WGRAD=pairs: the weight-gradient family that other compute-unit counts fall back to."""
    n = 1025
    monkeypatch.setenv("VQHIP_TRAIN_WGRAD", "pairs")
    c = new_codec(W0)
    monkeypatch.delenv("VQHIP_TRAIN_WGRAD")
    try:
        leaves, _ = tiled_batch(created, n)
        g, aux = fwdbwd(c, leaves)
    finally:
        c.close()
    vals, g64, g32 = ref_created(created, W0, n)
    check_gradients(f"pairs n={n}", g, g64, g32)
    check_loss(f"pairs n={n}", aux, vals)


# ---- d: new weights ----
def check_at_weights(label, c, W, cand):
    """33 leaves screened at W, the handle's assignment, gradients and loss against fp64 at W."""
    keep, idx64 = screen(cand, W)
    chosen = pick(keep, 33)
    print(f"{label}: {len(keep)} of {len(cand)} candidates pass the screening")
    leaves, idx =np.ascontiguousarray(cand[chosen]), idx64[chosen]
    assert np.array_equal(handle_idx(c, leaves), idx), f"{label}: the handle's assignment is not the fp64 argmin"
    g, aux = fwdbwd(c, leaves)
    vals, g64, g32 = references(leaves, np.ones(33), W, idx)
    check_gradients(label, g, g64, g32)
    check_loss(label, aux, vals)


def test_gradients_after_set_params(W0, cand):
    """seed 1's network through set_params (the codebook stays seed 0's): a fragment table or the stem table that was not rebuilt
    gives an error of order 1."""
    W1 = synth.make_weights(1)
    c = new_codec(W0)
    try:
        c.fulltrain_set_params(dict_to_flat(W1))
        check_at_weights("set_params", c, {**W1, "quantizer.embedding": W0["quantizer.embedding"]}, cand)
    finally:
        c.close()


def test_gradients_after_apply(W0, cand):
    """One AdamW step from zero moments on a gradient of random signs (no weight decay) moves every parameter by lr, and the EMA
    with the statistics of a 96-leaf batch moves the codebook; the gradients at the weights the handle then holds."""
    c = new_codec(W0)
    try:
        p0 = c.fulltrain_get_params()
        x = dev(cand[:96])
        scratch = torch.zeros(len(p0), dtype=torch.float32, device="cuda")
        aux = torch.zeros(AUX_FLOATS, dtype=torch.float32, device="cuda")
        c.fulltrain_fwdbwd_device(x.data_ptr(), 96, 96, scratch.data_ptr(), aux.data_ptr())
        G = np.where(np.random.default_rng(41).random(len(p0)) < 0.5, np.float32(-1.0), np.float32(1.0))
        d_g = dev(G)
        c.fulltrain_apply_device(d_g.data_ptr(), aux.data_ptr(), LR_APPLY, 1, weight_decay=0.0)
        torch.cuda.synchronize()
        p = c.fulltrain_get_params()
        # lr sign(g) / (1 + eps / |g|): a dozen roundings of the step, and the rounding of the parameter
        assert (np.abs((p.astype(np.float64) - p0) + LR_APPLY * G.astype(np.float64)) <= 1e-6 * LR_APPLY + U * (np.abs(p0) + LR_APPLY)).all()
        E = c.train_get_state()["embedding"]
        moved = np.abs(E - W0["quantizer.embedding"]).max(1)
        used = aux.cpu().numpy()[:256] > 0      # a code no row chose keeps its place: embed_avg and cluster_size decay alike
        print(f"apply: the batch used {int(used.sum())} of 256 codes; the EMA moved their rows by {float(moved[used].min()):.1e} .. "
              f"{float(moved[used].max()):.1e}, the others by at most {float(moved[~used].max()):.1e}")
        assert used.sum() >= 32 and (moved[used] > 1e-4).all() and (moved[~used] < 1e-6).all()
        check_at_weights("apply", c, {**flat_to_dict(p), "quantizer.embedding": E}, cand)
    finally:
        c.close()


# ---- e, f ----
def test_nothing_of_a_nan_batch_is_left_behind(created, fresh33, W0, cand):
    """Only the code gather, the loss head, dz and the loss sums mask leaf < n_leaves; everything else works on whole tiles and relies
    on freshly written activations.  After a 48-leaf batch whose leaves 40 and 41 (past the 33-leaf batch, inside its second tile)
    are all NaN and all +Inf, the 33-leaf batch must give the bits of a fresh handle."""
    c = new_codec(W0)
    try:
        bad = cand[:48].copy()
        bad[40], bad[41] = np.nan, np.inf
        g_bad, _ = fwdbwd(c, bad)
        assert not np.isfinite(g_bad).all()      # (the poison did reach the gradient buffers)
        g, aux = fwdbwd(c, np.ascontiguousarray(created["leaves"][:33]))
    finally:
        c.close()
    assert np.isfinite(g).all() and np.isfinite(aux).all()
    assert np.array_equal(bits(g), bits(fresh33[0])) and np.array_equal(bits(aux), bits(fresh33[1]))


def test_overlap_entry_point_gives_the_plain_calls_bits(created, fresh33):
    c, n = created["c"], 33
    x = dev(created["leaves"][:n])
    g = torch.zeros(c.fulltrain_param_count(), dtype=torch.float32, device="cuda")
    a = torch.zeros(AUX_FLOATS, dtype=torch.float32, device="cuda")
    calls = []
    c.fulltrain_fwdbwd_overlap_device(x.data_ptr(), n, n, g.data_ptr(), a.data_ptr(), 0, lambda: calls.append(1))
    torch.cuda.synchronize()
    assert calls == [1]
    assert np.array_equal(bits(g.cpu().numpy()), bits(fresh33[0])) and np.array_equal(bits(a.cpu().numpy()), bits(fresh33[1]))
