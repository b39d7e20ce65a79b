"""Vec3 full training at its edges: all 60 parameter gradients against fp64 autograd at ragged batch sizes (33, 17, 15 and 1 leaves:
partial leaf groups of wgrad_k / bias_part_k, a lone leaf in the two-leaves-per-workgroup data-gradient convs), with n_global != n,
and at weights that reached the handle through set_params and through apply (every table the backward reads is rebuilt); and
the optimizer both handles share, adamw_k, on teacher-forced gradients against an fp64 restatement, element by element."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch_ref_vec3_fulltrain as tf  # noqa: E402
from vec3_fulltrain_common import _screen, dev, forward, fwdbwd, new_codec, split  # noqa: E402
from vqvdb_amd import synth, synth_vec3, vec3_full_training, weightpack  # noqa: E402
from vqvdb_amd.codec import HipCodec, HipVec3Codec  # noqa: E402

pytestmark = pytest.mark.gpu

K = synth_vec3.K_CODES
NAMES = tf.param_names()
N_MAX = 33                 # two full groups of V3F_GROUP = 16 leaves and a group of one; an odd leaf count
SIZES = (33, 17, 15, 1)    # ..., a full group and a group of one, a single partial group, a lone leaf
BAR = 1e-5                 # of the tensor's largest fp64 gradient
LR_APPLY = 2e-3            # the one AdamW step of test_gradients_after_apply
U = 2.0 ** -24             # unit roundoff of float32


@pytest.fixture(scope="module")
def W0():
    return synth_vec3.make_weights(0)


@pytest.fixture(scope="module")
def cand():
    return synth_vec3.make_leaves(128, seed=9200)


def screened(c, cand, W):
    """The first N_MAX candidates that pass the screening at the weights W, with the handle's own assignment."""
    idx, _ = forward(c, cand)
    keep = _screen(cand, W, idx, n_keep=N_MAX)
    return np.ascontiguousarray(cand[keep[:N_MAX]])


def reference(c, leaves, W):
    """fp64 and fp32 autograd at the weights W with the handle's assignment of this very batch -> (values, g64, g32)"""
    idx, _ = forward(c, leaves)
    params = {k: np.asarray(W[k]) for k in NAMES}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    vals, g64 = tf.gradients(leaves, params, W["quantizer.embedding"], idx.reshape(-1), torch.float64)
    _, g32 = tf.gradients(leaves, params, W["quantizer.embedding"], idx.reshape(-1), torch.float32)
    return vals, g64, g32


def check_gradients(label, g, g64, g32, factor=1.0):
    """Every tensor of the flat gradient g against factor * g64, relative to that tensor's largest value.  The bar is BAR; on a
    tensor where torch's own fp32 gradient is more than 5e-6 from fp64 it is max(BAR, twice that error), since two fp32 sums in
    different orders may differ from each other by as much as each differs from fp64.  No bar comes from the GPU's number."""
    gpu = split(g)
    worst, worst32, widened, failed = 0.0, 0.0, [], []
    for k in NAMES:
        ref = g64[k].reshape(-1) * factor
        top = float(np.abs(ref).max())
        assert top > 0.0, f"{label} {k}: the fp64 gradient is all zero"
        err = float(np.abs(gpu[k] - ref).max()) / top
        err32 = float(np.abs(g32[k].reshape(-1).astype(np.float64) * factor - ref).max()) / top
        bar = max(BAR, 2.0 * err32) if err32 > 5e-6 else BAR
        print(f"{label} {k:40s} gpu {err:.2e}  torch fp32 {err32:.2e}  bar {bar:.2e}")
        worst, worst32 = max(worst, err), max(worst32, err32)
        if bar > BAR:
            widened.append(k)
        if not err < bar:
            failed.append((k, err, bar))
    print(f"{label}: worst parameter-gradient error {worst:.2e}, torch fp32's worst {worst32:.2e}, widened bars: {widened}")
    assert not failed, (label, failed)


# ---- a, b: ragged sizes and n_global at the created weights ----
@pytest.fixture(scope="module")
def created(W0, cand):
    """One handle at the weights it was created with, the screened batch, and the references by batch size (computed once)."""
    c = new_codec(W0)
    state = {"c": c, "leaves": screened(c, cand, W0), "ref": {}}
    fwdbwd(c, cand[:48])      # the gradient buffers of the leaves past every batch below hold another batch's values, not fresh memory
    yield state
    c.close()


def ref_created(created, W0, n):
    if n not in created["ref"]:
        created["ref"][n] = reference(created["c"], created["leaves"][:n], W0)
    return created["ref"][n]


@pytest.mark.parametrize("n", SIZES)
def test_gradients_at_ragged_batch_sizes(created, W0, n):
    c, leaves = created["c"], np.ascontiguousarray(created["leaves"][:n])
    g, aux = fwdbwd(c, leaves)
    vals, g64, g32 = ref_created(created, W0, n)
    check_gradients(f"n={n}", g, g64, g32)
    loss = vec3_full_training.losses_from_aux(aux, K)
    assert abs(loss["loss"] - vals["loss"]) / vals["loss"] < 1e-5, (loss["loss"], vals["loss"])


def test_gradients_with_a_larger_global_batch(created, W0):
    """n_global = 40 on 17 leaves: every term of the loss is a mean over leaves and GroupNorm is per leaf, so the gradient is the
    17-leaf mean loss's times 17 / 40 exactly."""
    n, n_global = 17, 40
    c, leaves = created["c"], np.ascontiguousarray(created["leaves"][:n])
    g, _ = fwdbwd(c, leaves, n_global)
    _, g64, g32 = ref_created(created, W0, n)
    check_gradients(f"n={n} n_global={n_global}", g, g64, g32, factor=n / n_global)


# ---- c, d: other weights ----
def test_gradients_after_set_params(W0, cand):
    """seed 1's network weights through set_params (the codebook stays seed 0's): a table the backward reads that was not rebuilt
    gives an error of order 1."""
    W1 = synth_vec3.make_weights(1)
    c = new_codec(W0)
    c.fulltrain_set_params(vec3_full_training.state_to_vec(W1))
    W = {**W1, "quantizer.embedding": W0["quantizer.embedding"]}
    leaves = screened(c, cand, W)
    g, aux = fwdbwd(c, leaves)
    vals, g64, g32 = reference(c, leaves, W)
    check_gradients("set_params", g, g64, g32)
    loss = vec3_full_training.losses_from_aux(aux, K)
    assert abs(loss["loss"] - vals["loss"]) / vals["loss"] < 1e-5, (loss["loss"], vals["loss"])
    c.close()


def sign_gradient(n):
    return np.where(np.random.default_rng(41).random(n) < 0.5, np.float32(-1.0), np.float32(1.0))


def test_gradients_after_apply(W0, cand):
    """One AdamW step from zero moments on a gradient of random signs (no weight decay, no EMA) moves every parameter by lr; the
    gradients at the weights the handle then holds."""
    c = new_codec(W0)
    p0 = c.fulltrain_get_params()
    G = sign_gradient(len(p0))
    d_g = dev(G)
    c.fulltrain_apply_device(d_g.data_ptr(), 0, LR_APPLY, 1, weight_decay=0.0)
    torch.cuda.synchronize()
    p = c.fulltrain_get_params()
    # lr sign(g) / (1 + eps / |g|): a dozen roundings of the step, and the rounding of the parameter
    assert (np.abs((p.astype(np.float64) - p0) + LR_APPLY * G.astype(np.float64)) <= 1e-6 * LR_APPLY + U * (np.abs(p0) + LR_APPLY)).all()
    W = {**vec3_full_training.vec_to_state(p), "quantizer.embedding": W0["quantizer.embedding"]}
    leaves = screened(c, cand, W)
    g, aux = fwdbwd(c, leaves)
    vals, g64, g32 = reference(c, leaves, W)
    check_gradients("apply", g, g64, g32)
    loss = vec3_full_training.losses_from_aux(aux, K)
    assert abs(loss["loss"] - vals["loss"]) / vals["loss"] < 1e-5, (loss["loss"], vals["loss"])
    c.close()


# ---- e: teacher-forced AdamW on both handles ----
STRETCH = 1024 * 256       # one sweep of adamw_k's grid-stride loop
TAIL = 300
SPECIAL = (0.0, 1e-15, -1e-15, 1e4, -1e4)


def adamw_gradient(n, rng):
    """Normal draws times 10**uniform(-6, 2); exact zeros, +-1e-15 and +-1e4 at every 1009th element and as the last five before
    the very last, which is a draw; 0 or |g| >= 1e-15 throughout, so g^2 (1 - beta2) stays a normal float."""
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    tiny = (g != 0) & (np.abs(g) < 1e-15)
    g[tiny] = np.copysign(np.float32(1e-15), g[tiny])
    for j, s in enumerate(SPECIAL):
        g[j * 211:n - 8:1009] = s
        g[n - 2 - j] = s
    return g


def adamw_moments(n, g, rng, beta1, cancelling):
    """m and sqrt(v) of one scale per element (independent of g's, over the same eight decades), v >= 0, and m = v = 0 on
    every other element with g = 0.

    The parameter bound counts the roundings on p's own path.  Where b1 m and (1 - b1) g have opposite signs and nearly cancel, the
    rounding of the new m (inside its own bound, relative to |b1 m| + |(1 - b1) g|) is a large relative error of m itself and so of the
    update; at |p| below lr that is outside the 16 operations (a float32 restatement of the kernel on the CPU then misses the bound
    on two or three of 5 124 067 elements, by up to 15 x).  Unless `cancelling`, m takes g's sign where the two terms are of
    opposite sign and within a factor 4 of each other: |m'| >= 0.6 (|b1 m| + |(1 - b1) g|) everywhere.  The case with lr = 0, where
    the parameters do not see m, keeps the cancelling elements for the bound on m."""
    s = 10.0 ** rng.uniform(-6, 2, n)
    m = (rng.standard_normal(n) * s).astype(np.float32)
    v = (((0.5 + np.abs(rng.standard_normal(n))) * s) ** 2).astype(np.float32)
    both = np.flatnonzero(g == 0)[::2]
    m[both], v[both] = 0.0, 0.0
    if not cancelling:
        a, b = np.abs(np.float64(beta1) * m), np.abs((1.0 - np.float64(beta1)) * g)
        near = (np.sign(m) * np.sign(g) < 0) & (a <= 4 * b) & (b <= 4 * a)
        m[near] = -m[near]
    return m, v


#             lr    step    betas         eps   wd    moments
ADAMW_CASES = {
    "first_step": (5e-4, 1, (0.9, 0.999), 1e-8, 1e-4, False),
    "late_step": (1e-3, 1000, (0.8, 0.99), 1e-6, 0.01, True),
    "corrections_of_one": (1e-3, 10 ** 6, (0.9, 0.999), 1e-8, 1e-4, True),
    "lr_zero": (0.0, 7, (0.9, 0.999), 1e-8, 1e-4, True),
}


def make_handle(kind):
    if kind == "vec3":
        W = synth_vec3.make_weights(0)
        return W, new_codec(W), 5124067
    W = synth.make_weights(0)
    c = HipCodec(weightpack.dumps(W))
    c.fulltrain_begin()
    return W, c, 995905


@pytest.mark.parametrize("case", list(ADAMW_CASES))
@pytest.mark.parametrize("kind", ["vec3", "scalar"])
def test_adamw_on_a_given_gradient(kind, case):
    """|dm| <= 4 u (|b1 m| + |(1 - b1) g|), |dv| <= 4 u (b2 v + (1 - b2) g^2), |dp| <= 16 u (|p| + |update|) against the fp64
    restatement of the float32 arguments, u = 2^-24: the kernel's operation count, each operation rounding by at most u."""
    lr, step, betas, eps, wd, with_moments = ADAMW_CASES[case]
    W, c, n = make_handle(kind)
    assert c.fulltrain_param_count() == n
    rng = np.random.default_rng(1000 + step)
    g = adamw_gradient(n, rng)
    for lo in list(range(0, n - TAIL, STRETCH // 2)) + [n - TAIL]:      # no trivial half stretch, so no trivial stretch; no trivial tail
        part = g[lo:min(lo + STRETCH // 2, n)]
        assert len(np.unique(part)) > 0.9 * len(part), lo
    assert all((g[n - TAIL:] == np.float32(s)).any() for s in SPECIAL) and g[n - 1] not in [np.float32(s) for s in SPECIAL]
    p0 = c.fulltrain_get_params()
    if with_moments:
        m0, v0 = adamw_moments(n, g, rng, np.float32(betas[0]), cancelling=lr == 0.0)
        assert ((g == 0) & (m0 == 0) & (v0 == 0)).any() and (v0 >= 0).all() and (np.sign(m0) * np.sign(g) < 0).any()
        c.fulltrain_set_opt_state(m0, v0)
    else:
        m0, v0 = c.fulltrain_get_opt_state()
        assert not m0.any() and not v0.any()
    d_g = dev(g)
    c.fulltrain_apply_device(d_g.data_ptr(), 0, lr, step, betas=betas, adam_eps=eps, weight_decay=wd)
    torch.cuda.synchronize()
    p, (m, v) = c.fulltrain_get_params(), c.fulltrain_get_opt_state()

    f = np.float32
    b1, b2 = float(f(betas[0])), float(f(betas[1]))
    rp, rm, rv = tf.adamw_fp64(p0, g, m0, v0, f(lr), step, (f(betas[0]), f(betas[1])), f(eps), f(wd))
    g64, m64, v64, p64 = (a.astype(np.float64) for a in (g, m0, v0, p0))
    bound_m = 4 * U * (np.abs(b1 * m64) + np.abs((1 - b1) * g64))
    bound_v = 4 * U * (b2 * v64 + (1 - b2) * g64 * g64)
    update = rp - p64 * (1.0 - float(f(lr)) * float(f(wd)))
    bound_p = 16 * U * (np.abs(p64) + np.abs(update))
    worst = {}
    for name, got, ref, bound in (("m", m, rm, bound_m), ("v", v, rv, bound_v), ("p", p, rp, bound_p)):
        assert np.isfinite(got).all(), name
        err = np.abs(got - ref)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst[name] = (float(ratio.max()), int(ratio.argmax()))
    print(f"adamw {kind} {case}: worst error / bound  m {worst['m'][0]:.3f}  v {worst['v'][0]:.3f}  p {worst['p'][0]:.3f}")
    for name, (r, i) in worst.items():
        assert r <= 1.0, (name, r, i, float(g[i]), float(m0[i]), float(v0[i]), float(p0[i]))
    if lr == 0.0:
        assert np.array_equal(p.view(np.uint32), p0.view(np.uint32)), "lr = 0 changed the parameters"
        assert not np.array_equal(m, m0) and not np.array_equal(v, v0)
    else:
        assert np.count_nonzero(p != p0) > 0.9 * n
    if kind == "vec3":      # the live forward tables follow P
        fresh = HipVec3Codec(weightpack.dumps({**W, **vec3_full_training.vec_to_state(p)}))
        leaves = synth_vec3.make_leaves(64, seed=9400)
        assert np.array_equal(c.encode(leaves), fresh.encode(leaves))
        fresh.close()
    c.close()
