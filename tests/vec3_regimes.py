"""Weight regimes and codebook-size edges of the Vec3 model — TEST INFRASTRUCTURE shared by tests/test_vec3_regimes_host.py,
tests/test_gpu_vec3_regimes.py and tests/golden/make_golden_vec3_regimes.py.

Every weight set is regenerated from numpy alone (synth_vec3.make_weights, float32 arithmetic with correctly rounded
elementwise operations only), so no weight file is stored and any machine gets the same bytes.  The bars of the GPU tests
live here too, each tied to what the float32 torch restatement itself achieves against float64, so that the CPU suite can
show them satisfiable by the restatement and violated by three deliberately wrong ones."""
from __future__ import annotations

import os

import numpy as np
import torch

import torch_ref_vec3 as tr
from vqvdb_amd import synth_vec3

F = np.float32
REGIMES = ("seed1", "seed2", "default_like", "deadcodes", "wide", "saturated")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# two files: the decoded voxels of six regimes do not fit one committed file of at most 1 MiB
FIXTURE_FILES = ((os.path.join(GOLDEN_DIR, "golden_vec3_regimes_v1.npz"), REGIMES[:3]),
                 (os.path.join(GOLDEN_DIR, "golden_vec3_regimes_v1_part2.npz"), REGIMES[3:]))
K_EDGES = (1, 2, 31, 32, 33, 127, 128, 129, 255, 257, 4095, 4097, 65535, 65536)
FIXTURE_LEAVES, FRESH_LEAVES, LEAF_SEED = 24, 40, 777
K_LEAVES, K_SEED = 8, 31
# leaves of the twelve-layer comparison (indices into fresh_leaves()): a natural leaf and the 1e-3 noise edge leaf, whose
# small GroupNorm variances make the layers sensitive to eps (a restatement with eps = 1e-6 is 2e-3 off there)
LAYER_LEAVES = (6, 46)
# constant index rows whose decode saturates in the `saturated` regime: float64 tanh is within 3e-10 of 1, a hundred times
# closer than the 3e-8 at which float32 rounds to 1.0 (found by decoding all 4096 constant rows; the host suite re-checks it)
SATURATING_CODES = (2220, 1277)


def is_groupnorm(name: str) -> bool:
    return ".gn1." in name or ".gn2." in name or name.startswith("encoder.pre.1.") or name.startswith("decoder.stem.1.")


def _row_norms(e: np.ndarray) -> np.ndarray:
    """float32 L2 norm of every row, summed in dimension order (elementwise operations only: the same bits anywhere)."""
    s = np.zeros(e.shape[0], F)
    for d in range(e.shape[1]):
        s = s + e[:, d] * e[:, d]
    return np.sqrt(s)


def regimes() -> dict:
    """name -> weight dict of the six file-free regimes (float32, synth_vec3.TENSORS' names and shapes)."""
    base = synth_vec3.make_weights(0)
    out = {"seed1": synth_vec3.make_weights(1), "seed2": synth_vec3.make_weights(2)}

    w = {k: v.copy() for k, v in base.items()}
    for k in w:
        if is_groupnorm(k):
            w[k] = np.full_like(w[k], 1.0 if k.endswith(".weight") else 0.0)
        elif k.endswith(".conv2.weight"):
            w[k] = w[k] * F(1e-3)
    e = w["quantizer.embedding"]
    w["quantizer.embedding"] = e / _row_norms(e)[:, None]
    out["default_like"] = w

    w = {k: v.copy() for k, v in base.items()}
    w["quantizer.embedding"][5::29] *= F(0.02)
    out["deadcodes"] = w

    w = {k: v.copy() for k, v in base.items()}
    for k in ("encoder.proj.weight", "encoder.proj.bias", "quantizer.embedding"):
        w[k] = w[k] * F(8.0)
    out["wide"] = w

    w = {k: v.copy() for k, v in base.items()}
    w["decoder.final.weight"] = w["decoder.final.weight"] * F(6.0)
    out["saturated"] = w
    return {k: {n: np.ascontiguousarray(v, dtype=F) for n, v in out[k].items()} for k in REGIMES}


def load_fixture() -> dict:
    """regime -> {"idx", "second", "gap", "rec"} of the reference model (tests/golden/make_golden_vec3_regimes.py)."""
    out = {}
    for path, names in FIXTURE_FILES:
        g = np.load(path)
        for name in names:
            out[name] = {k: g[f"{name}/{k}"] for k in ("idx", "second", "gap", "rec")}
    return out


def fixture_leaves() -> np.ndarray:
    """The 32 leaves of tests/golden/golden_vec3_regimes_v1.npz."""
    return np.ascontiguousarray(np.concatenate([synth_vec3.make_leaves(FIXTURE_LEAVES, seed=LEAF_SEED), synth_vec3.edge_leaves()]))


def fresh_leaves() -> np.ndarray:
    """The 48 leaves of the comparisons with float64 (the fixture's first 24 are its first 24)."""
    return np.ascontiguousarray(np.concatenate([synth_vec3.make_leaves(FRESH_LEAVES, seed=LEAF_SEED), synth_vec3.edge_leaves()]))


def k_leaves() -> np.ndarray:
    """The 16 leaves of the codebook-size edges."""
    return np.ascontiguousarray(np.concatenate([synth_vec3.make_leaves(K_LEAVES, seed=K_SEED), synth_vec3.edge_leaves()]))


def random_indices(k: int, n: int = 24, seed: int = 5) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, k, size=(n, 64)).astype(np.uint16)


def decode_indices(first, k: int, n_random: int = 24) -> np.ndarray:
    """The index rows every decode comparison uses: `first` (the fixture's indices, or an encode result), random rows and,
    where the codebook has them, the two constant rows SATURATING_CODES."""
    const = [np.full((1, 64), c, np.uint16) for c in SATURATING_CODES if c < k]
    return np.ascontiguousarray(np.concatenate([np.asarray(first, np.uint16), random_indices(k, n_random)] + const))


def decode_refs(idx, w32, w64) -> tuple:
    """(float32 restatement, float64 restatement) of decode(idx)."""
    with torch.no_grad():
        return tr.decode(idx, w32).numpy(), tr.decode(idx, w64).numpy()


def flat(z) -> torch.Tensor:
    """[n,64,4,4,4] latents -> [n*64, 64], position-major as VQVAE.encode."""
    z = torch.as_tensor(z)
    return z.reshape(z.shape[0], 64, 64).permute(0, 2, 1).reshape(-1, 64)


def latents(leaves, w) -> torch.Tensor:
    with torch.no_grad():
        return flat(tr.encoder(leaves, w))


def chunked_distances(zf, e, chunk: int = 256):
    """Yields (lo, hi, [hi-lo, K] expanded distances) of flattened latents zf against codebook e, `chunk` positions at a time."""
    ee = (e ** 2).sum(1)
    for lo in range(0, zf.shape[0], chunk):
        z = zf[lo:lo + chunk]
        yield lo, lo + len(z), (z ** 2).sum(1, keepdim=True) + ee - 2 * z @ e.t()


def top2(zf, e):
    """(first minimum, second-nearest code, relative top-2 gap (d2 - d1) / max(|d1|, |z|^2, 1e-30)) per position, in the
    dtype of zf; the gap is +inf for a one-row codebook."""
    idx = np.zeros(zf.shape[0], np.int64)
    second = np.zeros(zf.shape[0], np.int64)
    gap = np.full(zf.shape[0], np.inf)
    with torch.no_grad():
        for lo, hi, dist in chunked_distances(zf, e):
            first = torch.argmin(dist, dim=1)
            idx[lo:hi] = first.numpy()
            if e.shape[0] == 1:
                continue
            d1 = dist.gather(1, first[:, None])[:, 0]
            rest = dist.clone()
            rest.scatter_(1, first[:, None], float("inf"))
            sec = torch.argmin(rest, dim=1)
            d2 = rest.gather(1, sec[:, None])[:, 0]
            scale = torch.maximum(torch.maximum(d1.abs(), (zf[lo:hi] ** 2).sum(1)), torch.full_like(d1, 1e-30))
            second[lo:hi], gap[lo:hi] = sec.numpy(), ((d2 - d1) / scale).numpy()
    return idx, second, gap


def check_latent_vs_fp64(idx, zf64, e64):
    """check_vs_fp64's criterion of tests/test_gpu_vec3.py on given float64 latents [P, 64] (a precision mode's own latent, or
    a codebook too large for one distance matrix): the chosen code's float64 distance is within 1e-5 * max(|d_min|, |z|^2)
    of the float64 minimum.  Returns the worst excess in units of the bound."""
    pick = torch.as_tensor(np.asarray(idx).reshape(-1).astype(np.int64))
    worst = 0.0
    with torch.no_grad():
        for lo, hi, dist in chunked_distances(zf64, e64):
            dmin = dist.min(dim=1).values
            got = dist.gather(1, pick[lo:hi, None])[:, 0]
            bound = 1e-5 * torch.maximum(dmin.abs(), (zf64[lo:hi] ** 2).sum(1))
            worst = max(worst, float(((got - dmin) / bound.clamp_min(1e-300)).max()))
            assert bool((got - dmin <= bound).all()), f"worst excess {worst:.2f} x bound"
    return worst


def planted_codes(w: dict, leaves, rows=None, separation: float = 0.05, z64=None):
    """Overwrites codebook rows `rows` (default: 0, K-1 and the two around the last 128-code block's start, as planted_rows)
    with the float32-rounded float64 latents of as many distinct positions -> (weights, flat positions leaf*64 + p, rows).
    Positions are taken in a fixed order and kept when finite, non-zero and at least `separation` * |z|^2 (squared distance)
    from every latent kept before, so that no two planted rows compete; z64 may carry the float64 latents [P, 64] of `leaves`
    where a caller has them already (they do not depend on the codebook).  The precondition every caller asserts in float64:
    at each planted position the planted row wins with a relative top-2 gap >= 1e-3 (planted_precondition)."""
    k = w["quantizer.embedding"].shape[0]
    rows = planted_rows(k) if rows is None else [int(r) for r in rows]
    if z64 is None:
        z64 = latents(leaves, tr.weights_to_torch({n: v for n, v in w.items() if n != "quantizer.embedding"}, torch.float64))
    z = np.asarray(z64)
    n = z.shape[0] // 64
    order = np.arange(n * 64).reshape(n, 64)[:, (21 * np.arange(64) + 21) % 64].T.reshape(-1)   # position 21 of every leaf, then 42, ...
    kept = []
    for p in order:
        zz = float((z[p] ** 2).sum())
        if not np.isfinite(zz) or zz == 0.0:
            continue
        if all(float(((z[p] - z[q]) ** 2).sum()) >= separation * max(zz, float((z[q] ** 2).sum())) for q in kept):
            kept.append(int(p))
        if len(kept) == len(rows):
            break
    assert len(kept) == len(rows), "not enough distinct latents to plant"
    e = w["quantizer.embedding"].copy()
    e[rows] = z[kept].astype(F)
    out = dict(w)
    out["quantizer.embedding"] = e
    return out, np.array(kept, np.int64), np.array(rows, np.int64)


def planted_rows(k: int) -> list:
    """{0, K-1, start of the last (possibly partial) 128-code block, the row before it}, deduplicated, increasing."""
    last = 128 * ((k - 1) // 128)
    return sorted({0, k - 1, last} | ({last - 1} if last >= 1 else set()))


def planted_precondition(w: dict, leaves, positions, rows, z64=None):
    """Asserts in float64 that each planted row is the first minimum of its position with a relative gap >= 1e-3; returns the
    smallest gap."""
    e64 = torch.from_numpy(w["quantizer.embedding"]).double()
    if z64 is None:
        z64 = latents(leaves, tr.weights_to_torch({n: v for n, v in w.items() if n != "quantizer.embedding"}, torch.float64))
    idx, _second, gap = top2(torch.as_tensor(z64)[torch.as_tensor(positions)], e64)
    assert np.array_equal(idx, rows), f"planted rows {rows} do not win their positions in float64: {idx}"
    assert (gap >= 1e-3).all(), f"planted rows win by less than 1e-3: {gap}"
    return float(gap.min())


def k_edge_weights(big: dict, k: int) -> dict:
    """The K-code model sliced from make_weights(0, k_codes=65536) (code i is the same vector for every K)."""
    w = dict(big)
    w["quantizer.embedding"] = np.ascontiguousarray(big["quantizer.embedding"][:k])
    return w


# ---- the bars of the GPU tests ------------------------------------------------------------------------------------------
def voxel_bar(rec32, rec64) -> tuple:
    """(bar, d_ref): d_ref is the float32 restatement's largest distance from float64 on the same indices; the bar is
    max(1e-5, 2 * d_ref), the factor 2 because another valid float32 summation order may land on the other side of the exact
    value."""
    d_ref = float(np.abs(np.asarray(rec32, np.float64) - np.asarray(rec64, np.float64)).max())
    return max(1e-5, 2.0 * d_ref), d_ref


def check_voxels(rec, rec32, rec64) -> tuple:
    """Decoded voxels against float64 at the voxel bar, and |rec| <= 1.  Returns (distance, d_ref)."""
    bar, d_ref = voxel_bar(rec32, rec64)
    d = float(np.abs(np.asarray(rec, np.float64) - np.asarray(rec64, np.float64)).max())
    assert d <= bar, f"voxels {d:.3e} from float64, bar {bar:.3e} (float32 restatement: {d_ref:.3e})"
    assert float(np.abs(rec).max()) <= 1.0
    return d, d_ref


def layer_acts(leaves, idx, w) -> dict:
    """The twelve debug-fetch layers (encoder on the leaves, decoder on idx [n,64]) as float64 [n, C, positions] arrays."""
    acts = {}
    with torch.no_grad():
        tr.encoder(leaves, w, acts)
        tr.decode(idx, w, acts)
    return {k: v.reshape(v.shape[0], v.shape[1], -1).double().numpy() for k, v in acts.items()}


def check_layers(got: dict, acts32: dict, acts64: dict) -> tuple:
    """Every layer of every leaf against float64: largest error <= max(1e-5, 2 * the float32 restatement's own relative
    distance) of the leaf's tensor's largest value.  Returns (worst layer, its relative error, the restatement's relative error there)."""
    worst = ("", -1.0, 0.0)
    assert sorted(got) == sorted(acts64)
    for k, refs in acts64.items():
        for leaf, ref in enumerate(refs):
            top = float(np.abs(ref).max())
            rel32 = float(np.abs(acts32[k][leaf] - ref).max()) / top
            rel = float(np.abs(np.asarray(got[k][leaf], np.float64).reshape(ref.shape) - ref).max()) / top
            assert rel <= max(1e-5, 2.0 * rel32), f"{k}, leaf {leaf}: {rel:.3e} of the largest value, float32 restatement {rel32:.3e}"
            if rel > worst[1]:
                worst = (k, rel, rel32)
    return worst


def check_duplicates(first, idx, pairs):
    """After rows dst were overwritten with rows src: every position that chose src now has the lower index of the pair, the
    higher never occurs (the distances to both rows are bit-identical, and no other row moved closer)."""
    for src, dst, lo, hi in pairs:
        assert (first == src).any()
        assert (idx[first == src] == lo).all(), (src, dst)
        assert not (idx == hi).any(), (src, dst)
