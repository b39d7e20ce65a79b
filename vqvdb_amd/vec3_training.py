#!/usr/bin/env python3
"""Codebook (EMA) training of the Vec3 model VQVAE(3, 64, K) on the HIP backend — the Vec3 counterpart of
codebook_training.py + train_codebook.py.

The device work is in libvqvdb_hip.so (vqhip_vec3_train_*, include/vqvdb_hip_vec3_train.h): the training-mode forward of
VectorQuantizerEMA (python/VQVAE_v2.py:107-156) on the Vec3 encoder's latent, its eval forward (:344-348) and the buffers
check_and_reset_dead_codes (:382-417) works on.  Encoder and decoder weights stay frozen.  Per step and rank:

    stats = encoder -> latent -> assign -> {encodings_sum, dw, |z-e|^2, rows}     (HIP kernels, deterministic)
    all_reduce(stats, SUM)                                                         (the only collective)
    EMA update of cluster_size / embed_avg / embedding + search-table rebuild      (HIP kernels)

Epoch driver (one process per GPU, or under torch.distributed.run):

    python -m vqvdb_amd.vec3_training train --pack vec3.vqw --model_path out/vec3_quantizer.npz [--data_dir DIR] [--export-pack]

Data: `.npy` files of shape [N,8,8,8,3] float32, channels last, as the reference's VDBLeafDataset(in_channels=3) reads them;
every 12th leaf and a 50 % train / validation split as the Vec3 notebook (notebook_vec3f.ipynb); synthetic synth_vec3
leaves when no directory is given.  The rest of the loop follows python/training.py: shuffled batches, dead-code reset
every 5 epochs from the first batch's encoder outputs, validation, best-validation checkpoint, final save.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys
from typing import Optional

import numpy as np
import torch

from vqvdb_amd.codec import HipVec3Codec
from vqvdb_amd.training_common import LoopSpec, TrainerBase, allreduce_stats, leaves_arg, run_training, split_train_val, vq_metrics

D = 64
SUBSAMPLE = 12                   # notebook_vec3f.ipynb: every 12th leaf
TRAIN_FRACTION = 0.5             # notebook_vec3f.ipynb: 50 % / 50 % random_split
SPEC = LoopSpec()


def stats_floats(k: int) -> int:
    return 66 * k + 1


def metrics_from_stats(stats: np.ndarray, k: int, commitment_cost: float = 0.25) -> dict:
    """vq_loss, perplexity and codes used from an (all-reduced) statistics buffer [66K+1]."""
    return vq_metrics(stats, k, D, commitment_cost)


def _leaves_arg(leaves: torch.Tensor) -> tuple[torch.Tensor, int]:
    """A batch of Vec3 leaves ([n,512,3] or [n,8,8,8,3]) as a contiguous tensor and its leaf count."""
    return leaves_arg(leaves, 1536)


class Vec3CodebookTrainer(TrainerBase):
    """Drives vqhip_vec3_train_* for one rank.  `codec` is a vqvdb_amd.codec.HipVec3Codec on this rank's device."""
    leaf_values, d = 1536, D

    def __init__(self, codec, commitment_cost: float = 0.25, decay: float = 0.95, eps: float = 1e-4, group=None,
                 cluster_size: Optional[np.ndarray] = None, embed_avg: Optional[np.ndarray] = None, device: str = "cuda"):
        super().__init__(codec, commitment_cost, decay, eps, group, device)
        self.k = codec.model_info()["num_codes"]
        codec.train_begin(cluster_size, embed_avg)
        self.stats = torch.zeros(stats_floats(self.k), dtype=torch.float32, device=self.device)

    def step(self, leaves: torch.Tensor, keep_latent: bool = False, want_metrics: bool = True) -> Optional[dict]:
        """One EMA step on this rank's batch (float32 [n,512,3] or [n,8,8,8,3], resident on the device)."""
        leaves, n = self._leaves_arg(leaves)
        out = None
        with self._side_stream(leaves) as h:
            zptr = self._latent_ptr(n, keep_latent)
            self.codec.train_vq_stats_device(leaves.data_ptr(), n, self.stats.data_ptr(), latent_ptr=zptr, stream=h)
            allreduce_stats(self.stats, self.group)
            self.codec.train_vq_update_device(self.stats.data_ptr(), self.decay, self.eps, stream=h)
            if want_metrics:
                out = metrics_from_stats(self.stats.cpu().numpy(), self.k, self.commitment_cost)
        return out


# ---- epoch driver ------------------------------------------------------------------------------------------------------
def load_leaves(data_dir, synthetic_leaves: int, seed: int) -> np.ndarray:
    """All leaves as float32 [N,512,3]: every SUBSAMPLE-th leaf of the .npy files, or synthetic synth_vec3 leaves."""
    if data_dir:
        files = sorted(glob.glob(os.path.join(data_dir, "*.npy")))
        if not files:
            raise ValueError(f"No .npy files found in {data_dir}")
        arrs = []
        for f in files:
            a = np.load(f, mmap_mode="r")
            if a.shape[1:] != (8, 8, 8, 3):
                raise ValueError(f"File {f}: invalid shape {a.shape}. Expected suffix (8, 8, 8, 3)")
            arrs.append(np.asarray(a[::SUBSAMPLE], dtype=np.float32).reshape(-1, 512, 3))
        return np.concatenate(arrs)
    from vqvdb_amd import synth_vec3
    return synth_vec3.make_leaves(synthetic_leaves, seed=seed)


def export_pack(pack_path: str, state: dict, out_path: str):
    """The source pack with the trained quantizer.* buffers (vqhip_vec3_create reads quantizer.embedding)."""
    from vqvdb_amd import weightpack
    t = dict(weightpack.load(pack_path))
    for k in ("quantizer.embedding", "quantizer.cluster_size", "quantizer.embed_avg"):
        t[k] = np.ascontiguousarray(state[k], dtype=np.float32)
    weightpack.save(out_path, t)


def leaf_error_line(codec, batches) -> str:
    """--report-leaf-error: the per-leaf largest error |x - x^| of the given validation batches through
    HipVec3Codec.roundtrip (inference path, the handle's precision mode): median, 99th percentile and the worst leaf."""
    worst = torch.cat([codec.roundtrip(b.contiguous())[1][:, 0] for b in batches]).double().cpu().numpy()
    p50, p99, p100 = np.percentile(worst, [50, 99, 100])
    return f"         | Leaf max error over {len(worst)} val leaves: p50 {p50:.6f} | p99 {p99:.6f} | p100 (worst leaf) {p100:.6f}"


def train(args) -> dict:
    def build(local, device, world):
        codec = HipVec3Codec(args.pack, device_id=local)
        trainer = Vec3CodebookTrainer(codec, commitment_cost=args.commitment_cost, decay=args.decay, eps=args.eps, device=str(device))
        leaves = load_leaves(args.data_dir, args.synthetic_leaves, args.seed)
        return (codec, trainer, leaves, *split_train_val(len(leaves), args.seed, TRAIN_FRACTION))

    def export(trainer, path):
        export_pack(args.pack, trainer.state_dict(), path)
        return f"Vec3 weight pack with the trained codebook: {path}"

    def leaf_error(codec, vbatches, val):
        return {}, [], [leaf_error_line(codec, vbatches)]

    return run_training(args, SPEC, build, export=export if args.export_pack else None,
                        after_validation=leaf_error if args.report_leaf_error else None)


def main(argv=None):
    parser = argparse.ArgumentParser(description="EMA codebook training of the Vec3 VQ-VAE on MI355X.")
    sub = parser.add_subparsers(dest="command", required=True)
    p = sub.add_parser("train", help="Train the codebook (encoder/decoder frozen).")
    p.add_argument("--pack", required=True, help="Vec3 VQWPACK1 weight pack (VQVAE(3, 64, K) state_dict)")
    p.add_argument("--data_dir", type=str, default=None, help="Directory with .npy leaf arrays [N,8,8,8,3]; synthetic leaves if omitted.")
    p.add_argument("--synthetic_leaves", type=int, default=65536, help="synthetic mode: leaves in the dataset (before the split)")
    p.add_argument("--epochs", type=int, default=50)                      # notebook_vec3f.ipynb EPOCHS
    p.add_argument("--batch_size", type=int, default=1024, help="leaves per rank per step (notebook_vec3f.ipynb BATCH_SIZE)")
    p.add_argument("--commitment_cost", type=float, default=0.25)
    p.add_argument("--decay", type=float, default=0.95)
    p.add_argument("--eps", type=float, default=1e-4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log_every", type=int, default=100)
    p.add_argument("--model_path", type=str, default="models/vec3_quantizer.npz")
    p.add_argument("--resume", type=str, default=None, help="checkpoint (.npz written as --model_path) to continue from")
    p.add_argument("--export-pack", dest="export_pack", action="store_true",
                   help="also write <model_path>_final.vqw: the input pack with the trained quantizer.embedding")
    p.add_argument("--report-leaf-error", dest="report_leaf_error", action="store_true",
                   help="after each validation also print the per-leaf largest reconstruction error (median, 99th percentile, worst leaf)")
    p.add_argument("--backend", type=str, default="nccl", help="torch.distributed backend (nccl = RCCL)")
    p.add_argument("--single_gpu_rehearsal", action="store_true", help="tests: every rank on cuda:0 (use with --backend gloo)")
    p.set_defaults(func=train)
    args = parser.parse_args(argv)
    return args.func(args)


if __name__ == "__main__":
    main()
    sys.exit(0)
