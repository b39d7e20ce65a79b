#!/usr/bin/env python3
"""Epoch-level driver for codebook (EMA) training on the HIP backend — the quantizer part of the reference's
`train(args)` (python/training.py:47-258) and of BASELINE configs[4], one process per GPU:

    python -m vqvdb_amd.train_codebook train --pack model.vqw --model_path out/quantizer.npz [--data_dir DIR] ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m vqvdb_amd.train_codebook train ...

Same loop shape as the reference: 80/20 split (:77-81), per-epoch training pass over global batches of
`batch_size` leaves per rank, validation pass (:183-199), dead-code reset every 5 epochs from the first batch's
encoder outputs (:120,165-166,180-181), best-validation checkpoint (:216-233) and a final save (:252).  What is trained
is the codebook (EMA); encoder/decoder weights stay as loaded from the pack.  Data: `.npy` files of shape [N,8,8,8]
float32 like the reference's VDBLeafDataset (python/VQVAE_v2.py:21-66), or synthetic uniform leaves when no directory
is given.  Every rank holds its shard of each global batch in HBM; the only collective is the all-reduce of the
statistics buffer (RCCL).
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np

from vqvdb_amd.codebook_training import CodebookTrainer
from vqvdb_amd.full_training import FullTrainer
from vqvdb_amd.codec import HipCodec
from vqvdb_amd.training_common import LoopSpec, run_training, split_train_val

SUBSAMPLE = 6                    # training.py:72-73: every 6th leaf of the dataset
TRAIN_FRACTION = 0.8             # training.py:77-81
SPEC = LoopSpec(train_loss="last", rate_unit="M")


def load_leaves(data_dir, synthetic_leaves: int, seed: int) -> np.ndarray:
    """All leaves as float32 [N,512] (the reference subsamples every 6th block of its .npy files)."""
    if data_dir:
        files = sorted(glob.glob(os.path.join(data_dir, "*.npy")))
        if not files:
            raise ValueError(f"No .npy files found in {data_dir}")
        arrs = []
        for f in files:
            a = np.load(f, mmap_mode="r")
            if a.shape[1:] != (8, 8, 8):
                raise ValueError(f"File {f}: invalid shape {a.shape}. Expected suffix (8, 8, 8)")
            arrs.append(np.asarray(a[::SUBSAMPLE], dtype=np.float32).reshape(-1, 512))
        return np.concatenate(arrs)
    from vqvdb_amd import synth
    base = synth.make_leaves(min(synthetic_leaves, 65536), seed=seed)
    reps = -(-synthetic_leaves // len(base))
    return np.tile(base, (reps, 1))[:synthetic_leaves] if reps > 1 else base


def train(args) -> dict:
    full = args.mode == "full"

    def build(local, device, world):
        codec = HipCodec(args.pack, device_id=local)
        leaves = load_leaves(args.data_dir, args.leaves_per_epoch * 5 // 4, args.seed)
        tr_ids, va_ids = split_train_val(len(leaves), args.seed, TRAIN_FRACTION)
        if full:   # AdamW(lr, wd 1e-4, betas 0.9/0.999) + CosineAnnealingLR(T_max = epochs * steps) like training.py:104-108
            trainer = FullTrainer(codec, lr=args.lr, commitment_cost=args.commitment_cost, ema_decay=args.decay, ema_eps=args.eps,
                                  t_max=args.epochs * max(len(tr_ids) // (args.batch_size * world), 1), device=str(device))
        else:
            trainer = CodebookTrainer(codec, commitment_cost=args.commitment_cost, decay=args.decay, eps=args.eps, device=str(device))
        return codec, trainer, leaves, tr_ids, va_ids

    def export(trainer, path):
        # the role of the reference's scripted-model export (training.py:254-258): an inference artefact for this backend
        from vqvdb_amd import weightpack
        weightpack.save(path, {k: v for k, v in trainer.state_dict().items() if k not in ("quantizer.cluster_size", "quantizer.embed_avg")})

    # the best-validation checkpoint of full mode includes optimizer moments and step count (training.py:216-226), see FullTrainer.checkpoint
    return run_training(args, SPEC, build, export=export if full else None)


def main(argv=None):
    parser = argparse.ArgumentParser(description="EMA codebook training for the VQ-VAE leaf codec on MI355X.")
    sub = parser.add_subparsers(dest="command", required=True)
    p = sub.add_parser("train", help="Train the codebook (encoder/decoder frozen).")
    p.add_argument("--pack", required=True, help="VQWPACK1 weight pack (vqvdb_amd/weightpack.py)")
    p.add_argument("--mode", choices=("codebook", "full"), default="codebook",
                   help="codebook: EMA codebook only (encoder/decoder frozen); full: AdamW on every weight + EMA codebook (training.py)")
    p.add_argument("--lr", type=float, default=1e-4, help="full mode: AdamW learning rate (training.py:51)")
    p.add_argument("--data_dir", type=str, default=None, help="Directory with .npy leaf arrays [N,8,8,8]; synthetic leaves if omitted.")
    p.add_argument("--epochs", type=int, default=30)                      # training.py:50
    p.add_argument("--batch_size", type=int, default=2048, help="leaves per rank per step (training.py:49)")
    p.add_argument("--leaves_per_epoch", type=int, default=8_000_000, help="synthetic mode: training leaves per epoch (BASELINE configs[4])")
    p.add_argument("--commitment_cost", type=float, default=0.25)         # training.py:55
    p.add_argument("--decay", type=float, default=0.95)
    p.add_argument("--eps", type=float, default=1e-4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log_every", type=int, default=100)
    p.add_argument("--model_path", type=str, default="models/quantizer.npz")
    p.add_argument("--resume", type=str, default=None, help="checkpoint (.npz written as --model_path) to continue from")
    p.add_argument("--backend", type=str, default="nccl", help="torch.distributed backend (nccl = RCCL)")
    p.add_argument("--single_gpu_rehearsal", action="store_true", help="tests: every rank on cuda:0 (use with --backend gloo)")
    p.set_defaults(func=train)
    args = parser.parse_args(argv)
    return args.func(args)


if __name__ == "__main__":
    main()
    sys.exit(0)
