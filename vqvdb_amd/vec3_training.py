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
import time
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from vqvdb_amd.codebook_training import allreduce_stats, dead_code_reset
from vqvdb_amd.codec import HipVec3Codec

D = 64
DEAD_CODE_RESET_INTERVAL = 5     # training.py:120
SUBSAMPLE = 12                   # notebook_vec3f.ipynb: every 12th leaf
TRAIN_FRACTION = 0.5             # notebook_vec3f.ipynb: 50 % / 50 % random_split


def stats_floats(k: int) -> int:
    return 66 * k + 1


def metrics_from_stats(stats: np.ndarray, k: int, commitment_cost: float = 0.25) -> dict:
    """vq_loss = commitment_cost * mse(z, quantized) (VQVAE_v2.py:146), perplexity (:153-154) and codes used, from an
    (all-reduced) statistics buffer [66K+1]."""
    stats = np.asarray(stats, dtype=np.float64)
    if stats.size != stats_floats(k):
        raise ValueError(f"stats has {stats.size} values, expected 66*K+1 = {stats_floats(k)}")
    rows = stats[66 * k]
    counts = stats[:k]
    if rows <= 0:
        return {"rows": 0, "vq_loss": 0.0, "perplexity": 1.0, "codes_used": 0}
    p = counts / rows
    return {"rows": int(rows), "vq_loss": float(commitment_cost * stats[65 * k:66 * k].sum() / (rows * D)),
            "perplexity": float(np.exp(-(p * np.log(p + 1e-10)).sum())), "codes_used": int((counts > 0).sum())}


def _leaves_arg(leaves: torch.Tensor) -> tuple[torch.Tensor, int]:
    leaves = leaves.contiguous()
    if leaves.dtype != torch.float32 or leaves.numel() % 1536:
        raise ValueError("vec3 leaves must be float32 with 512 x 3 values per leaf ([n,512,3] or [n,8,8,8,3])")
    return leaves, leaves.numel() // 1536


class Vec3CodebookTrainer:
    """Drives vqhip_vec3_train_* for one rank.  `codec` is a vqvdb_amd.codec.HipVec3Codec on this rank's device."""

    def __init__(self, codec, commitment_cost: float = 0.25, decay: float = 0.95, eps: float = 1e-4, group=None,
                 cluster_size: Optional[np.ndarray] = None, embed_avg: Optional[np.ndarray] = None, device: str = "cuda"):
        HipVec3Codec.check_ema(decay, eps)
        self.codec, self.group = codec, group
        self.commitment_cost, self.decay, self.eps = commitment_cost, decay, eps
        self.device = torch.device(device)
        self.k = codec.model_info()["num_codes"]
        codec.train_begin(cluster_size, embed_avg)
        self.stats = torch.zeros(stats_floats(self.k), dtype=torch.float32, device=self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.latent = None   # flat encoder outputs [n*64, 64] of the last step that asked for them (dead-code reset input)

    def step(self, leaves: torch.Tensor, keep_latent: bool = False, want_metrics: bool = True) -> Optional[dict]:
        """One EMA step on this rank's batch (float32 [n,512,3] or [n,8,8,8,3], resident on the device)."""
        leaves, n = _leaves_arg(leaves)
        # a NULL stream means the codec's own stream, so torch's default (null) stream cannot be handed over: run on a side
        # stream ordered after the producer of `leaves` and before later consumers
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        out = None
        with torch.cuda.stream(self.stream):
            zptr = 0
            if keep_latent:
                if self.latent is None or self.latent.shape[0] != n * 64:
                    self.latent = torch.empty((n * 64, D), dtype=torch.float32, device=self.device)
                zptr = self.latent.data_ptr()
            h = self.stream.cuda_stream
            self.codec.train_vq_stats_device(leaves.data_ptr(), n, self.stats.data_ptr(), latent_ptr=zptr, stream=h)
            allreduce_stats(self.stats, self.group)
            self.codec.train_vq_update_device(self.stats.data_ptr(), self.decay, self.eps, stream=h)
            if want_metrics:
                out = metrics_from_stats(self.stats.cpu().numpy(), self.k, self.commitment_cost)
        leaves.record_stream(self.stream)
        cur.wait_stream(self.stream)
        return out

    def evaluate(self, leaves: torch.Tensor, mse_weight: float = 0.8, l1_weight: float = 0.2) -> dict:
        """Validation forward (training.py:183-199): reconstruction MSE / L1 (and the reference's 0.8 / 0.2 mix), vq_loss and
        perplexity over the GLOBAL batch; nothing is updated."""
        leaves, n = _leaves_arg(leaves)
        nf = stats_floats(self.k)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            buf = torch.zeros(nf + 3, dtype=torch.float32, device=self.device)
            self.codec.train_eval_device(leaves.data_ptr(), n, buf.data_ptr(), buf[nf:].data_ptr(), stream=self.stream.cuda_stream)
            allreduce_stats(buf, self.group)
            host = buf.cpu().numpy().astype(np.float64)
        leaves.record_stream(self.stream)
        cur.wait_stream(self.stream)
        out = metrics_from_stats(host[:nf], self.k, self.commitment_cost)
        sq, ab, elems = host[nf:]
        out.update(recon_mse=float(sq / max(elems, 1.0)), recon_l1=float(ab / max(elems, 1.0)))
        out["recon_error"] = mse_weight * out["recon_mse"] + l1_weight * out["recon_l1"]
        return out

    def reset_dead_codes(self, flat_z: Optional[torch.Tensor] = None, threshold: float = 1.0, generator=None) -> int:
        """check_and_reset_dead_codes (VQVAE_v2.py:382-417) on the kept encoder outputs (or `flat_z` [rows, 64])."""
        flat_z = self.latent if flat_z is None else flat_z
        if flat_z is None:
            raise ValueError("no encoder outputs kept: call step(..., keep_latent=True) first or pass flat_z")
        st = {k: torch.from_numpy(v).to(self.device) for k, v in self.codec.train_get_state().items()}
        n = dead_code_reset(st, flat_z, threshold, generator, self.group)
        if n:
            self.codec.train_set_state(**{k: v.cpu().numpy() for k, v in st.items()})
        return n

    def state_dict(self) -> dict:
        """quantizer.* buffers in the reference's state_dict naming (VQVAE_v2.py:103-105)."""
        return {f"quantizer.{k}": v for k, v in self.codec.train_get_state().items()}

    def load_state_dict(self, sd: dict):
        self.codec.train_set_state(embedding=sd["quantizer.embedding"], cluster_size=sd["quantizer.cluster_size"],
                                   embed_avg=sd["quantizer.embed_avg"])


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


def split_train_val(n: int, seed: int):
    perm = np.random.default_rng(seed).permutation(n)
    n_train = int(TRAIN_FRACTION * n)
    return perm[:n_train], perm[n_train:]


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
    from vqvdb_amd.sharding import shard_range
    distributed = "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if distributed and not dist.is_initialized():
        dist.init_process_group(args.backend, **({"device_id": torch.device("cuda", local)} if args.backend == "nccl" else {}))
    if args.single_gpu_rehearsal:
        local = 0
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    log = (lambda *a: print(*a, flush=True)) if rank == 0 else (lambda *a: None)

    codec = HipVec3Codec(args.pack, device_id=local)
    trainer = Vec3CodebookTrainer(codec, commitment_cost=args.commitment_cost, decay=args.decay, eps=args.eps, device=str(device))
    leaves = load_leaves(args.data_dir, args.synthetic_leaves, args.seed)
    tr_ids, va_ids = split_train_val(len(leaves), args.seed)
    gb = args.batch_size * world
    steps_per_epoch = len(tr_ids) // gb
    if steps_per_epoch < 1:
        raise SystemExit(f"training set of {len(tr_ids)} leaves is smaller than one global batch ({world} x {args.batch_size}); lower --batch_size")
    if len(va_ids) < world:
        raise SystemExit(f"validation set of {len(va_ids)} leaves cannot give each of the {world} ranks a leaf")
    log(f"Dataset: {len(leaves)} leaves, train {len(tr_ids)}, val {len(va_ids)}; {world} rank(s) x batch {args.batch_size}")

    def shard(ids, step):
        lo, hi = shard_range(gb, rank, world)
        return ids[step * gb + lo: step * gb + hi]

    d_all = torch.from_numpy(np.ascontiguousarray(leaves)).to(device)
    best_val, history, start_epoch = float("inf"), [], 0
    if args.resume:
        ck = dict(np.load(args.resume))
        start_epoch = int(ck.pop("epoch", 0))
        best_val = float(ck.pop("best_val_loss", best_val))
        trainer.load_state_dict(ck)
        log(f"Resumed from {args.resume} at epoch {start_epoch}")
    os.makedirs(os.path.dirname(os.path.abspath(args.model_path)) or ".", exist_ok=True)
    for epoch in range(start_epoch, args.epochs):
        order = np.random.default_rng(args.seed + 1 + epoch).permutation(tr_ids)   # shuffle=True
        t0 = time.perf_counter()
        last = None
        for step in range(steps_per_epoch):
            batch = d_all[torch.from_numpy(shard(order, step)).to(device)]
            want = (step % args.log_every == 0) or step == steps_per_epoch - 1
            m = trainer.step(batch, keep_latent=(step == 0), want_metrics=want)
            if m is not None:
                last = m
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        if (epoch + 1) % DEAD_CODE_RESET_INTERVAL == 0:
            n_dead = trainer.reset_dead_codes()
            if n_dead:
                log(f"INFO: Resetting {n_dead} dead codes.")
        val = {"recon_error": 0.0, "vq_loss": 0.0, "recon_mse": 0.0, "recon_l1": 0.0}
        n_val = max(len(va_ids) // gb, 1)
        vbatches = []
        for step in range(n_val):
            ids = shard(va_ids, step) if len(va_ids) >= gb else va_ids[rank::world]
            vbatch = d_all[torch.from_numpy(ids).to(device)]
            mv = trainer.evaluate(vbatch)
            for k in val:
                val[k] += mv[k] / n_val
            if args.report_leaf_error:
                vbatches.append(vbatch)
        val_loss = val["recon_error"] + val["vq_loss"]
        rec = {"epoch": epoch + 1, "train_vq_loss": last["vq_loss"], "perplexity": last["perplexity"], "codes_used": last["codes_used"],
               "val_loss": val_loss, **{f"val_{k}": v for k, v in val.items()}, "leaves_per_s": steps_per_epoch * gb / dt, "epoch_s": dt}
        history.append(rec)
        log(f"Epoch {epoch + 1:02d}/{args.epochs} | Train VQ: {last['vq_loss']:.6f} | Val Loss: {val_loss:.6f} | "
            f"Perplexity: {last['perplexity']:.2f} | {rec['leaves_per_s'] / 1e3:.1f} k leaves/s ({dt:.2f} s/epoch)")
        if args.report_leaf_error:
            log(leaf_error_line(codec, vbatches))
        if val_loss < best_val and rank == 0:
            best_val = val_loss
            np.savez(args.model_path, epoch=epoch + 1, best_val_loss=best_val, **trainer.state_dict())
            log(f"New best validation loss: {val_loss:.6f} - model saved.")
    if rank == 0:
        root, ext = os.path.splitext(args.model_path)
        sd = trainer.state_dict()
        np.savez(root + "_final" + (ext or ".npz"), epoch=args.epochs, **sd)
        if args.export_pack:
            export_pack(args.pack, sd, root + "_final.vqw")
            log(f"Vec3 weight pack with the trained codebook: {root}_final.vqw")
    log("Training completed!")
    codec.close()
    return {"history": history, "best_val_loss": best_val, "steps_per_epoch": steps_per_epoch, "world": world}


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
