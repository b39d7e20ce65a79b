#!/usr/bin/env python3
"""Full training of the Vec3 model VQVAE(3, 64, K) on the HIP backend — the Vec3 counterpart of
full_training.py + train_codebook.py --mode full.

The device work is in libvqvdb_hip.so (vqhip_vec3_fulltrain_*, include/vqvdb_hip_vec3_fulltrain.h): forward, backward of
0.8 mse + 0.2 l1 + vq_loss, AdamW and the EMA codebook update of the reference loop (python/training.py), in fp32.  Per
step and rank:

    grads, aux = fwdbwd(local batch, means over the global batch)     (HIP kernels, deterministic)
    all_reduce(grads), all_reduce(aux)                                (SUM; the only collectives)
    apply: AdamW, EMA update, weight-table rebuild                    (HIP kernels, identical on every rank)

Epoch driver (one process per GPU, or under torch.distributed.run):

    python -m vqvdb_amd.vec3_full_training train --pack vec3.vqw --model_path out/vec3_model.npz [--data_dir DIR] [--export-pack]

Data and the rest of the loop as vec3_training.py (the notebook's every-12th-leaf subsampling and 50 % split, synthetic
synth_vec3 leaves without a directory): shuffled batches of 1024 leaves per rank, LR 5e-4 with cosine annealing over all
steps (T_max = epochs x steps per epoch, stepped on the host), a dead-code reset every 5 epochs from the first batch's
latent, validation, a best-validation checkpoint and a final save.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from vqvdb_amd.codebook_training import allreduce_stats
from vqvdb_amd.codec import HipVec3Codec
from vqvdb_amd.full_training import cosine_lr
from vqvdb_amd.vec3_training import (DEAD_CODE_RESET_INTERVAL, Vec3CodebookTrainer, _leaves_arg, leaf_error_line, load_leaves, metrics_from_stats,
                                     split_train_val, stats_floats)

D = 64
MSE_WEIGHT, L1_WEIGHT = 0.8, 0.2


def losses_from_aux(aux: np.ndarray, k: int, commitment_cost: float = 0.25) -> dict:
    """loss, recon (0.8 mse + 0.2 l1), mse, l1, vq_loss, perplexity and codes used from an (all-reduced) aux buffer [66K+4]."""
    aux = np.asarray(aux, np.float64)
    nf = stats_floats(k)
    out = metrics_from_stats(aux[:nf], k, commitment_cost)
    sq, ab, elems = aux[nf:nf + 3]
    out["mse"] = float(sq / max(elems, 1.0))
    out["l1"] = float(ab / max(elems, 1.0))
    out["recon"] = MSE_WEIGHT * out["mse"] + L1_WEIGHT * out["l1"]
    out["loss"] = out["recon"] + out["vq_loss"]
    return out


class Vec3FullTrainer:
    """Drives vqhip_vec3_fulltrain_* for one rank.  `codec` is a vqvdb_amd.codec.HipVec3Codec on this rank's device."""

    def __init__(self, codec, lr: float = 5e-4, betas=(0.9, 0.999), adam_eps: float = 1e-8, weight_decay: float = 1e-4,
                 decay: float = 0.95, eps: float = 1e-4, group=None, device: str = "cuda", commitment_cost: float = 0.25):
        HipVec3Codec.check_ema(decay, eps)
        HipVec3Codec.check_adamw(lr, 1, betas, adam_eps, weight_decay)
        self.codec, self.group = codec, group
        self.lr, self.betas, self.adam_eps, self.weight_decay = lr, tuple(betas), adam_eps, weight_decay
        self.decay, self.eps, self.commitment_cost = decay, eps, commitment_cost
        self.device = torch.device(device)
        self.k = codec.model_info()["num_codes"]
        codec.fulltrain_begin()
        self.np = codec.fulltrain_param_count()
        self.naux = codec.fulltrain_aux_floats()
        self.grads = torch.zeros(self.np, dtype=torch.float32, device=self.device)
        self.aux = torch.zeros(self.naux, dtype=torch.float32, device=self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.step_count = 0
        self.sched_t, self.t_max = 0, None   # scheduler position (host cosine annealing when t_max is set)
        self.latent = None

    def _world(self) -> int:
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def current_lr(self) -> float:
        return self.lr if self.t_max is None else cosine_lr(self.lr, self.sched_t, self.t_max)

    def step(self, leaves: torch.Tensor, n_global: Optional[int] = None, keep_latent: bool = False, want_metrics: bool = True,
             lr: Optional[float] = None) -> Optional[dict]:
        """One optimizer step on this rank's batch (float32 [n,512,3] or [n,8,8,8,3] on the device).  n_global defaults to
        the all-reduced sum of the ranks' n.  -> loss, recon, vq_loss, perplexity (global batch, before the update)."""
        leaves, n = _leaves_arg(leaves)
        if n_global is None:
            t = torch.tensor([n], dtype=torch.int64)
            if self._world() > 1:
                dist.all_reduce(t, group=self.group)
            n_global = int(t.item())
        lr = self.current_lr() if lr is None else lr
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
            self.codec.fulltrain_fwdbwd_device(leaves.data_ptr(), n, n_global, self.grads.data_ptr(), self.aux.data_ptr(), zptr, stream=h)
            allreduce_stats(self.grads, self.group)
            allreduce_stats(self.aux, self.group)
            self.step_count += 1
            self.codec.fulltrain_apply_device(self.grads.data_ptr(), self.aux.data_ptr(), lr, self.step_count, self.betas, self.adam_eps,
                                              self.weight_decay, self.decay, self.eps, stream=h)
            if want_metrics:
                out = losses_from_aux(self.aux.cpu().numpy(), self.k, self.commitment_cost)
                out["lr"] = lr
        leaves.record_stream(self.stream)
        cur.wait_stream(self.stream)
        if self.t_max is not None:
            self.sched_t += 1
        return out

    def evaluate(self, leaves: torch.Tensor) -> dict:
        """Validation forward in eval mode (training.py:183-199) on the live model: recon (0.8 mse + 0.2 l1), mse, l1, vq_loss,
        perplexity over the global batch; nothing is updated."""
        # the stage-1 eval forward runs the handle's live tables, which apply rebuilds from the trained parameters
        return Vec3CodebookTrainer.evaluate(self, leaves)

    def reset_dead_codes(self, flat_z: Optional[torch.Tensor] = None, threshold: float = 1.0, generator=None) -> int:
        """check_and_reset_dead_codes (VQVAE_v2.py:382-417) on the kept latent (or `flat_z` [rows, 64])."""
        return Vec3CodebookTrainer.reset_dead_codes(self, flat_z, threshold, generator)

    def state_dict(self) -> dict:
        """The model in the reference's state_dict naming: every parameter and the quantizer buffers."""
        sd = vec_to_state(self.codec.fulltrain_get_params())
        sd.update({f"quantizer.{k}": v for k, v in self.codec.train_get_state().items()})
        return sd

    def load_state_dict(self, sd: dict):
        self.codec.fulltrain_set_params(state_to_vec(sd))
        self.codec.train_set_state(embedding=sd["quantizer.embedding"], cluster_size=sd["quantizer.cluster_size"],
                                   embed_avg=sd["quantizer.embed_avg"])

    def checkpoint(self) -> dict:
        """Everything a bit-exact resume needs: parameters, both Adam moments, step, EMA buffers, scheduler position."""
        m, v = self.codec.fulltrain_get_opt_state()
        ck = {"params": self.codec.fulltrain_get_params(), "exp_avg": m, "exp_avg_sq": v, "step": np.int64(self.step_count),
              "sched_t": np.int64(self.sched_t), "t_max": np.int64(-1 if self.t_max is None else self.t_max)}
        ck.update({f"quantizer.{k}": val for k, val in self.codec.train_get_state().items()})
        return ck

    def load_checkpoint(self, ck: dict):
        self.codec.fulltrain_set_params(ck["params"])
        self.codec.fulltrain_set_opt_state(ck["exp_avg"], ck["exp_avg_sq"])
        self.codec.train_set_state(embedding=ck["quantizer.embedding"], cluster_size=ck["quantizer.cluster_size"],
                                   embed_avg=ck["quantizer.embed_avg"])
        self.step_count = int(ck["step"])
        self.sched_t = int(ck["sched_t"])
        self.t_max = None if int(ck["t_max"]) < 0 else int(ck["t_max"])

    def finish(self):
        """Wait for the device; the handle then encodes / decodes with the trained model."""
        torch.cuda.synchronize(self.device)


# ---- flat vector <-> state_dict ----------------------------------------------------------------------------------------
def _param_specs() -> list:
    """(name, shape) of the 60 tensors of model.parameters() in order (the flat vector's layout)."""
    s = []
    conv = lambda p, co, ci, k: s.extend([(p + ".weight", (co, ci, k, k, k)), (p + ".bias", (co,))])  # noqa: E731
    gn = lambda p, c: s.extend([(p + ".weight", (c,)), (p + ".bias", (c,))])  # noqa: E731

    def rb(p, c):
        gn(p + ".gn1", c), conv(p + ".conv1", c, c, 3), gn(p + ".gn2", c), conv(p + ".conv2", c, c, 3)

    conv("encoder.pre.0", 64, 3, 3), gn("encoder.pre.1", 64), rb("encoder.pre.3", 64), conv("encoder.down1", 128, 64, 3)
    rb("encoder.res_stack.0", 128), rb("encoder.res_stack.1", 128)
    s.extend([("encoder.attn.fc.0.weight", (32, 128)), ("encoder.attn.fc.2.weight", (128, 32))])
    conv("encoder.proj", 64, 128, 1), conv("decoder.stem.0", 128, 64, 3), gn("decoder.stem.1", 128)
    rb("decoder.res_stack.0", 128), rb("decoder.res_stack.1", 128)
    s.extend([("decoder.attn.fc.0.weight", (32, 128)), ("decoder.attn.fc.2.weight", (128, 32))])
    conv("decoder.up_conv", 256, 128, 3), conv("decoder.final", 3, 32, 3)
    return s


PARAM_SPECS = _param_specs()


def vec_to_state(vec: np.ndarray) -> dict:
    out, off = {}, 0
    for name, shape in PARAM_SPECS:
        size = int(np.prod(shape))
        out[name] = np.asarray(vec[off:off + size], np.float32).reshape(shape).copy()
        off += size
    if off != len(vec):
        raise ValueError(f"parameter vector has {len(vec)} values, the Vec3 model has {off}")
    return out


def state_to_vec(sd: dict) -> np.ndarray:
    return np.concatenate([np.asarray(sd[name], np.float32).reshape(-1) for name, _ in PARAM_SPECS])


def export_pack(pack_path: str, state: dict, out_path: str):
    """The source pack with every trained parameter and the quantizer buffers replaced (VQWPACK1, HipVec3Codec loads it)."""
    from vqvdb_amd import weightpack
    t = dict(weightpack.load(pack_path))
    for k, v in state.items():
        if k in t or k.startswith("quantizer."):
            t[k] = np.ascontiguousarray(v, dtype=np.float32)
    weightpack.save(out_path, t)


def eval_roundtrip(codec, leaves: torch.Tensor) -> dict:
    """decode(encode(leaves)) of this rank's batch in the handle's current precision mode: reconstruction MSE and L1."""
    leaves = leaves.contiguous()
    n = leaves.shape[0]
    idx = torch.empty((n, 64), dtype=torch.int16, device=leaves.device)
    out = torch.empty((n, 512, 3), dtype=torch.float32, device=leaves.device)
    st = torch.cuda.current_stream(leaves.device)
    if st.cuda_stream == 0:   # a null handle means the codec's own stream: order it after the producer of `leaves` by hand
        torch.cuda.synchronize(leaves.device)
    codec.encode_device(leaves.data_ptr(), n, idx.data_ptr(), st.cuda_stream)
    codec.decode_device(idx.data_ptr(), n, out.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize(leaves.device)
    d = out - leaves.reshape(n, 512, 3)
    return {"recon_mse": float((d * d).mean()), "recon_l1": float(d.abs().mean())}


# ---- epoch driver ------------------------------------------------------------------------------------------------------
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
    trainer = Vec3FullTrainer(codec, lr=args.lr, weight_decay=args.weight_decay, decay=args.decay, eps=args.eps, device=str(device))
    leaves = load_leaves(args.data_dir, args.synthetic_leaves, args.seed)
    tr_ids, va_ids = split_train_val(len(leaves), args.seed)
    gb = args.batch_size * world
    steps_per_epoch = len(tr_ids) // gb
    if steps_per_epoch < 1:
        raise SystemExit(f"training set of {len(tr_ids)} leaves is smaller than one global batch ({world} x {args.batch_size}); lower --batch_size")
    if len(va_ids) < world:
        raise SystemExit(f"validation set of {len(va_ids)} leaves cannot give each of the {world} ranks a leaf")
    trainer.t_max = args.epochs * steps_per_epoch
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
        trainer.load_checkpoint(ck)
        log(f"Resumed from {args.resume} at epoch {start_epoch}")
    os.makedirs(os.path.dirname(os.path.abspath(args.model_path)) or ".", exist_ok=True)
    for epoch in range(start_epoch, args.epochs):
        order = np.random.default_rng(args.seed + 1 + epoch).permutation(tr_ids)   # shuffle=True
        t0 = time.perf_counter()
        total, last = 0.0, None
        for step in range(steps_per_epoch):
            batch = d_all[torch.from_numpy(shard(order, step)).to(device)]
            want = (step % args.log_every == 0) or step == steps_per_epoch - 1
            m = trainer.step(batch, n_global=gb, keep_latent=(step == 0), want_metrics=True)
            total += m["loss"]
            if want:
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
        if args.eval_precision == "bf16":   # the same validation batches through encode / decode in bf16-operand mode
            vb = {"recon_mse": 0.0, "recon_l1": 0.0}
            codec.precision = "bf16"
            for step in range(n_val):
                ids = shard(va_ids, step) if len(va_ids) >= gb else va_ids[rank::world]
                for k, v in eval_roundtrip(codec, d_all[torch.from_numpy(ids).to(device)]).items():
                    vb[k] += v / n_val
            codec.precision = "fp32"
            vb["recon_error"] = 0.8 * vb["recon_mse"] + 0.2 * vb["recon_l1"]
        rec = {"epoch": epoch + 1, "train_loss": total / steps_per_epoch, "train_vq_loss": last["vq_loss"], "perplexity": last["perplexity"],
               "codes_used": last["codes_used"], "val_loss": val_loss, **{f"val_{k}": v for k, v in val.items()},
               "leaves_per_s": steps_per_epoch * gb / dt, "epoch_s": dt, "lr": last["lr"]}
        if args.eval_precision == "bf16":
            rec.update({f"val_bf16_{k}": v for k, v in vb.items()})
            log(f"         | Val recon fp32: {val['recon_error']:.6f} | Val recon bf16 inference: {vb['recon_error']:.6f}")
        history.append(rec)
        log(f"Epoch {epoch + 1:02d}/{args.epochs} | Train Loss: {rec['train_loss']:.6f} | Val Loss: {val_loss:.6f} | "
            f"Perplexity: {last['perplexity']:.2f} | {rec['leaves_per_s'] / 1e3:.1f} k leaves/s ({dt:.2f} s/epoch)")
        if args.report_leaf_error:
            log(leaf_error_line(codec, vbatches))
        if val_loss < best_val and rank == 0:
            best_val = val_loss
            np.savez(args.model_path, epoch=epoch + 1, best_val_loss=best_val, **trainer.checkpoint())
            log(f"New best validation loss: {val_loss:.6f} - model saved.")
    trainer.finish()
    if rank == 0:
        root, ext = os.path.splitext(args.model_path)
        np.savez(root + "_final" + (ext or ".npz"), epoch=args.epochs, **trainer.checkpoint())
        if args.export_pack:
            export_pack(args.pack, trainer.state_dict(), root + "_final.vqw")
            log(f"Vec3 weight pack with the trained model: {root}_final.vqw")
    log("Training completed!")
    codec.close()
    return {"history": history, "best_val_loss": best_val, "steps_per_epoch": steps_per_epoch, "world": world}


def main(argv=None):
    parser = argparse.ArgumentParser(description="Full training of the Vec3 VQ-VAE on MI355X.")
    sub = parser.add_subparsers(dest="command", required=True)
    p = sub.add_parser("train", help="Train the whole model (encoder, decoder, codebook).")
    p.add_argument("--pack", required=True, help="Vec3 VQWPACK1 weight pack (VQVAE(3, 64, K) state_dict): the starting model")
    p.add_argument("--data_dir", type=str, default=None, help="Directory with .npy leaf arrays [N,8,8,8,3]; synthetic leaves if omitted.")
    p.add_argument("--synthetic_leaves", type=int, default=65536, help="synthetic mode: leaves in the dataset (before the split)")
    p.add_argument("--epochs", type=int, default=50)                      # notebook_vec3f.ipynb EPOCHS
    p.add_argument("--batch_size", type=int, default=1024, help="leaves per rank per step (notebook_vec3f.ipynb BATCH_SIZE)")
    p.add_argument("--lr", type=float, default=5e-4)                      # notebook_vec3f.ipynb LR
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--decay", type=float, default=0.95)
    p.add_argument("--eps", type=float, default=1e-4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log_every", type=int, default=100)
    p.add_argument("--model_path", type=str, default="models/vec3_model.npz")
    p.add_argument("--resume", type=str, default=None, help="checkpoint (.npz written as --model_path) to continue from")
    p.add_argument("--export-pack", dest="export_pack", action="store_true",
                   help="also write <model_path>_final.vqw: the input pack with the trained parameters and codebook")
    p.add_argument("--eval-precision", dest="eval_precision", choices=("fp32", "bf16"), default="fp32",
                   help="bf16: after each epoch also report the validation reconstruction sums of the bf16-operand inference mode (training stays fp32)")
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
