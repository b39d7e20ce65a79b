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
import sys
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from vqvdb_amd.codec import HipVec3Codec
from vqvdb_amd.full_training import cosine_lr
from vqvdb_amd.training_common import LoopSpec, TrainerBase, allreduce_stats, recon_metrics, run_training, split_train_val
from vqvdb_amd.vec3_training import TRAIN_FRACTION, leaf_error_line, load_leaves, metrics_from_stats, stats_floats

D = 64
SPEC = LoopSpec(train_loss="mean", pass_n_global=True, record_lr=True, final_checkpoint=True)


def losses_from_aux(aux: np.ndarray, k: int, commitment_cost: float = 0.25) -> dict:
    """loss, recon (0.8 mse + 0.2 l1), mse, l1, vq_loss, perplexity and codes used from an (all-reduced) aux buffer [66K+4]."""
    aux = np.asarray(aux, np.float64)
    nf = stats_floats(k)
    out = metrics_from_stats(aux[:nf], k, commitment_cost)
    out["mse"], out["l1"], out["recon"] = recon_metrics(aux[nf:nf + 3])
    out["loss"] = out["recon"] + out["vq_loss"]
    return out


class Vec3FullTrainer(TrainerBase):
    """Drives vqhip_vec3_fulltrain_* for one rank.  `codec` is a vqvdb_amd.codec.HipVec3Codec on this rank's device.
    evaluate() is the stage-1 eval forward: it runs the handle's live tables, which apply rebuilds from the trained parameters."""
    leaf_values, d = 1536, D

    def __init__(self, codec, lr: float = 5e-4, betas=(0.9, 0.999), adam_eps: float = 1e-8, weight_decay: float = 1e-4,
                 decay: float = 0.95, eps: float = 1e-4, group=None, device: str = "cuda", commitment_cost: float = 0.25):
        HipVec3Codec.check_adamw(lr, 1, betas, adam_eps, weight_decay)
        super().__init__(codec, commitment_cost, decay, eps, group, device)
        self.lr, self.betas, self.adam_eps, self.weight_decay = lr, tuple(betas), adam_eps, weight_decay
        self.k = codec.model_info()["num_codes"]
        codec.fulltrain_begin()
        self.np = codec.fulltrain_param_count()
        self.naux = codec.fulltrain_aux_floats()
        self.grads = torch.zeros(self.np, dtype=torch.float32, device=self.device)
        self.aux = torch.zeros(self.naux, dtype=torch.float32, device=self.device)
        self.step_count = 0
        self.sched_t, self.t_max = 0, None   # scheduler position (host cosine annealing when t_max is set)

    def current_lr(self) -> float:
        return self.lr if self.t_max is None else cosine_lr(self.lr, self.sched_t, self.t_max)

    def step(self, leaves: torch.Tensor, n_global: Optional[int] = None, keep_latent: bool = False, want_metrics: bool = True,
             lr: Optional[float] = None) -> Optional[dict]:
        """One optimizer step on this rank's batch (float32 [n,512,3] or [n,8,8,8,3] on the device).  n_global defaults to
        the all-reduced sum of the ranks' n.  -> loss, recon, vq_loss, perplexity (global batch, before the update)."""
        leaves, n = self._leaves_arg(leaves)
        if n_global is None:
            t = torch.tensor([n], dtype=torch.int64)
            if self._world() > 1:
                dist.all_reduce(t, group=self.group)
            n_global = int(t.item())
        lr = self.current_lr() if lr is None else lr
        out = None
        with self._side_stream(leaves) as h:
            zptr = self._latent_ptr(n, keep_latent)
            self.codec.fulltrain_fwdbwd_device(leaves.data_ptr(), n, n_global, self.grads.data_ptr(), self.aux.data_ptr(), zptr, stream=h)
            allreduce_stats(self.grads, self.group)
            allreduce_stats(self.aux, self.group)
            self.step_count += 1
            self.codec.fulltrain_apply_device(self.grads.data_ptr(), self.aux.data_ptr(), lr, self.step_count, self.betas, self.adam_eps,
                                              self.weight_decay, self.decay, self.eps, stream=h)
            if want_metrics:
                out = losses_from_aux(self.aux.cpu().numpy(), self.k, self.commitment_cost)
                out["lr"] = lr
        if self.t_max is not None:
            self.sched_t += 1
        return out

    def state_dict(self) -> dict:
        """The model in the reference's state_dict naming: every parameter and the quantizer buffers."""
        return {**vec_to_state(self.codec.fulltrain_get_params()), **super().state_dict()}

    def load_state_dict(self, sd: dict):
        self.codec.fulltrain_set_params(state_to_vec(sd))
        super().load_state_dict(sd)

    def checkpoint(self) -> dict:
        """Everything a bit-exact resume needs: parameters, both Adam moments, step, EMA buffers, scheduler position."""
        m, v = self.codec.fulltrain_get_opt_state()
        return {"params": self.codec.fulltrain_get_params(), "exp_avg": m, "exp_avg_sq": v, "step": np.int64(self.step_count),
                "sched_t": np.int64(self.sched_t), "t_max": np.int64(-1 if self.t_max is None else self.t_max), **super().state_dict()}

    def load_checkpoint(self, ck: dict):
        self.codec.fulltrain_set_params(ck["params"])
        self.codec.fulltrain_set_opt_state(ck["exp_avg"], ck["exp_avg_sq"])
        super().load_state_dict(ck)
        self.step_count = int(ck["step"])
        self.sched_t = int(ck["sched_t"])
        self.t_max = None if int(ck["t_max"]) < 0 else int(ck["t_max"])


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
    def build(local, device, world):
        codec = HipVec3Codec(args.pack, device_id=local)
        trainer = Vec3FullTrainer(codec, lr=args.lr, weight_decay=args.weight_decay, decay=args.decay, eps=args.eps, device=str(device))
        leaves = load_leaves(args.data_dir, args.synthetic_leaves, args.seed)
        tr_ids, va_ids = split_train_val(len(leaves), args.seed, TRAIN_FRACTION)
        trainer.t_max = args.epochs * (len(tr_ids) // (args.batch_size * world))   # cosine annealing over all steps
        return codec, trainer, leaves, tr_ids, va_ids

    def export(trainer, path):
        export_pack(args.pack, trainer.state_dict(), path)
        return f"Vec3 weight pack with the trained model: {path}"

    def extras(codec, vbatches, val):
        rec, before, after = {}, [], []
        if args.eval_precision == "bf16":   # the same validation batches through encode / decode in bf16-operand mode
            mse = l1 = 0.0
            codec.precision = "bf16"
            for vbatch in vbatches:
                r = eval_roundtrip(codec, vbatch)
                mse, l1 = mse + r["recon_mse"] / len(vbatches), l1 + r["recon_l1"] / len(vbatches)
            codec.precision = "fp32"
            rec = {"val_bf16_recon_mse": mse, "val_bf16_recon_l1": l1, "val_bf16_recon_error": 0.8 * mse + 0.2 * l1}
            before.append(f"         | Val recon fp32: {val['recon_error']:.6f} | Val recon bf16 inference: {rec['val_bf16_recon_error']:.6f}")
        if args.report_leaf_error:
            after.append(leaf_error_line(codec, vbatches))
        return rec, before, after

    return run_training(args, SPEC, build, export=export if args.export_pack else None,
                        after_validation=extras if args.eval_precision == "bf16" or args.report_leaf_error else None)


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
