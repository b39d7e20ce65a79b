"""What the four training drivers share (scalar / Vec3, codebook / full): the readers of the statistics and reconstruction
sums, the collective and the dead-code reset, the trainer base class (argument checks, side stream, validation forward,
quantizer buffers, checkpoints) and the one epoch loop of python/training.py:47-258.  Nothing here belongs to one trainer only.
"""
from __future__ import annotations

import contextlib
import os
import time
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch
import torch.distributed as dist

from vqvdb_amd.sharding import shard_range

DEAD_CODE_RESET_INTERVAL = 5     # training.py:120
MSE_WEIGHT, L1_WEIGHT = 0.8, 0.2   # training.py:151-155


def stats_floats(k: int, d: int) -> int:
    """Statistics buffer of K codes of width D: encodings_sum [K], dw [K,D], |z-e|^2 per code [K], rows [1]."""
    return k + k * d + k + 1


def vq_metrics(stats: np.ndarray, k: int, d: int, commitment_cost: float = 0.25) -> dict:
    """vq_loss = commitment_cost * mse(z, quantized) (VQVAE_v2.py:146), perplexity (:153-154) and codes used, from an
    (all-reduced) statistics buffer."""
    stats = np.asarray(stats, dtype=np.float64)
    if stats.size != stats_floats(k, d):
        raise ValueError(f"stats has {stats.size} values, expected {d + 2}*K+1 = {stats_floats(k, d)}")
    rows, counts = stats[-1], stats[:k]
    if rows <= 0:
        return {"rows": 0, "vq_loss": 0.0, "perplexity": 1.0, "codes_used": 0}
    p = counts / rows
    return {"rows": int(rows), "vq_loss": float(commitment_cost * stats[k + k * d:-1].sum() / (rows * d)),
            "perplexity": float(np.exp(-(p * np.log(p + 1e-10)).sum())), "codes_used": int((counts > 0).sum())}


def recon_metrics(sums, mse_weight: float = MSE_WEIGHT, l1_weight: float = L1_WEIGHT) -> tuple:
    """(sum of squared errors, sum of absolute errors, elements) -> reconstruction MSE, L1 and the reference's mix of the two."""
    sq, ab, elems = sums
    mse, l1 = float(sq / max(elems, 1.0)), float(ab / max(elems, 1.0))
    return mse, l1, mse_weight * mse + l1_weight * l1


def allreduce_stats(stats: torch.Tensor, group=None) -> torch.Tensor:
    """Sum the per-rank statistics in place (no-op without an initialised process group)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=group)
    return stats


def dead_code_reset(state: dict, flat_z: torch.Tensor, threshold: float = 1.0, generator: Optional[torch.Generator] = None,
                    group=None, src: int = 0) -> int:
    """check_and_reset_dead_codes (VQVAE_v2.py:382-417): codes with cluster_size < threshold are re-sampled from the given
    encoder outputs (uniform row indices), their embed_avg set to the same rows and cluster_size to 1.  `state` holds torch
    tensors embedding [K,D], cluster_size [K], embed_avg [K,D] and is modified in place.  With a process group,
    rank `src` draws the samples and the three buffers are broadcast (the draw uses that rank's RNG)."""
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    n_dead = 0
    if not distributed or dist.get_rank(group) == src:
        dead = torch.where(state["cluster_size"] < threshold)[0]
        n_dead = int(dead.numel())
        if n_dead and flat_z.shape[0]:
            pick = torch.randint(0, flat_z.shape[0], (n_dead,), device=flat_z.device, generator=generator)
            new = flat_z[pick].to(state["embedding"].device, torch.float32)
            state["embedding"][dead] = new
            state["embed_avg"][dead] = new
            state["cluster_size"][dead] = 1.0
    if distributed:
        n = torch.tensor([n_dead], device=state["embedding"].device)
        dist.broadcast(n, src=src, group=group)
        n_dead = int(n.item())
        if n_dead:
            for k in ("embedding", "cluster_size", "embed_avg"):
                dist.broadcast(state[k], src=src, group=group)
    return n_dead


def leaves_arg(leaves: torch.Tensor, values: int) -> tuple[torch.Tensor, int]:
    """A batch of leaves as a contiguous tensor and its leaf count (`values` per leaf: 512 scalar, 512 x 3 Vec3)."""
    leaves = leaves.contiguous()
    if leaves.dtype != torch.float32 or leaves.numel() % values:
        raise ValueError("leaves must be float32 with 512 values per leaf" if values == 512 else
                         "vec3 leaves must be float32 with 512 x 3 values per leaf ([n,512,3] or [n,8,8,8,3])")
    return leaves, leaves.numel() // values


class TrainerBase:
    """One rank's trainer around a codec handle.  A subclass gives `leaf_values` (values per leaf), `d` (latent width) and
    `k` (codes; a class constant or set after __init__), its `step`, and what it adds to the state dict or checkpoint."""
    leaf_values: int
    d: int
    k: int

    def __init__(self, codec, commitment_cost: float, decay: float, eps: float, group, device: str):
        if not (0.0 <= decay <= 1.0):   # the argument checks come before the codec is touched
            raise ValueError(f"decay must be in [0, 1], got {decay}")
        if not eps > 0.0:
            raise ValueError(f"eps must be > 0, got {eps}")
        self.codec, self.group = codec, group
        self.commitment_cost, self.decay, self.eps = commitment_cost, decay, eps
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.latent = None   # flat encoder outputs [n*64, d] of the last step that asked for them (dead-code reset input)

    def _world(self) -> int:
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def _leaves_arg(self, leaves: torch.Tensor) -> tuple[torch.Tensor, int]:
        return leaves_arg(leaves, self.leaf_values)

    @contextlib.contextmanager
    def _side_stream(self, leaves: torch.Tensor):
        """The library treats a NULL stream as "use the codec's own stream", so torch's default (null) stream cannot be handed
        over: the body runs on a side stream ordered after the producer of `leaves` and before later consumers.  Yields the
        stream's handle."""
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield self.stream.cuda_stream
        leaves.record_stream(self.stream)
        cur.wait_stream(self.stream)

    def _latent_ptr(self, n: int, keep: bool) -> int:
        """Device pointer of the kept-latent buffer for n leaves (0: do not keep); call on the side stream."""
        if not keep:
            return 0
        if self.latent is None or self.latent.shape[0] != n * 64:
            self.latent = torch.empty((n * 64, self.d), dtype=torch.float32, device=self.device)
        return self.latent.data_ptr()

    def evaluate(self, leaves: torch.Tensor, mse_weight: float = MSE_WEIGHT, l1_weight: float = L1_WEIGHT) -> dict:
        """Validation forward on this rank's batch (training.py:183-199) with the handle's live tables: reconstruction MSE / L1
        (and the reference's 0.8 / 0.2 mix, :151-155), vq_loss and perplexity over the GLOBAL batch; nothing is updated."""
        leaves, n = self._leaves_arg(leaves)
        nf = stats_floats(self.k, self.d)
        with self._side_stream(leaves) as h:
            buf = torch.zeros(nf + 3, dtype=torch.float32, device=self.device)
            self.codec.train_eval_device(leaves.data_ptr(), n, buf.data_ptr(), buf[nf:].data_ptr(), stream=h)
            allreduce_stats(buf, self.group)
            host = buf.cpu().numpy().astype(np.float64)
        out = vq_metrics(host[:nf], self.k, self.d, self.commitment_cost)
        out["recon_mse"], out["recon_l1"], out["recon_error"] = recon_metrics(host[nf:], mse_weight, l1_weight)
        return out

    def reset_dead_codes(self, flat_z: Optional[torch.Tensor] = None, threshold: float = 1.0, generator=None) -> int:
        """check_and_reset_dead_codes (VQVAE_v2.py:382-417) on the kept encoder outputs (or `flat_z` [rows, d])."""
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
        """Resume from quantizer.* buffers saved by state_dict() or by the reference's checkpoints (training.py:216-233)."""
        self.codec.train_set_state(embedding=sd["quantizer.embedding"], cluster_size=sd["quantizer.cluster_size"],
                                   embed_avg=sd["quantizer.embed_avg"])

    def checkpoint(self) -> dict:
        """Everything a resumed run needs; a trainer with optimizer state adds it."""
        return self.state_dict()

    def load_checkpoint(self, ck: dict):
        self.load_state_dict(ck)

    def sync(self):
        torch.cuda.synchronize(self.device)

    def finish(self):
        """After the last step: wait for the device; a trainer whose inference tables need a rebuild does it here."""
        self.sync()


# ---- epoch loop --------------------------------------------------------------------------------------------------------
def split_train_val(n: int, seed: int, train_fraction: float):
    """Random train / validation split (training.py:77-81), identical on every rank."""
    perm = np.random.default_rng(seed).permutation(n)
    n_train = int(train_fraction * n)
    return perm[:n_train], perm[n_train:]


@dataclass(frozen=True)
class LoopSpec:
    """What differs between the drivers inside the epoch loop."""
    train_loss: Optional[str] = None   # record's train_loss: None = absent, "last" = the last logged step's loss (None without one),
    #                                    "mean" = metrics every step, their mean loss (also what the log line then shows)
    pass_n_global: bool = False        # step(..., n_global=global batch)
    record_lr: bool = False            # record carries the last logged step's lr
    rate_unit: str = "k"               # log line: "k" or "M" leaves/s
    final_checkpoint: bool = False     # the final .npz holds checkpoint() instead of state_dict()


def run_training(args, spec: LoopSpec, build: Callable, export: Optional[Callable] = None, after_validation: Optional[Callable] = None,
                 device=None) -> dict:
    """The loop of the reference's train(args) (training.py:47-258), one process per GPU: shuffled global batches of
    `args.batch_size` leaves per rank, a dead-code reset every DEAD_CODE_RESET_INTERVAL epochs from the first batch's encoder
    outputs (:120,165-166,180-181), a validation pass (:183-199), the best-validation checkpoint (:216-233), a final save (:252).

    build(local_rank, device, world) -> (codec, trainer, leaves, train ids, validation ids); leaves is a numpy array, one row
    per leaf, and this rank keeps all of it resident on `device` (default: this rank's GPU).
    export(trainer, path) writes the final weight pack on rank 0 and may return a line to log.
    after_validation(codec, validation batches, val) -> (extra record entries, lines logged before the epoch line, lines after).
    """
    distributed = "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if distributed and not dist.is_initialized():
        dist.init_process_group(args.backend, **({"device_id": torch.device("cuda", local)} if args.backend == "nccl" else {}))
    if args.single_gpu_rehearsal:
        local = 0
    if device is None:
        device = torch.device("cuda", local)
        torch.cuda.set_device(device)
    device = torch.device(device)
    log = (lambda *a: print(*a, flush=True)) if rank == 0 else (lambda *a: None)

    codec, trainer, leaves, tr_ids, va_ids = build(local, device, world)
    log(f"Dataset: {len(leaves)} leaves, train {len(tr_ids)}, val {len(va_ids)}; {world} rank(s) x batch {args.batch_size}")
    gb = args.batch_size * world
    steps_per_epoch = len(tr_ids) // gb
    # every rank sees the same sizes, so every rank raises here together (a rank with an empty shard would otherwise fail alone
    # inside a step while its peers block in all_reduce)
    if steps_per_epoch < 1:
        raise SystemExit(f"training set of {len(tr_ids)} leaves is smaller than one global batch ({world} x {args.batch_size}); lower --batch_size")
    if len(va_ids) < world:
        raise SystemExit(f"validation set of {len(va_ids)} leaves cannot give each of the {world} ranks a leaf")

    d_all = torch.from_numpy(np.ascontiguousarray(leaves)).to(device)

    def batch(ids, step):   # this rank's shard of a global batch
        lo, hi = shard_range(gb, rank, world)
        return d_all[torch.from_numpy(ids[step * gb + lo: step * gb + hi]).to(device)]

    best_val, history, start_epoch = float("inf"), [], 0
    if args.resume:   # continue from a best-validation checkpoint written below
        ck = dict(np.load(args.resume))
        start_epoch = int(ck.pop("epoch", 0))
        best_val = float(ck.pop("best_val_loss", best_val))
        trainer.load_checkpoint(ck)
        log(f"Resumed from {args.resume} at epoch {start_epoch}")
    os.makedirs(os.path.dirname(os.path.abspath(args.model_path)) or ".", exist_ok=True)
    every_step = spec.train_loss == "mean"
    step_args = {"n_global": gb} if spec.pass_n_global else {}
    for epoch in range(start_epoch, args.epochs):
        order = np.random.default_rng(args.seed + 1 + epoch).permutation(tr_ids)        # shuffle=True (training.py:87-94)
        t0 = time.perf_counter()
        total, last = 0.0, None
        for step in range(steps_per_epoch):
            want = (step % args.log_every == 0) or step == steps_per_epoch - 1
            m = trainer.step(batch(order, step), keep_latent=(step == 0), want_metrics=want or every_step, **step_args)
            if every_step:
                total += m["loss"]
            if want:
                last = m
        trainer.sync()
        dt = time.perf_counter() - t0
        if (epoch + 1) % DEAD_CODE_RESET_INTERVAL == 0:
            n_dead = trainer.reset_dead_codes()
            if n_dead:
                log(f"INFO: Resetting {n_dead} dead codes.")
        # validation (training.py:183-199): whole validation set in global batches, metrics averaged over batches
        val = {"recon_error": 0.0, "vq_loss": 0.0, "recon_mse": 0.0, "recon_l1": 0.0}
        n_val = max(len(va_ids) // gb, 1)
        vbatches = []
        for step in range(n_val):
            vbatch = batch(va_ids, step) if len(va_ids) >= gb else d_all[torch.from_numpy(va_ids[rank::world]).to(device)]
            mv = trainer.evaluate(vbatch)
            for k in val:
                val[k] += mv[k] / n_val
            if after_validation:
                vbatches.append(vbatch)
        val_loss = val["recon_error"] + val["vq_loss"]
        rec = {"epoch": epoch + 1}
        if spec.train_loss:
            rec["train_loss"] = total / steps_per_epoch if every_step else last.get("loss")
        rec.update({"train_vq_loss": last["vq_loss"], "perplexity": last["perplexity"], "codes_used": last["codes_used"], "val_loss": val_loss,
                    **{f"val_{k}": v for k, v in val.items()}, "leaves_per_s": steps_per_epoch * gb / dt, "epoch_s": dt})
        if spec.record_lr:
            rec["lr"] = last["lr"]
        extra, before, after = after_validation(codec, vbatches, val) if after_validation else ({}, [], [])
        rec.update(extra)
        history.append(rec)
        shown = f"Train Loss: {rec['train_loss']:.6f}" if every_step else f"Train VQ: {last['vq_loss']:.6f}"
        rate = f"{rec['leaves_per_s'] / 1e6:.3f} M" if spec.rate_unit == "M" else f"{rec['leaves_per_s'] / 1e3:.1f} k"
        for line in (*before, f"Epoch {epoch + 1:02d}/{args.epochs} | {shown} | Val Loss: {val_loss:.6f} | Perplexity: {last['perplexity']:.2f} | "
                              f"{rate} leaves/s ({dt:.2f} s/epoch)", *after):
            log(line)
        if val_loss < best_val and rank == 0:
            best_val = val_loss
            np.savez(args.model_path, epoch=epoch + 1, best_val_loss=best_val, **trainer.checkpoint())
            log(f"New best validation loss: {val_loss:.6f} - model saved.")
    trainer.finish()
    if rank == 0:
        root, ext = os.path.splitext(args.model_path)
        np.savez(root + "_final" + (ext or ".npz"), epoch=args.epochs, **(trainer.checkpoint() if spec.final_checkpoint else trainer.state_dict()))
        line = export(trainer, root + "_final.vqw") if export else None
        if line:
            log(line)
    log("Training completed!")
    codec.close()
    return {"history": history, "best_val_loss": best_val, "steps_per_epoch": steps_per_epoch, "world": world}
