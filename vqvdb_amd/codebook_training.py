"""Codebook (EMA) training on the HIP backend — host side of SURVEY.md §8 f-2, stage 1.

Mirrors what the reference's training loop does for the quantizer (python/training.py:47-258 drives
VectorQuantizerEMA.forward in training mode, python/VQVAE_v2.py:107-156, and check_and_reset_dead_codes,
:382-417), with the encoder and decoder weights frozen.  The device work is in libvqvdb_hip.so
(vqhip_train_*); this module is the data-parallel plumbing around it:

    per step and rank:  stats = encoder -> latent -> assign -> {encodings_sum, dw, |z-e|^2, rows}   (HIP kernels)
                        all_reduce(stats, SUM)          # RCCL over xGMI; the only collective on the path
                        EMA update of cluster_size / embed_avg / embedding from the global stats    (HIP kernel)

Every rank applies the identical update, so codebooks stay replicated without a broadcast.  torch is used for device
memory, streams and torch.distributed only.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from vqvdb_amd.training_common import TrainerBase, allreduce_stats, dead_code_reset, vq_metrics  # noqa: F401  (re-exported)

K, D = 256, 128
STATS_FLOATS = K + K * D + K + 1


def metrics_from_stats(stats: np.ndarray, commitment_cost: float = 0.25) -> dict:
    """vq_loss, perplexity and codes used from the (all-reduced) statistics buffer [STATS_FLOATS]."""
    return vq_metrics(stats, K, D, commitment_cost)


class CodebookTrainer(TrainerBase):
    """Drives vqhip_train_* for one rank.  `codec` is a vqvdb_amd.codec.HipCodec on this rank's device."""
    leaf_values, k, d = 512, K, D

    def __init__(self, codec, commitment_cost: float = 0.25, decay: float = 0.95, eps: float = 1e-4, group=None,
                 cluster_size: Optional[np.ndarray] = None, embed_avg: Optional[np.ndarray] = None, device: str = "cuda"):
        super().__init__(codec, commitment_cost, decay, eps, group, device)
        codec.train_begin(cluster_size, embed_avg)
        self.stats = torch.zeros(STATS_FLOATS, dtype=torch.float32, device=self.device)

    def step(self, leaves: torch.Tensor, keep_latent: bool = False, want_metrics: bool = True) -> Optional[dict]:
        """One EMA step on this rank's batch (float32 [n,512] or [n,1,8,8,8], resident on the device)."""
        leaves, n = self._leaves_arg(leaves)
        out = None
        with self._side_stream(leaves) as h:
            zptr = self._latent_ptr(n, keep_latent)
            self.codec.train_vq_stats_device(leaves.data_ptr(), n, self.stats.data_ptr(), latent_ptr=zptr, stream=h)
            allreduce_stats(self.stats, self.group)
            self.codec.train_vq_update_device(self.stats.data_ptr(), self.decay, self.eps, stream=h)
            if want_metrics:
                out = metrics_from_stats(self.stats.cpu().numpy(), self.commitment_cost)
        return out

    def finish(self):
        """Refresh the inference tables (folded search, decoder stem table) from the trained codebook."""
        self.codec.train_commit()
