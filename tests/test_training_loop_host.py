"""The one epoch loop of the four training drivers (vqvdb_amd/training_common.py::run_training) on device="cpu" with a stub
trainer that records its calls: batches and shards, keep_latent, the dead-code reset schedule, best / final checkpoints,
resume, the size checks, and the key sets of the history records and the written .npz files.  Runs without a GPU."""
import argparse
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from vqvdb_amd import train_codebook, vec3_full_training, vec3_training
from vqvdb_amd.sharding import shard_range
from vqvdb_amd.training_common import TrainerBase, run_training

N_TRAIN, N_VAL, BATCH = 40, 10, 4
QUANTIZER = ["quantizer.embedding", "quantizer.cluster_size", "quantizer.embed_avg"]
OPTIMIZER = ["optimizer.exp_avg", "optimizer.exp_avg_sq", "optimizer.steps_done"]      # FullTrainer.checkpoint adds these to its state_dict
VEC3_CHECKPOINT = ["params", "exp_avg", "exp_avg_sq", "step", "sched_t", "t_max"] + QUANTIZER   # Vec3FullTrainer.checkpoint
RECORD = ["epoch", "train_vq_loss", "perplexity", "codes_used", "val_loss", "val_recon_error", "val_vq_loss", "val_recon_mse", "val_recon_l1",
          "leaves_per_s", "epoch_s"]


class StubCodec:
    closed = False

    def close(self):
        self.closed = True


class StubTrainer(TrainerBase):
    """Records every call; leaf i holds the value i, so a batch tells which leaves it is.  The validation loss of epoch e
    (counted from the start of this run) is val_losses[e]."""

    def __init__(self, val_losses):
        self.val_losses, self.calls, self.epochs_done, self.loaded = list(val_losses), [], 0, None

    @staticmethod
    def ids(leaves):
        return leaves[:, 0].long().tolist()

    def step(self, leaves, keep_latent=False, want_metrics=True, **kw):
        self.calls.append(("step", self.ids(leaves), keep_latent, want_metrics, kw))
        return {"loss": 1.0, "vq_loss": 0.5, "perplexity": 2.0, "codes_used": 3, "lr": 1e-4} if want_metrics else None

    def evaluate(self, leaves):
        self.calls.append(("evaluate", self.ids(leaves)))
        return {"recon_error": self.val_losses[self.epochs_done - 1], "vq_loss": 0.0, "recon_mse": 0.0, "recon_l1": 0.0}

    def reset_dead_codes(self):
        self.calls.append(("reset", self.epochs_done))
        return 0

    def sync(self):
        self.epochs_done += 1

    def state_dict(self):
        return {k: np.zeros(2, np.float32) for k in QUANTIZER}

    def load_state_dict(self, sd):
        self.loaded = dict(sd)


class StubFullTrainer(StubTrainer):
    """A trainer with weights and optimizer state: checkpoint() holds more than state_dict()."""

    def state_dict(self):
        return {"encoder.pre.0.weight": np.zeros(2, np.float32), **super().state_dict()}

    def checkpoint(self):
        return {**self.state_dict(), **{k: np.zeros(2, np.float32) for k in OPTIMIZER}}


class StubVec3FullTrainer(StubFullTrainer):
    """Vec3FullTrainer's checkpoint: the flat parameter vector and optimizer state under their own names."""

    def checkpoint(self):
        return {k: np.zeros(2, np.float32) for k in VEC3_CHECKPOINT}


def run(tmp_path, monkeypatch, trainer, spec=vec3_training.SPEC, rank=0, world=1, n_train=N_TRAIN, n_val=N_VAL, epochs=11, resume=None, seed=3):
    monkeypatch.setenv("RANK", str(rank))
    monkeypatch.setenv("WORLD_SIZE", str(world))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)   # the ranks of this test never talk to each other
    args = argparse.Namespace(batch_size=BATCH, seed=seed, epochs=epochs, log_every=2, model_path=str(tmp_path / "ck" / "m.npz"), resume=resume,
                              backend="gloo", single_gpu_rehearsal=False)
    ids = np.random.default_rng(seed).permutation(n_train + n_val)
    tr_ids, va_ids = ids[:n_train], ids[n_train:]
    leaves = np.arange(n_train + n_val, dtype=np.float32).reshape(-1, 1)
    codec = StubCodec()
    saved = []
    savez = np.savez
    monkeypatch.setattr(np, "savez", lambda path, **kw: (saved.append((os.path.basename(path), int(kw["epoch"]))), savez(path, **kw)))

    def build(local, device, w):
        assert (local, device, w) == (0, torch.device("cpu"), world)
        return codec, trainer, leaves, tr_ids, va_ids

    out = run_training(args, spec, build, device="cpu")
    assert codec.closed
    return out, tr_ids, va_ids, saved


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_batches_shards_resets_and_best_checkpoint(tmp_path, monkeypatch, rank, world):
    val_losses = [5.0, 4.0, 4.5, 3.0, 3.0, 3.5, 2.0, 9.0, 9.0, 1.0, 1.5]
    t = StubTrainer(val_losses)
    out, tr_ids, va_ids, saved = run(tmp_path, monkeypatch, t, rank=rank, world=world)
    gb = BATCH * world
    steps = N_TRAIN // gb
    lo, hi = shard_range(gb, rank, world)
    assert out["steps_per_epoch"] == steps and out["world"] == world and len(out["history"]) == 11
    step_calls = [c for c in t.calls if c[0] == "step"]
    assert len(step_calls) == 11 * steps
    for epoch in range(11):
        order = np.random.default_rng(3 + 1 + epoch).permutation(tr_ids)
        mine = step_calls[epoch * steps:(epoch + 1) * steps]
        for s, (_, ids, keep_latent, want, kw) in enumerate(mine):
            assert ids == order[s * gb + lo: s * gb + hi].tolist()          # this rank's shard_range slice of the epoch's permutation
            assert keep_latent == (s == 0)
            assert want == (s % 2 == 0 or s == steps - 1) and kw == {}
        seen = [i for c in mine for i in c[1]]
        assert len(set(seen)) == len(seen) == steps * (hi - lo)              # disjoint batches
    assert [c[1] for c in t.calls if c[0] == "reset"] == [5, 10]
    n_val = N_VAL // gb
    assert [c[1] for c in t.calls if c[0] == "evaluate"] == [va_ids[s * gb + lo: s * gb + hi].tolist() for s in range(n_val)] * 11
    # reset comes after the epoch's steps and before its validation
    kinds = [c[0] for c in t.calls]
    assert kinds[4 * (steps + n_val) + steps:][:2] == ["reset", "evaluate"]
    improved = [e + 1 for e, v in enumerate(val_losses) if v < min([float("inf")] + val_losses[:e])]
    assert improved == [1, 2, 4, 7, 10]
    if rank == 0:
        assert saved == [("m.npz", e) for e in improved] + [("m_final.npz", 11)]
        assert out["best_val_loss"] == 1.0
    else:
        assert saved == [] and not (tmp_path / "ck" / "m.npz").exists() and not (tmp_path / "ck" / "m_final.npz").exists()


def test_validation_set_smaller_than_a_global_batch_is_strided(tmp_path, monkeypatch):
    t = StubTrainer([1.0])
    _, _, va_ids, _ = run(tmp_path, monkeypatch, t, rank=1, world=2, n_val=5, epochs=1)
    assert [c[1] for c in t.calls if c[0] == "evaluate"] == [va_ids[1::2].tolist()]


def test_resume_starts_at_the_stored_epoch_with_the_stored_best(tmp_path, monkeypatch):
    first = StubFullTrainer([5.0, 2.0, 3.0])
    out, tr_ids, _, _ = run(tmp_path, monkeypatch, first, epochs=3)
    assert out["best_val_loss"] == 2.0
    t = StubFullTrainer([4.0, 3.0, 2.0])   # never better than the stored best
    out, _, _, saved = run(tmp_path, monkeypatch, t, epochs=5, resume=str(tmp_path / "ck" / "m.npz"))
    assert sorted(t.loaded) == sorted(first.checkpoint())          # epoch and best_val_loss are the loop's, the rest the trainer's
    assert [r["epoch"] for r in out["history"]] == [3, 4, 5]         # the best checkpoint was written after epoch 2
    assert out["best_val_loss"] == 2.0 and saved == [("m_final.npz", 5)]
    first_step = next(c for c in t.calls if c[0] == "step")
    assert first_step[1] == np.random.default_rng(3 + 1 + 2).permutation(tr_ids)[:BATCH].tolist()


def test_too_small_sets_exit_on_every_rank(tmp_path, monkeypatch):
    with pytest.raises(SystemExit, match="smaller than one global batch.*--batch_size"):
        run(tmp_path, monkeypatch, StubTrainer([1.0]), world=2, n_train=2 * BATCH - 1)
    with pytest.raises(SystemExit, match="cannot give each of the 2 ranks a leaf"):
        run(tmp_path, monkeypatch, StubTrainer([1.0]), rank=1, world=2, n_val=1)


@pytest.mark.parametrize("module,trainer,record,best,final", [
    (train_codebook, StubTrainer, ["train_loss"] + RECORD, QUANTIZER, QUANTIZER),                                       # --mode codebook
    (train_codebook, StubFullTrainer, ["train_loss"] + RECORD, ["encoder.pre.0.weight"] + QUANTIZER + OPTIMIZER,
     ["encoder.pre.0.weight"] + QUANTIZER),                                                                               # --mode full
    (vec3_training, StubTrainer, RECORD, QUANTIZER, QUANTIZER),
    (vec3_full_training, StubVec3FullTrainer, ["train_loss", "lr"] + RECORD, VEC3_CHECKPOINT, VEC3_CHECKPOINT),
])
def test_record_and_file_key_sets_of_each_driver(tmp_path, monkeypatch, module, trainer, record, best, final):
    t = trainer([1.0, 2.0])
    out, _, _, _ = run(tmp_path, monkeypatch, t, spec=module.SPEC, epochs=2)
    for rec in out["history"]:
        assert sorted(rec) == sorted(record)
    assert sorted(np.load(tmp_path / "ck" / "m.npz").files) == sorted(["epoch", "best_val_loss"] + best)
    assert sorted(np.load(tmp_path / "ck" / "m_final.npz").files) == sorted(["epoch"] + final)
    steps = [c for c in t.calls if c[0] == "step"]
    if module is vec3_full_training:   # metrics every step (the record's train_loss is their mean), the global batch passed along
        assert all(c[3] and c[4] == {"n_global": BATCH} for c in steps) and out["history"][0]["train_loss"] == 1.0
    else:
        assert not all(c[3] for c in steps) and all(c[4] == {} for c in steps)
