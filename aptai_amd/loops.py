"""What the three training loops (train_aptai, train_force_aptai, train_phoneme_recognizer) share, once: the batch upload
through the optional device front end, Adam + LambdaLR, the common hyper-parameters and command-line flags, and `EpochDriver`,
the epoch skeleton of the reference's train() functions (train/train_aptai.py:392-531 and its two siblings): train step, clip
monitor, graphed runner, schedule step, validation, best checkpoint, epoch log.  Which batches an epoch trains on, how the model
is called and what gets printed stay in each loop's own module.
"""
from __future__ import annotations

import contextlib
import functools
import pickle
from pathlib import Path
from types import SimpleNamespace

import torch

from . import hostlogic
from .frontend import make_frontend, parse_speeds, raw_batch_to_device, uses_frontend


def to_device(batch, device, frontend, audio_key, length_key, host_lengths=False, augment=False):
    """The collate's batch on the device.  With a front end (cfg.source_rate / cfg.normalize_audio / cfg.speed_perturb) the batch
    is a `collate_*_raw` one: its packed audio is uploaded as it is and resampled / normalised there into `audio_key` /
    `length_key`.  `augment` (the training step only): a front end with speeds perturbs the batch, audio and frame-level targets;
    the indices it applied stay on it as `frontend.last_speed_index` and do not travel into the model's arguments."""
    if frontend is None:
        return {k: v.to(device) for k, v in batch.items()}
    out = raw_batch_to_device(batch, frontend, device, audio_key, length_key, host_lengths=host_lengths, augment=augment)
    frontend.last_speed_index = out.pop("_speed_index", None)
    return out


def _dp_rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def adam_and_schedule(params, args_cfg, publish_to=None):
    """Adam and LambdaLR with the 10x warm-up schedule, as the reference's load_model_optimizer functions build them.  The
    optimiser is torch.optim.Adam's update rule as one multi-tensor HIP kernel (aptai_amd.optim.Adam; same constructor,
    param_groups and state keys): `torch.optim.Adam(params, ...)` works unchanged on the same parameters.  `publish_to`: the model
    whose bf16 weight copies the step refreshes in the same pass."""
    from .optim import Adam
    optimizer = Adam(params, lr=args_cfg.learning_rate, betas=(args_cfg.adam_beta1, args_cfg.adam_beta2), eps=args_cfg.adam_epsilon,
                     weight_decay=args_cfg.adam_weight_decay, max_grad_norm=getattr(args_cfg, "max_grad_norm", None),
                     gradient_accumulation_steps=getattr(args_cfg, "gradient_accumulation_steps", 1),
                     ema_decay=getattr(args_cfg, "ema_decay", None), ema_warmup=getattr(args_cfg, "ema_warmup", False))
    if publish_to is not None:
        optimizer.publish_to(publish_to)
    lr_scheduler = torch.optim.lr_scheduler.LambdaLR(
        optimizer=optimizer, lr_lambda=hostlogic.get_lr_schedule(args_cfg.num_warmup_epochs, args_cfg.num_static_epochs, args_cfg.lr_decay))
    return optimizer, lr_scheduler


def default_cfg(overrides, **own):
    """The hyper-parameters all three loops take at the reference's argparse defaults, the loop's `own` ones, then `overrides`."""
    cfg = SimpleNamespace(device="cuda", num_epochs=2, adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8, adam_weight_decay=0.0,
                          num_warmup_epochs=10, num_static_epochs=30, lr_decay=0.96, target_metric_bigger_better=False,
                          device_metrics=False, batch_invariant_eval=False, source_rate=None, normalize_audio=False, ema_decay=None,
                          ema_warmup=False, mask_feature_prob=None, mask_feature_length=None, speed_perturb=None, speed_perturb_seed=0,
                          **own)
    cfg.__dict__.update(overrides)
    return cfg


def add_shared_arguments(ap):
    ap.add_argument("--max_grad_norm", type=float, default=None,
                    help="clip the gradients at this global 2-norm inside the optimiser step (off by default)")
    ap.add_argument("--gradient_accumulation_steps", type=int, default=1,
                    help="update once per this many batches, with the mean of their gradients (accumulated inside the optimiser; off by default)")
    ap.add_argument("--ema_decay", type=float, default=None,
                    help="keep an exponential moving average of the weights inside the optimiser step with this decay; validation and "
                         "the best checkpoint then use the averaged weights (off by default)")
    ap.add_argument("--ema_warmup", action="store_true",
                    help="with --ema_decay: the k-th update uses min(ema_decay, (1 + k) / (10 + k))")
    ap.add_argument("--mask_feature_prob", type=float, default=None,
                    help="SpecAugment along the hidden axis: the share of channels that starts a masked span, per utterance and "
                         "train step (default: the checkpoint's config value)")
    ap.add_argument("--mask_feature_length", type=int, default=None,
                    help="channels per span of --mask_feature_prob (default: the checkpoint's config value)")
    ap.add_argument("--source_rate", type=int, default=None,
                    help="the corpus' sampling rate: the audio is uploaded at that rate and resampled to 16 kHz on the device")
    ap.add_argument("--normalize_audio", action="store_true", help="zero-mean / unit-variance normalisation on the device")
    ap.add_argument("--speed_perturb", type=str, default=None,
                    help="speed perturbation of the training batches on the device: comma-separated factors in [0.5, 2.0], at most 8 "
                         "(e.g. 0.9,1.0,1.1), one drawn per utterance and step; frame-level targets are stretched to match (off by default)")
    ap.add_argument("--speed_perturb_seed", type=int, default=0, help="seed of the --speed_perturb draws (a data-parallel rank adds its rank)")
    ap.add_argument("--batch_invariant_eval", action="store_true",
                    help="validate() / test() with the model's batch_invariant switch on: every utterance of a batch scored as if it "
                         "ran alone, so evaluation may run at any batch size (off by default)")


def shared_arguments(a) -> dict:
    """The parsed flags of add_shared_arguments as default_cfg entries."""
    return dict(max_grad_norm=a.max_grad_norm, gradient_accumulation_steps=a.gradient_accumulation_steps, source_rate=a.source_rate,
                normalize_audio=a.normalize_audio, batch_invariant_eval=a.batch_invariant_eval, ema_decay=a.ema_decay,
                ema_warmup=a.ema_warmup, mask_feature_prob=a.mask_feature_prob, mask_feature_length=a.mask_feature_length,
                speed_perturb=parse_speeds(a.speed_perturb), speed_perturb_seed=a.speed_perturb_seed)


def apply_mask_feature_arguments(w2v_cfg, a):
    """--mask_feature_prob / --mask_feature_length onto a W2V2Config, in place: a flag that was not given (None) leaves the
    checkpoint's value alone.  `a` is the parsed command line or a loop cfg.  The result is validated, so a length the hidden
    axis cannot hold is refused before a model is built."""
    for name in ("mask_feature_prob", "mask_feature_length"):
        v = getattr(a, name, None)
        if v is not None:
            setattr(w2v_cfg, name, v)
    w2v_cfg.validate()
    return w2v_cfg


def batch_invariant_eval(fn):
    """Gives a loop's validate() / test() the keyword `batch_invariant=False` (cfg.batch_invariant_eval in train()): the model's
    `batch_invariant` attribute is set for the duration of the pass, on the host-metrics and the device-metrics path alike, and put
    back afterwards.  Every utterance of a batch then gets its batch-1 predictions, so the per-utterance metrics do not depend on
    the loader's batch size; `val_mean_loss` stays a mean over BATCHES of the model's batch loss."""
    @functools.wraps(fn)
    def run(model, *args, batch_invariant=False, **kw):
        if not batch_invariant:
            return fn(model, *args, **kw)
        prev = model.batch_invariant
        model.batch_invariant = True
        try:
            return fn(model, *args, **kw)
        finally:
            model.batch_invariant = prev
    return run


def save_checkpoint(model, path):
    """The two files a checkpoint directory holds."""
    torch.save(model.state_dict(), path / "pytorch_model.bin")
    pickle.dump(model.get_config(), open(path / "model_cfg.pkl", "wb"))


def epoch_line(cfg, epoch_log) -> str:
    """The epoch line of the two TV loops: the float-valued entries, in the log's order."""
    return (f"Epoch {epoch_log['epoch'] + 1}/{cfg.num_epochs} -> "
            + " | ".join(f"{k}: {v:.4f}" for k, v in epoch_log.items() if isinstance(v, float)))


class EpochDriver:
    """The state a train() carries from step to step and from epoch to epoch.  Per trained batch the loop calls `eager_step` or
    `graphed_step`, per epoch `end_epoch`, at the end `close`.

        frontend   None unless cfg.source_rate / cfg.normalize_audio / cfg.speed_perturb: then the loaders use the `collate_*_raw`
                   functions (its speed draws are seeded with cfg.speed_perturb_seed + the data-parallel rank)
        steps      batches trained on in this epoch so far
    """

    def __init__(self, cfg, model, optimizer, lr_scheduler, best_ckpt_path):
        self.cfg, self.model, self.optimizer, self.lr_scheduler = cfg, model, optimizer, lr_scheduler
        self.frontend = make_frontend(cfg, rank=_dp_rank())
        # cfg.max_grad_norm: the optimiser clips at this global norm inside step(); the loop only adds the device-side norm and the
        # "was clipped" flag into two device scalars per step and reads them once per epoch (optim.ClipMonitor)
        self.clip = None
        if getattr(cfg, "max_grad_norm", None) is not None:
            from . import optim
            self.clip = optim.ClipMonitor(optimizer)
        self.best_ckpt_path = Path(best_ckpt_path)
        self.best_ckpt_path.mkdir(parents=True, exist_ok=True)
        self.runner = None
        self.eval_target = None
        self.history = []
        # cfg.gradient_accumulation_steps: every optimizer.step() below is one micro-step of a window (aptai_amd.optim.Adam); the loop
        # counts the updates, keeps the clip monitor to them and closes an unfinished window at the end of the epoch
        self.accumulate = getattr(cfg, "gradient_accumulation_steps", 1) > 1
        # cfg.ema_decay: the optimiser averages the weights inside step(); validation and the best checkpoint see the averages
        self.ema = getattr(cfg, "ema_decay", None) is not None and hasattr(optimizer, "ema_weights")
        self.sum_train_loss, self.steps, self.updates = 0.0, 0, 0

    def eager_step(self, forward):
        """zero_grad -> `forward()` (the loop's model call on its uploaded batch) -> backward -> optimizer.step.  Returns the outputs.
        (Under accumulation too: the window's sum lives in the optimiser, not in `.grad`.)"""
        self.optimizer.zero_grad()
        outputs = forward()
        outputs["loss"].backward()
        self.optimizer.step()
        return self._trained(outputs)

    def graphed_step(self, batch):
        """The same step replayed as hipGraph segments.  The collates pad every batch to its own longest utterance (and label
        list), so shapes vary: BucketedGraphedStep keeps one captured runner per (batch size, bucket length, label width) and
        feeds each batch to the next larger bucket (results equal the eager step on the batch's own shape).  `batch`: the
        collate's HOST batch (pinned staging ring + asynchronous copies), or a device batch whose lengths are host tensors."""
        if self.runner is None:
            from . import graphed
            self.runner = graphed.BucketedGraphedStep(self.model, self.optimizer)
        return self._trained(self.runner.step(batch))

    def _updated(self):
        """After an optimizer.step() or flush() that moved the parameters (every one, unless accumulation is on)."""
        self.updates += 1
        if self.clip is not None:
            self.clip.update()

    def _trained(self, outputs):
        if getattr(self.optimizer, "last_step_updated", True):
            self._updated()
        self.sum_train_loss += float(outputs["loss"].detach())
        self.steps += 1
        return outputs

    def end_epoch(self, epoch, validate, planned_steps=None, extra_checkpoints=None):
        """Schedule step, validation (`validate()` -> its dictionary), best checkpoint, the epoch's log dictionary (also appended
        to `history`).  A tie on cfg.target_metric counts as better and writes the checkpoint again.  `planned_steps`: the
        recogniser's fixed number of steps per epoch; the mean train loss divides by it and the log gains `trained_batches`.
        `extra_checkpoints()`: further files, written after the best checkpoint.  With cfg.ema_decay, validation and the best
        checkpoint run on the AVERAGED weights (optimizer.ema_weights); `extra_checkpoints()` and the next epoch see the raw ones."""
        cfg, model = self.cfg, self.model
        if getattr(self.optimizer, "micro_step", 0) and self.optimizer.flush():        # a remainder of the epoch's last window
            self._updated()
        self.lr_scheduler.step()
        if self.runner is not None:
            self.runner.suspend()        # the eager validation below rebuilds its weight copies; the captured buckets stay
        model.eval()
        with self.optimizer.ema_weights(model) if self.ema else contextlib.nullcontext():
            val_logs = validate()
            better = (self.eval_target is None
                      or (cfg.target_metric_bigger_better and self.eval_target <= val_logs[cfg.target_metric])
                      or (not cfg.target_metric_bigger_better and self.eval_target >= val_logs[cfg.target_metric]))
            if better:
                self.eval_target = val_logs[cfg.target_metric]
                save_checkpoint(model, self.best_ckpt_path)
        if extra_checkpoints is not None:
            extra_checkpoints()
        divisor = self.steps if planned_steps is None else planned_steps
        epoch_log = dict(val_logs, epoch=epoch, mean_train_loss=self.sum_train_loss / max(divisor, 1),
                         lr=self.optimizer.param_groups[0]["lr"], saved=bool(better))
        if planned_steps is not None:
            epoch_log["trained_batches"] = self.steps
        if self.accumulate:
            epoch_log["optimizer_updates"] = self.updates
        if self.clip is not None:
            epoch_log.update(self.clip.epoch_log())
        if self.ema:
            epoch_log["ema_updates"] = getattr(self.optimizer, "ema_updates", 0)
        self.history.append(epoch_log)
        self.sum_train_loss, self.steps, self.updates = 0.0, 0, 0
        return epoch_log

    def close(self):
        """After the last epoch: releases the graphed runner.  Returns the per-epoch log dictionaries."""
        if self.runner is not None:
            self.runner.close()
        return self.history
