"""The APTAI training loop of the reference (train/train_aptai.py) on the MI355X build: same function surface
(`load_model_optimizer`, `train`, `validate`), same per-batch protocol (`model(epoch, **batch_x)` -> `loss.backward()` ->
`optimizer.step()`), same schedule, same validation metrics and return keys, same best-checkpoint files
(`pytorch_model.bin` + `model_cfg.pkl`).  What is NOT here: the HPRC corpus reader, leave-one-speaker-out bookkeeping, wandb
(SURVEY.md §2 rows marked out of scope) — `SyntheticHPRC` yields items with the fields `_collate_fn` consumes instead.

    python -m aptai_amd.train_aptai --model_dir <local wav2vec2 dir> --num_epochs 2 --steps_per_epoch 20 --batch_size 16
    python -m aptai_amd.train_aptai --random_init base --graphed        # hipGraph segments, one captured runner per length bucket
"""
from __future__ import annotations

import argparse
import tempfile
from typing import Dict, Optional

import numpy as np
import torch

from . import hostlogic, loops, metrics
from .aptai import APTAI
from .config import W2V2Config
from .wav2vec2 import Wav2Vec2Model

VOCAB_SIZE = 46        # models/aptai.py:54 hard-codes Linear(1024, 46)


class SyntheticHPRC(torch.utils.data.Dataset):
    """Items shaped like data/dataset_hprc.py's (audio, audio_len, phn_frames_49hz, tvs_norm_49hz[9 tracks]) with the
    synthetic content SURVEY.md §8d prescribes: N(0,1) audio, uniform frame labels, N(0,1) trajectories."""

    def __init__(self, n_items: int, seconds: float = 10.0, vary_length: bool = True, seed: int = 0, cfg: Optional[W2V2Config] = None,
                 source_rate: Optional[int] = None):
        # source_rate: the audio is emitted at that rate (`audio_len` = the raw length); frame labels and TV targets are sized
        # from the 16 kHz length ceil(16000 n / source_rate) the device front end produces
        self.rate = int(source_rate or 16000)
        self.n, self.S, self.vary, self.seed = n_items, int(self.rate * seconds), vary_length, seed
        self.cfg = cfg or W2V2Config.base()

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = np.random.RandomState(self.seed * 100003 + i)
        n = self.S if (not self.vary or i % 2 == 0) else int(g.randint(int(0.8 * self.S), self.S + 1))
        T = int(hostlogic.feat_extract_output_lengths(hostlogic.resample_out_length(n, self.rate, 16000), self.cfg.conv_kernel,
                                                      self.cfg.conv_stride))
        labels = np.repeat(g.randint(1, VOCAB_SIZE, size=T // 4 + 1), 4)[:T]        # phone-like runs of 4 frames
        return {"audio": g.randn(n).astype(np.float32), "audio_len": n, "phn_frames_49hz": labels.astype(np.int64),
                "tvs_norm_49hz": {k: g.randn(T) for k in hostlogic.TV_NAMES}}


def _to_device(batch_x, device, frontend=None, host_lengths=False, augment=False):
    return loops.to_device(batch_x, device, frontend, "audio_inputs", "audio_lengths", host_lengths, augment)


def load_model_optimizer(args_cfg):
    """train/train_aptai.py:334-372: APTAI on a LOCAL wav2vec2 directory, Adam, LambdaLR with the 10x warm-up schedule."""
    pretrain_cfg = args_cfg.pretrain_cfg
    model = APTAI(device=args_cfg.device, vocab=args_cfg.vocab, huggingface_model_id=args_cfg.huggingface_model_id,
                  pretrain_cfg=pretrain_cfg, cache_dir=getattr(args_cfg, "cache_dir", None)).to(args_cfg.device)
    optimizer, lr_scheduler = loops.adam_and_schedule(model.parameters(), args_cfg, publish_to=model)
    return model, optimizer, lr_scheduler


def train(cfg, model, optimizer, lr_scheduler, train_dataloader, valid_dataloader, test_spk, best_ckpt_path, log=print):
    """train/train_aptai.py:392-531.  Returns the per-epoch log dicts (the reference only prints them)."""
    run = loops.EpochDriver(cfg, model, optimizer, lr_scheduler, best_ckpt_path)
    frontend = run.frontend                  # not None: the loaders use collate_aptai_raw
    for epoch in range(cfg.num_epochs):
        model.train()
        for batch_idx, batch_x in enumerate(train_dataloader):
            if getattr(cfg, "graphed", False):
                # the runners take the collate_fn's HOST batch; with a front end that runs eagerly first, and its output is the
                # device batch the runners take as well
                outputs = run.graphed_step(batch_x if frontend is None else _to_device(batch_x, cfg.device, frontend, host_lengths=True,
                                                                                             augment=True))
            else:
                batch_x = _to_device(batch_x, cfg.device, frontend, augment=True)          # cfg.speed_perturb: the train step only
                outputs = run.eager_step(lambda: model(epoch, **batch_x))
            log(f"\tepoch {epoch + 1} ~ batch {batch_idx + 1}/{len(train_dataloader)}, train_loss: {float(outputs['loss'].detach()):.4f}, "
                f"train_mse_loss: {float(outputs['mse_loss'].detach()):.4f}, train_ce_loss: {float(outputs['ce_loss'].detach()):.4f}, "
                f"lr: {optimizer.param_groups[0]['lr']:.6f}")
        epoch_log = run.end_epoch(epoch, lambda: validate(model, cfg.device, cfg.vocab, epoch, getattr(cfg, "exp_dir", None), test_spk,
                                                          valid_dataloader, device_metrics=getattr(cfg, "device_metrics", False),
                                                          batch_invariant=getattr(cfg, "batch_invariant_eval", False),
                                                          frontend=frontend))
        log(loops.epoch_line(cfg, epoch_log))
    return run.close()


def _device_eval(model, device, epoch, dl, acc, frontend=None):
    """The evaluation pass of validate()/test() with `device_metrics=True`: the same forward, the metrics of every utterance of
    the batch computed by the kernels of aptai_amd.device_metrics and left on the device (no blocking call per batch).  Any batch
    size: frame counts come from `audio_lengths` through the encoder's length formula."""
    from . import device_metrics as dm
    for batch_x in dl:
        with torch.no_grad():
            batch_x = _to_device(batch_x, device, frontend)
            tvs_gt = _stack_gt(batch_x)
            outputs = model(epoch, **batch_x)
        tvs_pred = outputs["tvs_pred"]
        lens = dm.frame_lengths(model.wav2vec2, batch_x["audio_lengths"], tvs_pred.shape[1])
        acc.add_loss(outputs["loss"])
        acc.add_tv(tvs_gt, tvs_pred, lens)
        acc.add_frames(batch_x["phn_frames_49hz"], outputs["phn_fc_pred"], lens)
    return acc.result()


@loops.batch_invariant_eval
def validate(model, device, vocab, epoch, exp_dir, test_spk, val_dl, log_step=100, device_metrics=False, frontend=None) -> Dict[str, float]:
    """train/train_aptai.py:533-652, batch size 1.  Reproduces the reference as written, including its two quirks: the ground
    truth stack lists TTCD in the TMCD slot (:557-560) and `get_stats` receives frame label sequences, not boundary times.
    `device_metrics=True` (opt-in) computes the same entries with aptai_amd.device_metrics: one device->host transfer per call."""
    if device_metrics:
        from .device_metrics import EvalAccumulator
        return _device_eval(model, device, epoch, val_dl, EvalAccumulator("val", per="frames_rounded"), frontend=frontend)
    s = _scores()
    for batch_x in val_dl:
        outputs, _, y, yhat = _score_file(s, model, device, epoch, batch_x, frontend)
        s["losses"].append(outputs["loss"].item())
        y_grp, yhat_grp = metrics.phn_frame_id2phn(y.tolist()), metrics.phn_frame_id2phn(yhat.tolist())
        s["edit_d"].append(metrics.compute_PER(y_grp, yhat_grp) / 100.0 * len(y_grp))
        s["n_phn"].append(len(y_grp))
    return metrics.eval_summary("val", **s)


def _eval_frames(gt_frames, pred_frames):
    """Frame-level scores shared by validate()/test() of both TV models (train/train_aptai.py:583-607, 717-749): number of
    frames, number correct, overlap, boundary precision / recall / F1 / R-value as the reference calls `get_stats`."""
    gt_f, p_f = gt_frames.cpu().numpy(), pred_frames.cpu().numpy()
    y, yhat = gt_f.squeeze(), p_f.squeeze()
    return (gt_frames.size(1), int(torch.sum(torch.eq(gt_frames, pred_frames.to(gt_frames.device))).item()),
            metrics.evaluate_overlap(gt_f, p_f), metrics.get_stats(y, yhat, tolerance=0.02), y, yhat)


def _stack_gt(batch_x):
    """Ground-truth stack of validate()/test() AS WRITTEN in the reference: TTCD sits in the TMCD slot (:557-560, :702-705)."""
    return torch.stack([batch_x["LA"], batch_x["LP"], batch_x["JA"], batch_x["TTCL"], batch_x["TTCD"], batch_x["TMCL"],
                        batch_x["TTCD"], batch_x["TBCL"], batch_x["TBCD"]], dim=-1).float()


_tv_test_summary = metrics.tv_test_summary


def _scores():
    """Per-utterance values of a host evaluation pass, under the argument names of metrics.eval_summary."""
    return {k: [] for k in ("losses", "rmse", "pcc", "frames", "correct", "overlaps", "stats", "edit_d", "n_phn")}


def _score_file(s, model, device, epoch, batch_x, frontend, pred_frames=lambda outputs: outputs["phn_fc_pred"]):
    """One batch-1 evaluation pass of the host validate() / test() of both TV models: the forward, then the utterance's per-track
    RMSE / PCC and frame scores appended to `s`.  Returns (outputs, device batch, gt frame labels, predicted frame labels); the
    distance behind the PER differs per caller."""
    with torch.no_grad():
        tvs_gt = _stack_gt(batch_x)                     # from the host batch, before the upload
        batch_x = _to_device(batch_x, device, frontend)
        outputs = model(epoch, **batch_x)
    tvs_gt = torch.squeeze(tvs_gt, dim=0).cpu().numpy()
    tvs_pred = torch.squeeze(outputs["tvs_pred"], dim=0).float().cpu().numpy()
    s["rmse"].append(list(metrics.tvs_metric_rmse(tvs_gt, tvs_pred).values()))
    s["pcc"].append([v[0] for v in metrics.tvs_metric_ppc(tvs_gt, tvs_pred).values()])
    frames, corr, overlap, stats, y, yhat = _eval_frames(batch_x["phn_frames_49hz"], pred_frames(outputs))
    s["frames"].append(frames); s["correct"].append(corr); s["overlaps"].append(overlap); s["stats"].append(stats)
    return outputs, batch_x, y, yhat


@loops.batch_invariant_eval
def test(model, device, vocab, exp_dir, test_spk, test_dl, rate, log_step=100, num_epochs=0, device_metrics=False,
         frontend=None) -> Dict[str, float]:
    """train/train_aptai.py:655-850, batch size 1: per-track RMSE / PCC means, FER, frame-grouped PER, overlap, boundary scores,
    keyed `test_{rate}_...` with rate in {'F', 'N'} (fast / normal speaking rate splits of the corpus).  `num_epochs` stands for
    the module-global `cfg.num_epochs` the reference passes as the epoch argument (:709)."""
    assert rate in ["F", "N"]
    model.eval()
    if device_metrics:
        from .device_metrics import EvalAccumulator
        return _device_eval(model, device, num_epochs, test_dl, EvalAccumulator("test", rate=rate, per="frames"), frontend=frontend)
    s = _scores()
    for batch_x in test_dl:
        _, _, y, yhat = _score_file(s, model, device, num_epochs, batch_x, frontend)
        y_grp, yhat_grp = metrics.phn_frame_id2phn(y.tolist()), metrics.phn_frame_id2phn(yhat.tolist())
        s["edit_d"].append(metrics.edit_distance(y_grp, yhat_grp))
        s["n_phn"].append(len(y_grp))
    return metrics.eval_summary("test", rate=rate, **s)


def default_cfg(**kw):
    """Hyper-parameters at the reference's argparse defaults (train/train_aptai.py:45-140)."""
    return loops.default_cfg(kw, batch_size=16, learning_rate=1e-5, target_metric="val_mean_rmse", graphed=False, exp_dir=None,
                             vocab={f"p{i}": i for i in range(VOCAB_SIZE)}, cache_dir=None)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model_dir", default=None, help="local wav2vec2 checkpoint directory (config.json + weights)")
    ap.add_argument("--random_init", default="base", choices=["base", "large"], help="without --model_dir: random-init backbone")
    ap.add_argument("--num_epochs", type=int, default=2)
    ap.add_argument("--steps_per_epoch", type=int, default=8)
    ap.add_argument("--val_items", type=int, default=4)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--learning_rate", type=float, default=1e-5)
    loops.add_shared_arguments(ap)
    ap.add_argument("--graphed", action="store_true")
    ap.add_argument("--out", default="aptai_ckpt")
    a = ap.parse_args(argv)
    w2v = W2V2Config.base(vocab_size=VOCAB_SIZE) if a.random_init == "base" else W2V2Config.large(vocab_size=VOCAB_SIZE)
    loops.apply_mask_feature_arguments(w2v, a)
    with tempfile.TemporaryDirectory() as tmp:
        model_dir = a.model_dir
        if model_dir is None:
            torch.manual_seed(0)
            Wav2Vec2Model(w2v).save_pretrained(tmp)
            model_dir = tmp
        cfg = default_cfg(num_epochs=a.num_epochs, batch_size=a.batch_size, learning_rate=a.learning_rate, graphed=a.graphed,
                          huggingface_model_id=model_dir, pretrain_cfg=w2v, **loops.shared_arguments(a))
        model, optimizer, lr_scheduler = load_model_optimizer(cfg)
    train_ds = SyntheticHPRC(a.steps_per_epoch * a.batch_size, a.seconds, vary_length=True, seed=1, cfg=w2v, source_rate=a.source_rate)
    val_ds = SyntheticHPRC(a.val_items, a.seconds, vary_length=True, seed=2, cfg=w2v, source_rate=a.source_rate)
    collate = hostlogic.collate_aptai_raw if loops.uses_frontend(a) else hostlogic.collate_aptai
    train_dl = torch.utils.data.DataLoader(train_ds, batch_size=a.batch_size, shuffle=True, drop_last=True, collate_fn=collate)
    val_dl = torch.utils.data.DataLoader(val_ds, batch_size=1, shuffle=False, collate_fn=collate)
    return train(cfg, model, optimizer, lr_scheduler, train_dl, val_dl, "synthetic", a.out)


if __name__ == "__main__":
    main()
