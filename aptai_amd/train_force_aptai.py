"""The Force_APTAI training loop of the reference (train/train_force_aptai.py) on the MI355X build: same function surface
(`load_model_optimizer`, `train`, `validate`, `test`), per-batch protocol (`model(epoch, **batch_x)` -> `loss.backward()` ->
`optimizer.step()`; only the heads train, the `Wav2Vec2_PR` encoder is frozen and runs in inference mode), schedule, validation /
test keys and best-checkpoint files.  Differences from train_aptai.py follow the reference's own diff: `--pr_model_path`,
`phoneme_labels` in the batch (:271-275), tv/align losses in the log, CTC-based PER (:578-586), `pred_frame_phns` as the
frame prediction.  The corpus reader, LOSO bookkeeping and wandb are out of scope: `SyntheticHPRC` items
carry a `phoneme_label` sequence as well.

    python -m aptai_amd.train_force_aptai --pr_model_path <dir with best-model-ckpt/> --num_epochs 2
"""
from __future__ import annotations

import argparse
from typing import Dict

import numpy as np
import torch

from . import hostlogic, loops, metrics
from .force_aptai import Force_APTAI
from .train_aptai import SyntheticHPRC, _score_file, _scores, _stack_gt, _to_device


class SyntheticHPRCWithLabels(SyntheticHPRC):
    """SyntheticHPRC items + the `phoneme_label` id sequence of data/dataset_hprc.py (20..55 ids)."""

    def __init__(self, *a, vocab_size: int = 40, **kw):
        super().__init__(*a, **kw)
        self.vocab_size = vocab_size

    def __getitem__(self, i):
        item = super().__getitem__(i)
        g = np.random.RandomState(self.seed * 7919 + i + 17)
        item["phn_frames_49hz"] = (item["phn_frames_49hz"] % (self.vocab_size - 1) + 1).astype(np.int64)
        item["phoneme_label"] = g.randint(1, self.vocab_size, size=int(g.randint(20, 56))).astype(np.int32)
        return item


def collate(batch):
    return hostlogic.collate_aptai(batch, with_phoneme_labels=True)


def collate_raw(batch):
    """`collate` for a corpus at its native rate (cfg.source_rate / cfg.normalize_audio): packed audio + offsets."""
    return hostlogic.collate_aptai_raw(batch, with_phoneme_labels=True)


def load_model_optimizer(args_cfg):
    """train/train_force_aptai.py:328-368: Force_APTAI over a trained recogniser checkpoint, Adam over the parameters that
    require gradients (the heads), LambdaLR with the 10x warm-up schedule."""
    model = Force_APTAI(args_cfg.pr_model_path, args_cfg.device, args_cfg.vocab,
                        max_phn_seq_len=getattr(args_cfg, "max_phn_seq_len", 60)).to(args_cfg.device)
    model.transcript = getattr(args_cfg, "transcript", "decoded")
    # --mask_feature_prob / --mask_feature_length land on the recogniser's config once its checkpoint is loaded (its parameter set
    # follows the pickled config).  They are recorded, not used: the frozen recogniser runs in eval mode, so it is never masked.
    loops.apply_mask_feature_arguments(model.w2v2_pr.wav2vec2.config, args_cfg)
    optimizer, lr_scheduler = loops.adam_and_schedule([p for p in model.parameters() if p.requires_grad], args_cfg)
    return model, optimizer, lr_scheduler


def train(cfg, model, optimizer, lr_scheduler, train_dataloader, valid_dataloader, test_spk, best_ckpt_path, log=print):
    """train/train_force_aptai.py:392-531.  Returns the per-epoch log dicts."""
    run = loops.EpochDriver(cfg, model, optimizer, lr_scheduler, best_ckpt_path)
    frontend = run.frontend                  # not None: the loaders use collate_raw
    for epoch in range(cfg.num_epochs):
        model.train()
        # one batch of lookahead: the frozen recogniser's pass for batch i+1 is started on a side stream before the heads of
        # batch i are launched (Force_APTAI.prefetch; results do not depend on it).  cfg.pipeline_encoder = False turns it off.
        pipelined = bool(getattr(cfg, "pipeline_encoder", True)) and str(cfg.device).startswith("cuda")
        it = iter(train_dataloader)
        nxt = next(it, None)
        if nxt is not None:
            nxt = _to_device(nxt, cfg.device, frontend, augment=True)          # cfg.speed_perturb: the train batches only
        while nxt is not None:
            batch_x, nxt = nxt, next(it, None)
            if nxt is not None:
                nxt = _to_device(nxt, cfg.device, frontend, augment=True)
            ahead = (nxt["audio_inputs"], nxt["audio_lengths"]) if (pipelined and nxt is not None) else None
            outputs = run.eager_step(lambda: model(epoch, **batch_x, _prefetch_next=ahead))
            log(f"\tepoch {epoch + 1} ~ batch {run.steps}/{len(train_dataloader)}, train_loss: {float(outputs['loss'].detach()):.4f}, "
                f"train_tv_loss: {float(outputs['tv_loss'].detach()):.4f}, train_align_loss: {float(outputs['align_loss'].detach()):.4f}, "
                f"lr: {optimizer.param_groups[0]['lr']:.6f}")
        epoch_log = run.end_epoch(epoch, lambda: validate(model, cfg.device, cfg.vocab, epoch, getattr(cfg, "exp_dir", None), test_spk,
                                                          valid_dataloader, device_metrics=getattr(cfg, "device_metrics", False),
                                                          batch_invariant=getattr(cfg, "batch_invariant_eval", False),
                                                          frontend=frontend))
        log(loops.epoch_line(cfg, epoch_log))
    return run.close()


def _one_file(s, model, device, epoch, batch_x, frontend=None):
    """One batch-1 evaluation pass shared by validate() and test(): TV and frame scores with `pred_frame_phns` as the prediction
    (:588-600), CTC-based edit distance (:578-586), all appended to `s`."""
    outputs, batch_x, _, _ = _score_file(s, model, device, epoch, batch_x, frontend,
                                         pred_frames=lambda outputs: torch.tensor(outputs["pred_frame_phns"], device=device))
    gt_phn = batch_x["phoneme_labels"].cpu().numpy()[0]
    pred_phn = np.asarray(outputs["pred_ctc_phn_seq"][0]).tolist()
    s["edit_d"].append(metrics.edit_distance(gt_phn, pred_phn))
    s["n_phn"].append(len(gt_phn))
    return outputs


def _device_eval(model, device, epoch, dl, acc, frontend=None):
    """validate()/test() with `device_metrics=True`: Force_APTAI's device-output route (no Python lists), every metric through
    aptai_amd.device_metrics.  The decoded-length check and the BiLSTM status words `_lists` reads per step are accumulated on
    the device and checked once in `acc.result()`."""
    from . import device_metrics as dm
    acc.max_phonemes = model.max_phn_seq_len
    for batch_x in dl:
        with torch.no_grad():
            batch_x = _to_device(batch_x, device, frontend)
            tvs_gt = _stack_gt(batch_x)
            outputs = model(epoch, **batch_x, _device_outputs=True)
        lens = outputs["frame_lens"]
        acc.add_loss(outputs["loss"])
        acc.add_tv(tvs_gt, outputs["tvs_pred"], lens)
        labels = batch_x["phoneme_labels"]
        acc.add_edit(labels, dm.label_lengths(labels), outputs["ctc_ids"], outputs["ctc_lens"])
        acc.add_frames(batch_x["phn_frames_49hz"], outputs["frame_phns"], lens)
        acc.add_decoded_lengths(outputs["ctc_lens"])
        acc.add_lstm_status(outputs["frame_phns"].device)
    return acc.result()


@loops.batch_invariant_eval
def validate(model, device, vocab, epoch, exp_dir, test_spk, val_dl, log_step=100, device_metrics=False, frontend=None) -> Dict[str, float]:
    """train/train_force_aptai.py:533-652, batch size 1 (incl. the TTCD-twice ground-truth stack).  `device_metrics=True`
    (opt-in): the same entries from aptai_amd.device_metrics, one device->host transfer per call."""
    if device_metrics:
        from .device_metrics import EvalAccumulator
        return _device_eval(model, device, epoch, val_dl, EvalAccumulator("val", per="edit"), frontend=frontend)
    s = _scores()
    for batch_x in val_dl:
        s["losses"].append(_one_file(s, model, device, epoch, batch_x, frontend)["loss"].item())
    return metrics.eval_summary("val", **s)


@loops.batch_invariant_eval
def test(model, device, vocab, exp_dir, test_spk, test_dl, rate, log_step=100, num_epochs=0, device_metrics=False,
         frontend=None) -> Dict[str, float]:
    """train/train_force_aptai.py:655-838: as train_aptai.test plus the std entries and the CTC-based PER."""
    assert rate in ["F", "N"]
    model.eval()
    if device_metrics:
        from .device_metrics import EvalAccumulator
        return _device_eval(model, device, num_epochs, test_dl, EvalAccumulator("test", rate=rate, per="edit", with_std=True),
                            frontend=frontend)
    s = _scores()
    for batch_x in test_dl:
        _one_file(s, model, device, num_epochs, batch_x, frontend)
    return metrics.eval_summary("test", rate=rate, with_std=True, **s)


def default_cfg(**kw):
    """Hyper-parameters at the reference's argparse defaults (train/train_force_aptai.py:45-140; start_train_force_aptai.sh)."""
    vocab = {"(blank)": 0, "(...)": 1}
    vocab.update({f"p{i}": i for i in range(2, 40)})
    return loops.default_cfg(kw, batch_size=5, learning_rate=1e-5, target_metric="val_mean_rmse", exp_dir=None, vocab=vocab,
                             pr_model_path=None, max_phn_seq_len=60, transcript="decoded")


def parse_args(argv=None):
    """The command line of main()."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pr_model_path", required=True, help="directory holding best-model-ckpt/{pytorch_model.bin, model_cfg.pkl}")
    ap.add_argument("--num_epochs", type=int, default=2)
    ap.add_argument("--steps_per_epoch", type=int, default=8)
    ap.add_argument("--val_items", type=int, default=4)
    ap.add_argument("--batch_size", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--learning_rate", type=float, default=1e-5)
    loops.add_shared_arguments(ap)
    ap.add_argument("--max_phn_seq_len", type=int, default=60,
                    help="phoneme slots per utterance, 2..255: a transcript must be shorter than this (the reference's constant: 60)")
    ap.add_argument("--transcript", choices=("decoded", "labels"), default="decoded",
                    help="what the aligner aligns to: the frozen recogniser's decode, or the batch's phoneme_labels")
    ap.add_argument("--out", default="force_aptai_ckpt")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    cfg = default_cfg(num_epochs=a.num_epochs, batch_size=a.batch_size, learning_rate=a.learning_rate, pr_model_path=a.pr_model_path,
                      max_phn_seq_len=a.max_phn_seq_len, transcript=a.transcript, **loops.shared_arguments(a))
    model, optimizer, lr_scheduler = load_model_optimizer(cfg)
    w2v = model.w2v2_pr.wav2vec2.config
    train_ds = SyntheticHPRCWithLabels(a.steps_per_epoch * a.batch_size, a.seconds, seed=1, cfg=w2v, vocab_size=len(cfg.vocab),
                                       source_rate=a.source_rate)
    val_ds = SyntheticHPRCWithLabels(a.val_items, a.seconds, seed=2, cfg=w2v, vocab_size=len(cfg.vocab), source_rate=a.source_rate)
    coll = collate_raw if loops.uses_frontend(a) else collate
    train_dl = torch.utils.data.DataLoader(train_ds, batch_size=a.batch_size, shuffle=True, drop_last=True, collate_fn=coll)
    val_dl = torch.utils.data.DataLoader(val_ds, batch_size=1, shuffle=False, collate_fn=coll)
    return train(cfg, model, optimizer, lr_scheduler, train_dl, val_dl, "synthetic", a.out)


if __name__ == "__main__":
    main()
