"""The CTC phoneme-recogniser fine-tuning loop of the reference (train/train_phoneme_recognizer.py) on the MI355X build: same
function surface (`load_model_optimizer`, `train`, `validate`, `test`), per-batch protocol (`model(**batch_x)` ->
`loss.backward()` -> `optimizer.step()`, everything trainable unless `freeze_feature_extractor`), the reference's RANDOM SUBSET of
batches per epoch (:406,413), LambdaLR schedule, PER metric, and the three checkpoint families it writes (:472-486):
`best-model-ckpt/`, `model-ckpts/e%04d.bin` (with `save_all_epochs`) and `last-model-ckpt/` incl. optimizer / scheduler state.
Decoding for the PER is the best path by default.  The torchaudio package behind the beam decoder of utility.py:448-471 is absent,
so parity with torchaudio itself stays unpinned; `--decoder beam` (cfg.decoder, with cfg.beam_size / cfg.beam_log_add) runs that
decoder's published algorithm on the device instead (aptai_ctc_beam_search, pinned against hostlogic.ctc_beam_search), and
`--decoder flashlight` its closed form for the reference's settings.  With `--decoder beam`, `--lm_arpa PATH` or `--lm_order N`
(a phoneme n-gram estimated from the training set's labels before the first epoch) and `--lm_weight W` fuse a token language
model into that search (ngram.NGramLM, aptai_ctc_beam_search_lm): what the reference's decoder call leaves at lm=None.
The CommonPhone reader, wandb and resume-from-hub are out of scope; `SyntheticCommonPhone` yields items
with the fields `_collator` consumes.  The shipped script's stale imports / constructor arity are not
reproduced: the model is `aptai_amd.w2v2_pr.Wav2Vec2_PR(pretrain_cfg, cache_dir, huggingface_model_id, vocab)`.

    python -m aptai_amd.train_phoneme_recognizer --random_init base --num_epochs 2 --samples_per_epoch 64 --batch_size 16
"""
from __future__ import annotations

import argparse
import pickle
import random
import tempfile
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch

from . import hostlogic, loops, metrics
from .config import W2V2Config
from .w2v2_pr import Wav2Vec2_PR
from .wav2vec2 import Wav2Vec2Model


def default_vocab(n: int = 40) -> dict:
    vocab = {"(blank)": 0, "(...)": 1}
    vocab.update({f"p{i}": i for i in range(2, n)})
    return vocab


class SyntheticCommonPhone(torch.utils.data.Dataset):
    """Items shaped like data/dataset_commonphone.py's (audio, audio_len, phoneme_label): N(0,1) 16 kHz audio (optionally the
    reference's 1-second crop), 20..55 label ids in [1, V-1] (scaled down for clips that hold fewer frames)."""

    def __init__(self, n_items: int, seconds: float = 10.0, vocab_size: int = 40, vary_length: bool = True, seed: int = 0,
                 source_rate: Optional[int] = None):
        # source_rate: the audio is emitted at that rate (`audio_len` = the raw length) and the label count is sized from the
        # 16 kHz length ceil(16000 n / source_rate) the device front end produces
        self.rate = int(source_rate or 16000)
        self.n, self.S, self.V, self.vary, self.seed = n_items, int(self.rate * seconds), vocab_size, vary_length, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = np.random.RandomState(self.seed * 100003 + i)
        n = self.S if (not self.vary or i % 2 == 0) else int(g.randint(int(0.8 * self.S), self.S + 1))
        frames = max(hostlogic.resample_out_length(n, self.rate, 16000) // 320 - 1, 2)
        hi = max(2, min(55, frames // 3))
        lo = max(1, min(20, hi - 1))
        return {"audio": g.randn(n).astype(np.float32), "audio_len": n,
                "phoneme_label": g.randint(1, self.V, size=int(g.randint(lo, hi + 1))).astype(np.int32)}


def _to_device(batch_x, device, frontend=None, host_lengths=False, augment=False):
    return loops.to_device(batch_x, device, frontend, "input_values", "input_lengths", host_lengths, augment)


def load_model_optimizer(args_cfg, vocab):
    """train/train_phoneme_recognizer.py:322-379: config edits (:339-342), model on a LOCAL wav2vec2 directory, Adam over ALL
    parameters, LambdaLR."""
    pretrain_cfg = W2V2Config.from_any(args_cfg.pretrain_cfg)
    pretrain_cfg.vocab_size = len(vocab)
    pretrain_cfg.final_dropout = args_cfg.final_dropout
    if getattr(args_cfg, "num_hidden_layers", None):
        pretrain_cfg.num_hidden_layers = args_cfg.num_hidden_layers
    pretrain_cfg.ctc_loss_reduction = "mean"
    pretrain_cfg.ctc_zero_infinity = True
    pretrain_cfg.blank = 0
    model = Wav2Vec2_PR(pretrain_cfg, getattr(args_cfg, "cache_dir", None), args_cfg.huggingface_model_id, vocab).to(args_cfg.device)
    if getattr(args_cfg, "freeze_feature_extractor", False):
        model.freeze_feature_encoder()
    # opt-in decoder for the PER of validate() / test(); the class defaults (best path; the reference's beam settings) otherwise
    model.decoder = getattr(args_cfg, "decoder", None) or Wav2Vec2_PR.decoder
    beam = {k: v for k, v in (("beam_size", getattr(args_cfg, "beam_size", None)),
                              ("log_add", getattr(args_cfg, "beam_log_add", None))) if v is not None}
    if beam:
        model.beam_options = dict(Wav2Vec2_PR.beam_options, **beam)
    optimizer, lr_scheduler = loops.adam_and_schedule(model.parameters(), args_cfg, publish_to=model)
    return model, optimizer, lr_scheduler


def train(cfg, model, optimizer, lr_scheduler, vocab, train_dataloader, valid_dataloader, best_ckpt_path, last_ckpt_path,
          all_ckpt_path, log=print):
    """train/train_phoneme_recognizer.py:384-505.  Returns the per-epoch log dicts."""
    run = loops.EpochDriver(cfg, model, optimizer, lr_scheduler, best_ckpt_path)
    frontend = run.frontend                  # not None: the loaders use collate_pr_raw
    last_ckpt_path, all_ckpt_path = Path(last_ckpt_path), Path(all_ckpt_path)
    last_ckpt_path.mkdir(parents=True, exist_ok=True)
    if cfg.save_all_epochs:
        all_ckpt_path.mkdir(parents=True, exist_ok=True)

    def save_epoch_and_last(epoch):
        if cfg.save_all_epochs:
            torch.save(model.state_dict(), all_ckpt_path / f"e{epoch:04d}.bin")
            if not (all_ckpt_path / "model_cfg.pkl").exists():
                pickle.dump(model.get_config(), open(all_ckpt_path / "model_cfg.pkl", "wb"))
        torch.save(optimizer.state_dict(), last_ckpt_path / "optimizer.pt")
        if run.ema:                              # cfg.ema_decay: the averages a resumed run continues from
            torch.save(optimizer.ema_state_dict(), last_ckpt_path / "ema.pt")
        torch.save({"last_epoch": cfg.num_epochs}, last_ckpt_path / "scheduler.pt")          # as written (:484)
        loops.save_checkpoint(model, last_ckpt_path)

    for epoch in range(cfg.num_epochs):
        epoch_train_steps = int(cfg.samples_per_epoch / cfg.batch_size)
        # a random subset of this epoch's batches is trained on, the others are skipped (:406,413); `random` is the module the
        # reference draws from, so `random.seed` reproduces an epoch's subset
        subset_random = set(random.sample(range(len(train_dataloader)), epoch_train_steps))
        model.train()
        for batch_idx, batch_x in enumerate(train_dataloader):
            if batch_idx not in subset_random:
                continue
            if getattr(cfg, "graphed", False):
                outputs = run.graphed_step(_to_device(batch_x, cfg.device, frontend, host_lengths=True, augment=True))
            else:
                batch_x = _to_device(batch_x, cfg.device, frontend, augment=True)          # cfg.speed_perturb: the train step only
                outputs = run.eager_step(lambda: model(**batch_x))
            log(f"\tepoch {epoch + 1} ~ batch {run.steps}/{epoch_train_steps}, train_loss: {float(outputs['loss'].detach()):.4f}")
        epoch_log = run.end_epoch(epoch, lambda: validate(model, cfg.device, vocab, epoch, valid_dataloader,
                                                          device_metrics=getattr(cfg, "device_metrics", False),
                                                          batch_invariant=getattr(cfg, "batch_invariant_eval", False), frontend=frontend),
                                  planned_steps=epoch_train_steps, extra_checkpoints=lambda: save_epoch_and_last(epoch))
        log(f"Epoch {epoch + 1}/{cfg.num_epochs} -> lr: {epoch_log['lr']}| mean_train_loss: {epoch_log['mean_train_loss']}| "
            f"mean_val_loss: {epoch_log['mean_val_loss']}| val_per: {epoch_log['mean_val_per']}")
    return run.close()


def _decode_ids(model, outputs):
    """(ids int32 [B][slots] zero-padded, n int32 [B]) on the device, over all frames of the fp32 logits the forward just produced:
    the best path (aptai_ctc_greedy_decode) unless the model's `decoder` says "flashlight" or "beam" (Wav2Vec2_PR._decode_device)."""
    lg = outputs["phoneme_logits"].float().contiguous()
    B, T, V = lg.shape
    if getattr(model, "decoder", "best_path") != "best_path":
        out = SimpleNamespace(_geom=SimpleNamespace(B=B, T=T, Tp=T), _logits_full=lg.view(B * T, V))
        return model._decode_device(out, T + 2)
    from . import ops
    return ops.ctc_greedy_decode(lg, V, T, B, T, V, model._blank(), T)


def _decode(model, outputs) -> list:
    """`_ctc_decode(vocab, phoneme_logits)` (utility.py:448-471) for the batch-1 logits: `_decode_ids`, read back."""
    ids, n = _decode_ids(model, outputs)
    return [int(i) for i in ids[0, :int(n[0])].cpu().numpy()]


def _device_eval(model, device, dl, acc, with_loss, laptop=False, frontend=None):
    """validate()/test() with `device_metrics=True`: the decode's ids and lengths go straight into the device
    Levenshtein kernel; nothing is read back before `acc.result()`.  Any batch size (label counts from the -100 padding)."""
    from . import device_metrics as dm
    for batch_idx, batch_x in enumerate(dl):
        if laptop and batch_idx >= 1:
            break
        with torch.no_grad():
            batch_x = _to_device(batch_x, device, frontend)
            outputs = model(**batch_x)
        if with_loss:
            acc.add_loss(outputs["loss"])
        ids, n = _decode_ids(model, outputs)
        labels = batch_x["phoneme_labels"]
        acc.add_edit(labels, dm.label_lengths(labels), ids, n)
    return acc.result()


@loops.batch_invariant_eval
def validate(model, device, vocab, epoch, validate_dataloader, log_step=100, device_metrics=False, frontend=None) -> Dict[str, float]:
    """train/train_phoneme_recognizer.py:509-561, batch size 1.  `device_metrics=True` (opt-in): the edit distances stay on the
    device (aptai_amd.device_metrics), one device->host transfer per call."""
    if device_metrics:
        from .device_metrics import EvalAccumulator
        return _device_eval(model, device, validate_dataloader, EvalAccumulator("pr_val"), True, frontend=frontend)
    val_losses, edit_d, n_phn = [], [], []
    for batch_x in validate_dataloader:
        with torch.no_grad():
            phoneme_label = batch_x["phoneme_labels"].numpy()[0]
            batch_x = _to_device(batch_x, device, frontend)
            outputs = model(**batch_x)
        val_losses.append(outputs["loss"].item())
        edit_d.append(metrics.edit_distance(phoneme_label, _decode(model, outputs)))
        n_phn.append(len(phoneme_label))
    return metrics.eval_summary("pr_val", edit_d, n_phn, losses=val_losses)


@loops.batch_invariant_eval
def test(model, device, vocab, test_dl, dataset_name, log_step=100, laptop=False, device_metrics=False, frontend=None) -> Dict[str, float]:
    """train/train_phoneme_recognizer.py:566-617."""
    edit_d, n_phn = [], []
    model.eval()
    if device_metrics:
        from .device_metrics import EvalAccumulator
        return _device_eval(model, device, test_dl, EvalAccumulator("pr_test"), False, laptop=laptop, frontend=frontend)
    for batch_idx, batch_x in enumerate(test_dl):
        if laptop and batch_idx >= 1:
            break
        with torch.no_grad():
            phoneme_label = batch_x["phoneme_labels"].numpy()[0]
            batch_x = _to_device(batch_x, device, frontend)
            outputs = model(**batch_x)
        edit_d.append(metrics.edit_distance(phoneme_label, _decode(model, outputs)))
        n_phn.append(len(phoneme_label))
    return metrics.eval_summary("pr_test", edit_d, n_phn)


def default_cfg(**kw):
    """Hyper-parameters at the reference's argparse defaults / start_train_phoneme_recognizer.sh (bs 2, lr 5e-6)."""
    return loops.default_cfg(kw, batch_size=2, samples_per_epoch=8, learning_rate=5e-6, target_metric="mean_val_per", final_dropout=0.1,
                             num_hidden_layers=None, freeze_feature_extractor=False, save_all_epochs=False, cache_dir=None)


def language_model(args, vocab, train_dataset):
    """The n-gram of --lm_arpa / --lm_order (ngram.NGramLM) over the vocabulary in id order, or None: read from an ARPA file, or
    estimated once, on the host, from the `phoneme_label` of every training item (interpolated Witten-Bell)."""
    from .ngram import NGramLM
    tokens = sorted(vocab, key=vocab.get)
    blank = int(vocab.get("(blank)", 0))
    if args.lm_arpa is not None:
        return NGramLM.from_arpa(args.lm_arpa, tokens, blank=blank)
    if args.lm_order is not None:
        return NGramLM.estimate((train_dataset[i]["phoneme_label"] for i in range(len(train_dataset))), tokens, order=args.lm_order,
                                blank=blank)
    return None


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model_dir", default=None, help="local wav2vec2 checkpoint directory (config.json + weights)")
    ap.add_argument("--random_init", default="base", choices=["base", "large"])
    ap.add_argument("--num_epochs", type=int, default=2)
    ap.add_argument("--samples_per_epoch", type=int, default=64)
    ap.add_argument("--train_items", type=int, default=128)
    ap.add_argument("--val_items", type=int, default=4)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--learning_rate", type=float, default=5e-6)
    loops.add_shared_arguments(ap)
    ap.add_argument("--save_all_epochs", action="store_true")
    ap.add_argument("--decoder", default=None, choices=["best_path", "flashlight", "beam"],
                    help="decoder behind the PER of validate() / test(): the frame argmax (default), the reference's decoder call in "
                         "closed form, or the lexicon-free CTC beam search on the device")
    ap.add_argument("--beam_size", type=int, default=None, help="with --decoder beam: hypotheses kept per frame, 1..32 (default 10)")
    ap.add_argument("--beam_log_add", action="store_true", default=None,
                    help="with --decoder beam: sum the scores of hypotheses with equal history (true prefix scores) instead of the maximum")
    ap.add_argument("--lm_arpa", default=None, metavar="PATH",
                    help="with --decoder beam: fuse the token n-gram of this ARPA file into the search (words = the vocabulary's tokens)")
    ap.add_argument("--lm_order", type=int, default=None, metavar="N",
                    help="with --decoder beam: estimate an N-gram (1..5) from the training set's phoneme labels before the first epoch")
    ap.add_argument("--lm_weight", type=float, default=None, metavar="W", help="with an LM: its weight in the search (default 1.0)")
    ap.add_argument("--out", default="pr_exp")
    a = ap.parse_args(argv)
    if (a.lm_arpa is not None or a.lm_order is not None or a.lm_weight is not None) and a.decoder != "beam":
        ap.error("--lm_arpa / --lm_order / --lm_weight need --decoder beam")
    if a.lm_arpa is not None and a.lm_order is not None:
        ap.error("--lm_arpa and --lm_order exclude each other")
    if a.lm_weight is not None and a.lm_arpa is None and a.lm_order is None:
        ap.error("--lm_weight needs --lm_arpa or --lm_order")
    return a


def main(argv=None):
    a = parse_args(argv)
    vocab = default_vocab()
    w2v = W2V2Config.base() if a.random_init == "base" else W2V2Config.large()
    loops.apply_mask_feature_arguments(w2v, a)
    with tempfile.TemporaryDirectory() as tmp:
        model_dir = a.model_dir
        if model_dir is None:
            torch.manual_seed(0)
            Wav2Vec2Model(w2v).save_pretrained(tmp)
            model_dir = tmp
        cfg = default_cfg(num_epochs=a.num_epochs, batch_size=a.batch_size, samples_per_epoch=a.samples_per_epoch,
                          learning_rate=a.learning_rate, save_all_epochs=a.save_all_epochs, huggingface_model_id=model_dir,
                          pretrain_cfg=w2v, decoder=a.decoder, beam_size=a.beam_size, beam_log_add=a.beam_log_add,
                          **loops.shared_arguments(a))
        model, optimizer, lr_scheduler = load_model_optimizer(cfg, vocab)
    collate = hostlogic.collate_pr_raw if loops.uses_frontend(a) else hostlogic.collate_pr
    tr = torch.utils.data.DataLoader(SyntheticCommonPhone(a.train_items, a.seconds, len(vocab), seed=1, source_rate=a.source_rate),
                                     batch_size=a.batch_size, shuffle=True, drop_last=True, collate_fn=collate)
    va = torch.utils.data.DataLoader(SyntheticCommonPhone(a.val_items, a.seconds, len(vocab), seed=2, source_rate=a.source_rate),
                                     batch_size=1, collate_fn=collate)
    lm = language_model(a, vocab, tr.dataset)
    if lm is not None:          # validate() / test() decode with it: Wav2Vec2_PR.beam_options reaches ops.ctc_beam_search
        model.beam_options = dict(model.beam_options, lm=lm, lm_weight=1.0 if a.lm_weight is None else a.lm_weight)
    out = Path(a.out)
    return train(cfg, model, optimizer, lr_scheduler, vocab, tr, va, out / "best-model-ckpt", out / "last-model-ckpt", out / "model-ckpts")


if __name__ == "__main__":
    main()
