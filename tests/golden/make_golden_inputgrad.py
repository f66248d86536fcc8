#!/usr/bin/env python3
"""Generate tests/golden/inputgrad_2x1s.npz: gradients w.r.t. the INPUT WAVEFORM of the unmodified reference.

Same setting as make_golden.py (whose helpers, stand-in modules and reference imports this file reuses without changing it): runs only
where the reference checkout exists, never on the GPU box, never from pytest.  Synthetic weights (oracle.synth), synthetic ragged batches.

  group/*  Wav2Vec2_PR.get_embeddings_grad, wav2vec2-base shape (GroupNorm conv stack, post-LN), 3 layers, 2 x 1 s, eval mode:
           d/d(waveform) of sum(phoneme_logits_inter**2) + sum(phoneme_logits_last**2) (the loss of case_pr_embgrad).
  layer/*  APTAI as shipped (wav2vec2-large, 24 layers: the reference hard-codes hidden_states[24] and 1024-wide heads), 2 x 1 s,
           train mode with head dropouts and regularisers at 0 (as case_aptai_large), frozen conv stack (the default):
           d/d(waveform) of loss.backward().

Usage:  python tests/golden/make_golden_inputgrad.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the stand-ins and imports the reference modules)

NAME = "inputgrad_2x1s"


def case_group(seconds=1.0, seed=0, layers=3):
    cfg_kw = dict(mg.BASE, num_hidden_layers=layers, vocab_size=40, ctc_loss_reduction="mean", ctc_zero_infinity=True, blank=0,
                  **mg.NOREG)
    cfg = mg.hf_config(cfg_kw)
    S = int(16000 * seconds)
    batch = mg.synth.synth_pr_batch(cfg, 2, S, seed=77, lo=8, hi=12)
    vocab = {f"p{i}": i for i in range(40)}
    with tempfile.TemporaryDirectory() as tmp:
        model = mg.ref_w2v2_pr.Wav2Vec2_PR(cfg, None, mg.local_model_dir(cfg, tmp), vocab)
    model.load_state_dict(mg.synth.make_state_dict(mg.synth.pr_param_shapes(cfg), seed))
    model.eval()
    audio = batch["input_values"].clone().requires_grad_(True)
    out = model.get_embeddings_grad(audio, batch["input_lengths"], vocab, 1, 2)
    loss = out["phoneme_logits_inter"].pow(2).sum() + out["phoneme_logits_last"].pow(2).sum()
    loss.backward()
    arrays = {"group/in/input_values": batch["input_values"].numpy(), "group/in/input_lengths": batch["input_lengths"].numpy(),
              "group/loss": loss.detach().numpy(), "group/audio_grad": audio.grad.numpy()}
    meta = dict(cfg=cfg_kw, seed=seed, S=S, batch_seed=77, intermediate_hidden=1, latter_hidden=2,
                model="Wav2Vec2_PR.get_embeddings_grad", mode="eval")
    return arrays, meta


def case_layer(seconds=1.0, seed=0):
    cfg_kw = dict(mg.LARGE, vocab_size=46, **mg.NOREG)
    cfg = mg.hf_config(cfg_kw)
    S = int(16000 * seconds)
    batch = mg.synth.synth_aptai_batch(cfg, 2, S, seed=1234)
    vocab = {f"p{i}": i for i in range(46)}
    with tempfile.TemporaryDirectory() as tmp:
        model = mg.ref_aptai.APTAI("cpu", vocab, mg.local_model_dir(cfg, tmp), cfg, None)
    model.load_state_dict(mg.synth.make_state_dict(mg.synth.aptai_param_shapes(cfg), seed))
    model.tv_head[0].p = 0.0
    model.phn_head[0].p = 0.0
    model.train()
    audio = batch["audio_inputs"].clone().requires_grad_(True)
    out = model(0, **dict(batch, audio_inputs=audio))
    out["loss"].backward()
    arrays = {"layer/in/" + k: v.numpy() for k, v in batch.items()}
    arrays["layer/loss"] = out["loss"].detach().numpy()
    arrays["layer/audio_grad"] = audio.grad.numpy()
    arrays["layer/frozen_has_grad"] = np.array(
        [p.grad is not None for n, p in model.named_parameters() if "feature_extractor" in n])
    meta = dict(cfg=cfg_kw, seed=seed, S=S, batch_seed=1234, model="APTAI", mode="train, frozen conv stack, head dropouts 0")
    return arrays, meta


if __name__ == "__main__":
    torch.set_num_threads(8)
    arrays, meta = {}, {}
    for tag, fn in (("group", case_group), ("layer", case_layer)):
        a, m = fn()
        arrays.update(a)
        meta[tag] = m
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    arrays["__meta__"] = np.array(repr(dict(meta, case=NAME, versions=mg.VERSIONS, generator="tests/golden/make_golden_inputgrad.py")))
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}  ({os.path.getsize(path)/1024:.0f} KiB)")
