#!/usr/bin/env python3
"""Generate tests/golden/attn_base_2x1s.npz and attn_large_2x1s.npz: the attention probabilities (`output_attentions=True`) of the
unmodified reference's wav2vec2 encoder and the gradients of a loss on them.

Same setting as make_golden.py (whose helpers, stand-in modules and reference imports this file reuses without changing it): runs only
where the reference checkout exists, never on the GPU box, never from pytest.  Synthetic weights (oracle.synth), synthetic waveforms,
RAGGED lengths set here (16000 and 9000 samples: 49 and 27 frames).

  base   Wav2Vec2_PR's encoder, wav2vec2-base shape (GroupNorm conv stack, post-LN), 3 layers, 12 heads, 2 x 1 s, eval mode.
  large  APTAI's encoder, wav2vec2-large shape (LayerNorm conv stack, pre-LN), 3 layers, 16 heads, 2 x 1 s, eval mode.

Both call `model.wav2vec2(audio, attention_mask=lengths[:, None], ...)` as the reference's own modules do, after
`set_attn_implementation("eager")` (the default sdpa path returns no maps).  Loss: L = sum_l <attentions[l], G>,
G[b, a, i, j] = ((7 i + 13 j + 3 a + b) % 17 - 8) / 8.  Stored per case: the waveform, the lengths, the maps (`maps_layers` in the
meta says of which layers), L, the gradient w.r.t. the waveform, the full gradients of every layer's q_proj.bias, of
feature_projection.projection.bias and of feature_projection.layer_norm.weight, and rows 0-7 of every layer's q_proj.weight and
k_proj.weight gradients.  float32 as computed.

Usage:  python tests/golden/make_golden_attn.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the stand-ins and imports the reference modules)

LENGTHS = [16000, 9000]


def loss_weights(B, heads, T):
    b, a, i, j = torch.meshgrid(torch.arange(B), torch.arange(heads), torch.arange(T), torch.arange(T), indexing="ij")
    return (((7 * i + 13 * j + 3 * a + b) % 17) - 8).float() / 8


def run(model, cfg_kw, audio0, seed, batch_seed, which, maps_layers):
    w = model.wav2vec2
    w.set_attn_implementation("eager")
    model.eval()
    for p in model.parameters():
        p.grad = None
    lengths = torch.tensor(LENGTHS, dtype=torch.long)
    audio = audio0.clone().requires_grad_(True)
    out = w(audio, attention_mask=lengths[:, None], output_attentions=True, output_hidden_states=True, return_dict=True)
    att = out.attentions
    B, heads, T, _ = att[0].shape
    G = loss_weights(B, heads, T)
    loss = sum((a * G).sum() for a in att)
    loss.backward()
    arrays = {"in/audio": audio0.numpy(), "in/lengths": lengths.numpy(), "loss": loss.detach().numpy(), "grad/audio": audio.grad.numpy()}
    for l in maps_layers:
        arrays[f"attn/{l}"] = att[l].detach().numpy()
    named = dict(w.named_parameters())
    arrays["grad/feature_projection.projection.bias"] = named["feature_projection.projection.bias"].grad.numpy()
    arrays["grad/feature_projection.layer_norm.weight"] = named["feature_projection.layer_norm.weight"].grad.numpy()
    for l in range(len(att)):
        pre = f"encoder.layers.{l}.attention."
        arrays[f"grad/{pre}q_proj.bias"] = named[pre + "q_proj.bias"].grad.numpy()
        arrays[f"grad/{pre}q_proj.weight[0:8]"] = named[pre + "q_proj.weight"].grad[0:8].numpy()
        arrays[f"grad/{pre}k_proj.weight[0:8]"] = named[pre + "k_proj.weight"].grad[0:8].numpy()
    meta = dict(cfg=cfg_kw, seed=seed, batch_seed=batch_seed, lengths=LENGTHS, frames=T, heads=heads, layers=len(att), model=which,
                mode="eval", attn_implementation="eager", maps_layers=list(maps_layers),
                loss="sum_l <attentions[l], G>, G[b,a,i,j] = ((7 i + 13 j + 3 a + b) % 17 - 8) / 8")
    return arrays, meta


def case_base(seed=0, layers=3):
    cfg_kw = dict(mg.BASE, num_hidden_layers=layers, vocab_size=40, ctc_loss_reduction="mean", ctc_zero_infinity=True, blank=0,
                  **mg.NOREG)
    cfg = mg.hf_config(cfg_kw)
    batch = mg.synth.synth_pr_batch(cfg, 2, 16000, seed=77, lo=8, hi=12)
    vocab = {f"p{i}": i for i in range(40)}
    with tempfile.TemporaryDirectory() as tmp:
        model = mg.ref_w2v2_pr.Wav2Vec2_PR(cfg, None, mg.local_model_dir(cfg, tmp), vocab)
    model.load_state_dict(mg.synth.make_state_dict(mg.synth.pr_param_shapes(cfg), seed))
    return run(model, cfg_kw, batch["input_values"], seed, 77, "Wav2Vec2_PR.wav2vec2", range(layers))


def case_large(seed=0, layers=3):
    cfg_kw = dict(mg.LARGE, num_hidden_layers=layers, vocab_size=46, **mg.NOREG)
    cfg = mg.hf_config(cfg_kw)
    batch = mg.synth.synth_aptai_batch(cfg, 2, 16000, seed=1234)
    vocab = {f"p{i}": i for i in range(46)}
    with tempfile.TemporaryDirectory() as tmp:
        model = mg.ref_aptai.APTAI("cpu", vocab, mg.local_model_dir(cfg, tmp), cfg, None)
    model.load_state_dict(mg.synth.make_state_dict(mg.synth.aptai_param_shapes(cfg), seed))
    return run(model, cfg_kw, batch["audio_inputs"], seed, 1234, "APTAI.wav2vec2", (0, layers - 1))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for name, fn in (("attn_base_2x1s", case_base), ("attn_large_2x1s", case_large)):
        arrays, meta = fn()
        arrays = {k: np.asarray(v) for k, v in arrays.items()}
        arrays["__meta__"] = np.array(repr(dict(meta, case=name, versions=mg.VERSIONS, generator="tests/golden/make_golden_attn.py")))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {path}  ({os.path.getsize(path)/1024:.0f} KiB)  L = {float(arrays['loss']):.4f}  "
              f"|d audio| = {np.linalg.norm(arrays['grad/audio']):.2f}")
