"""CPU: pin the attention-map fixtures (tests/golden/attn_{base,large}_2x1s.npz, written by tests/golden/make_golden_attn.py from the
reference's eager attention) and the oracle to each other: the stored maps equal softmax(q_proj(x) d^-1/2 k_proj(x)^T + key mask)
recomputed here from the oracle's hidden states and the synthetic weights.  fp32 CPU vs fp32 CPU: rounding order only (measured max
absolute difference 2.1e-7 to 4.8e-7 per layer, largest probability 0.25-0.45; bound 5e-6, ten times that, because fp32 summation order
differs between hosts)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import synth, w2v2_ref
from aptai_amd.config import W2V2Config


def _maps_from_oracle(name, shapes_fn):
    z, meta = load_golden(name)
    cfg = W2V2Config.from_any(meta["cfg"])
    sd = synth.make_state_dict(shapes_fn(cfg), meta["seed"])
    audio = torch.from_numpy(np.asarray(z["in/audio"]))
    lengths = torch.from_numpy(np.asarray(z["in/lengths"]))
    with torch.no_grad():
        out = w2v2_ref.wav2vec2_forward(sd, cfg, audio, lengths)
    km = out["frame_mask"]
    nh = cfg.num_attention_heads
    maps = {}
    for l in meta["maps_layers"]:
        p = f"wav2vec2.encoder.layers.{l}."
        x = out["hidden_states"][l]
        if cfg.do_stable_layer_norm:                            # pre-LN: the attention block reads the normalised stream
            x = F.layer_norm(x, (x.shape[-1],), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], cfg.layer_norm_eps)
        B, T, H = x.shape
        d = H // nh
        q = F.linear(x, sd[p + "attention.q_proj.weight"], sd[p + "attention.q_proj.bias"]).view(B, T, nh, d).transpose(1, 2)
        k = F.linear(x, sd[p + "attention.k_proj.weight"], sd[p + "attention.k_proj.bias"]).view(B, T, nh, d).transpose(1, 2)
        w = torch.matmul(q * d ** -0.5, k.transpose(2, 3))
        w = w.masked_fill(~km[:, None, None, :], torch.finfo(w.dtype).min)
        maps[l] = torch.softmax(w, -1).numpy()
    return z, meta, km.numpy(), maps


@pytest.mark.parametrize("name,shapes", [("attn_base_2x1s", "pr_param_shapes"), ("attn_large_2x1s", "aptai_param_shapes")])
def test_fixture_maps_equal_the_softmax_of_the_oracle(name, shapes):
    z, meta, km, maps = _maps_from_oracle(name, getattr(synth, shapes))
    assert meta["lengths"] == [16000, 9000] and meta["frames"] == 49 and list(km.sum(1)) == [49, 27]
    for l, got in maps.items():
        ref = np.asarray(z[f"attn/{l}"])
        assert ref.dtype == np.float32 and ref.shape == (2, meta["heads"], 49, 49)
        err = float(np.abs(got - ref).max())
        print(f"[attn-oracle] {name} layer {l}: max abs diff {err:.2e} (largest probability {ref.max():.3f})")
        assert err <= 5e-6
        assert (ref[1][:, :, 27:] == 0).all()                   # padded key columns: exactly zero
        assert np.abs(ref.sum(-1) - 1).max() <= 1e-6            # every row, padded query rows included, is a distribution
    # the backward fixtures are not degenerate
    assert abs(float(z["loss"])) > 1 and np.linalg.norm(np.asarray(z["grad/audio"])) > 5
