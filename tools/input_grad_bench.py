#!/usr/bin/env python3
"""Cost of gradients w.r.t. the input waveform (run on the GPU box).

1. aptai_conv0_bwd_data against aptai_conv0_bwd on the same shapes in the same process: 16 x 10 s, group mode (wav2vec2-base) and
   layer mode (wav2vec2-large: conv bias + LayerNorm).
2. The eager APTAI step (forward + backward, wav2vec2-base shape, frozen conv stack) at 16 x 10 s without and with
   audio_inputs.requires_grad_().
Prints one line per figure and a JSON summary line."""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aptai_amd import ops
from tools.gemm_round import bench

TV = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")


def kernels(res):
    B, S = 16, 160000
    g = torch.Generator().manual_seed(1)
    dev = "cuda"
    audio = torch.randn(B, S, generator=g).to(dev)
    w = (torch.randn(512, 1, 10, generator=g) * 0.3).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(512, generator=g)).to(dev)
    beta = (0.1 * torch.randn(512, generator=g)).to(dev)
    bias = (0.1 * torch.randn(512, generator=g)).to(dev)
    T = (S - 10) // 5 + 1
    Ta = (T + 63) // 64 * 64
    dy = (torch.randn(B, Ta, 512, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    dy[:, T:] = 0
    for mode, name, bb in ((0, "group", None), (1, "layer", bias)):
        out = torch.empty(B, Ta, 512, device=dev, dtype=torch.bfloat16)
        stats = ops.conv0_fwd(audio, w, bb, gamma, beta, mode, out, T, Ta, want_stats=True)
        t_w = bench(lambda: ops.conv0_bwd(audio, w, bb, gamma, beta, mode, dy, T, Ta, stats), iters=20)
        t_d = bench(lambda: ops.conv0_bwd_data(audio, w, bb, gamma, beta, mode, dy, T, Ta, stats), iters=20)
        print(f"{name} mode 16 x 10 s: aptai_conv0_bwd {t_w:.0f} us, aptai_conv0_bwd_data {t_d:.0f} us, ratio {t_d / t_w:.3f}")
        res[f"{name}_conv0_bwd_us"], res[f"{name}_conv0_bwd_data_us"] = round(t_w, 1), round(t_d, 1)


def step(res, steps=10, warmup=3):
    from safetensors.torch import save_file
    from aptai_amd.aptai import APTAI
    from aptai_amd.config import W2V2Config
    from oracle import synth
    cfg = W2V2Config.base(vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "config.json"), "w") as f:
            json.dump(cfg.to_dict(), f)
        save_file({k[len("wav2vec2."):]: v.contiguous() for k, v in sd.items() if k.startswith("wav2vec2.")},
                  os.path.join(tmp, "model.safetensors"))
        model = APTAI("cuda", {f"p{i}": i for i in range(46)}, tmp, cfg, None)
    model.load_state_dict(sd)
    model = model.cuda().train()
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 16, 160000, seed=3).items()}
    for want in (False, True):
        def one():
            model.zero_grad(set_to_none=True)
            b = dict(batch)
            if want:
                b["audio_inputs"] = batch["audio_inputs"].clone().requires_grad_(True)
            model(0, **b)["loss"].backward()
        for _ in range(warmup):
            one()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            one()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        key = "step_input_grad_ms" if want else "step_ms"
        res[key] = round(ms, 3)
        print(f"eager APTAI base step 16 x 10 s, audio requires grad = {want}: {ms:.2f} ms")


if __name__ == "__main__":
    res = {}
    kernels(res)
    step(res)
    print(json.dumps(res))
