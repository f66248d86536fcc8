#!/usr/bin/env python3
"""Cost of the attention maps (output_attentions=True) and of a loss on them (run on the GPU box).

At 16 x 10 s wav2vec2-base (12 heads, T = 499, Tp = 512) and 8 x 10 s wav2vec2-large (16 heads), device events, warmed up:
  aptai_attention_probs_fwd   microseconds per launch; algorithmic bytes = the fp32 map written (B heads T T 4) + Q, K and lse2 read
  aptai_attention_probs_bwd   (two kernels) microseconds per call; algorithmic bytes = the map's gradient read ONCE + Q, K, lse2 read
                              + dQ, dK read and written (accumulate form)
each as bytes/s and as a share of the 6.29 TB/s HBM roof the project judges its HBM-bound kernels by.
Alternating with them in the same process, what a user had to do before to get the same tensor: torch.softmax of a masked torch.matmul
of the bf16 Q and K slices in fp32, and its autograd backward.  Prints one line per figure and a JSON summary line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aptai_amd import ops

ROOF = 6.29e12


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def case(name, B, heads, T, res, rounds=5, iters=10):
    dev = "cuda"
    H, Tp = heads * 64, (T + 2 + 127) // 128 * 128
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * Tp, 3 * H, generator=g).to(torch.bfloat16)
    qs = qkv.view(B * Tp, 3, H)
    qs[:, 0] = (qs[:, 0].float() * ops.attention_qscale(H, heads)).to(torch.bfloat16)
    qkv = qkv.to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    _, st = ops.attention_fwd(qkv, lens, B, Tp, H, heads, q_prescaled=True)
    dprobs = torch.randn(B, heads, Tp, Tp, generator=g).to(dev)
    dqkv = torch.zeros_like(qkv)
    # the composition a user had to write: fp32 scores from the bf16 slices, key mask, softmax
    q4 = qkv.view(B, Tp, 3, heads, 64)
    mask = (torch.arange(Tp, device=dev)[None, :] >= lens[:, None])[:, None, None, :]

    def torch_fwd(q, k):
        s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * (0.6931471805599453)      # q carries log2(e) / 8
        return torch.softmax(s.masked_fill(mask, float("-inf")), -1)
    qh = q4[:, :, 0].permute(0, 2, 1, 3).contiguous()
    kh = q4[:, :, 1].permute(0, 2, 1, 3).contiguous()
    qg, kg = qh.clone().requires_grad_(True), kh.clone().requires_grad_(True)

    def torch_fwd_bwd():
        qg.grad = kg.grad = None
        torch_fwd(qg, kg).backward(dprobs)
    f_new = lambda: ops.attention_probs_fwd(qkv, lens, st[0], B, Tp, H, heads, q_prescaled=True)      # noqa: E731
    b_new = lambda: ops.attention_probs_bwd(qkv, lens, st[0], dprobs, B, Tp, H, heads, q_prescaled=True, dqkv=dqkv)      # noqa: E731
    f_old = lambda: torch_fwd(qh, kh)      # noqa: E731
    fns = {"fwd": f_new, "bwd": b_new, "torch_fwd": f_old, "torch_fwd_bwd": torch_fwd_bwd}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):                                     # alternate, so that clocks and neighbours hit all of them alike
        for k, fn in fns.items():
            t[k].append(_time(fn, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    map_bytes = B * heads * T * T * 4
    opnd = 2 * B * T * H * 2 + B * heads * T * 4
    fwd_bytes = map_bytes + opnd
    bwd_bytes = map_bytes + opnd + 2 * (2 * B * T * H * 2)
    for k, nbytes in (("fwd", fwd_bytes), ("bwd", bwd_bytes)):
        bw = nbytes / (med[k] * 1e-6)
        print(f"{name} aptai_attention_probs_{k}: {med[k]:.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f}), {nbytes / 1e6:.1f} MB algorithmic, "
              f"{bw / 1e12:.2f} TB/s = {100 * bw / ROOF:.0f} % of the 6.29 TB/s roof")
        res[f"{name}_{k}_us"], res[f"{name}_{k}_roof_share"] = round(med[k], 1), round(bw / ROOF, 3)
    print(f"{name} torch matmul + mask + softmax (fp32): {med['torch_fwd']:.1f} us = {med['torch_fwd'] / med['fwd']:.2f} x the kernel; "
          f"with its autograd backward {med['torch_fwd_bwd']:.1f} us = {med['torch_fwd_bwd'] / (med['fwd'] + med['bwd']):.2f} x fwd + bwd")
    res[f"{name}_torch_fwd_us"], res[f"{name}_torch_fwd_bwd_us"] = round(med["torch_fwd"], 1), round(med["torch_fwd_bwd"], 1)


if __name__ == "__main__":
    res = {}
    case("base_16x10s", 16, 12, 499, res)
    case("large_8x10s", 8, 16, 499, res)
    print(json.dumps(res))
