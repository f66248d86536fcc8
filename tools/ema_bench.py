#!/usr/bin/env python3
"""What the exponential moving average of the weights costs beside the Adam launch (run on the GPU box).

The parameter set of the wav2vec2-base APTAI model (shapes from oracle.synth, ~95 M fp32 parameters, no model is built), one
aptai_amd.optim.Adam(ema_decay=0.999) on it, two averaged steps so that every table exists, then the launches themselves on those
tables, alternating round by round inside one process:
  adam  aptai_adam_multi   reads p, m, v, g, writes p, m, v    28 B per parameter
  ema   aptai_ema_multi    reads p, ema, writes ema            12 B per parameter
  swap  aptai_swap_multi   reads and writes p and ema          16 B per parameter (an even number of launches: the weights come back)
Device events around `iters` back-to-back launches, warmed up; median, min and max of the rounds, the implied bytes per second and the
ratio ema / adam (bytes say 12/28 = 0.43).  One line per figure and a JSON summary."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aptai_amd import ops
from aptai_amd.config import W2V2Config
from aptai_amd.optim import Adam
from oracle import synth


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main(rounds=9, iters=20):
    shapes = [s for n, s in synth.aptai_param_shapes(W2V2Config.base(vocab_size=46)).items() if "lowpass" not in n]
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).cuda() * 0.02) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).cuda() * 1e-2
    opt = Adam(ps, lr=1e-5, ema_decay=0.999)
    opt.step()
    opt.step()
    t, ema = opt._table, opt._ema                                                       # one group: its rows are the whole job table
    gi, r0, r1, max_n = t.groups[0]
    stream = torch.cuda.current_stream().cuda_stream
    tab, ptrs, n = t.table_ptr, ema.ptrs_dev.data_ptr(), t.n
    fns = {"adam": lambda: opt._launch(t, gi, 0, r0, r1, max_n, None, stream),          # the per-step rows of the last step()
           "ema": lambda: ops.ema_multi(tab, ptrs, n, max_n, 1.0 - 0.999),
           "swap": lambda: ops.swap_multi(tab, ptrs, n, max_n)}
    for fn in fns.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    n_par = sum(p.numel() for p in ps)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(_time(fn, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    nbytes = {"adam": 28, "ema": 12, "swap": 16}
    tb = {k: nbytes[k] * n_par / med[k] / 1e6 for k in fns}
    print(f"{len(shapes)} tensors, {n_par / 1e6:.1f} M parameters, grid {(max_n + 4095) // 4096} x {n}")
    for k in fns:
        print(f"{k}: {med[k]:.1f} us (min {min(times[k]):.1f}, max {max(times[k]):.1f}) over {rounds} rounds of {iters} launches; "
              f"{nbytes[k]} B per parameter = {nbytes[k] * n_par / 1e9:.2f} GB, {tb[k]:.2f} TB/s")
    print(f"ema / adam = {med['ema'] / med['adam']:.3f} (bytes say 12/28 = 0.429); swap / adam = {med['swap'] / med['adam']:.3f} (16/28 = 0.571)")
    print(json.dumps({"params_M": round(n_par / 1e6, 1), **{f"{k}_us": round(v, 1) for k, v in med.items()},
                      **{f"{k}_TBps": round(v, 3) for k, v in tb.items()}, "ema_over_adam": round(med["ema"] / med["adam"], 3)}))


if __name__ == "__main__":
    main()
