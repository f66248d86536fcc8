#!/usr/bin/env python3
"""What global-norm gradient clipping and gradient accumulation cost in `optimizer.step()` (run on the GPU box).

The parameter set of the wav2vec2-base APTAI model (shapes from oracle.synth, ~95 M fp32 parameters, no model is built), random
gradients, five optimisers on their own parameter copies:
  off      aptai_amd.optim.Adam(...)                             one aptai_adam_multi launch                   (the default step)
  fused    aptai_amd.optim.Adam(..., max_grad_norm=1.0)          two norm launches + one aptai_adam_multi_scaled
  twopass  aptai_amd.optim.clip_grad_norm_(params, 1.0) + off    two norm launches + aptai_scale_multi + aptai_adam_multi
  accum        Adam(..., gradient_accumulation_steps=2**30)      a micro-step inside a window: one aptai_grad_accum_multi launch
  accum_close  Adam(..., gradient_accumulation_steps=2), its     a micro-step that closes its window: aptai_grad_accum_multi with
               window marked as one micro-step old before each   scale 1/2, then aptai_adam_multi on the accumulators
Device events around `iters` back-to-back steps, warmed up, the five alternating round by round inside one process so that clocks and
neighbours hit them alike; median, min and max of the rounds.  Expected: the norm pass reads 4 of the 28 bytes per parameter the
Adam launch moves, so fused - off is about one seventh of `off` plus a one-block launch; the accumulate launch moves 12 bytes per
parameter, three sevenths of `off`.  Bytes per second of `accum` and `off` are reported side by side (both stream the same chunks).
One line per figure and a JSON summary."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aptai_amd.config import W2V2Config
from aptai_amd.optim import Adam, clip_grad_norm_
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
    grads = [torch.randn(s, generator=g).cuda() * 1e-2 for s in shapes]
    sets = {}
    for k in ("off", "fused", "twopass", "accum", "accum_close"):
        ps = [torch.nn.Parameter(torch.randn(s, generator=g).cuda() * 0.02) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()                     # twopass rescales its copies in place every step: each set owns its gradients
        sets[k] = (ps, Adam(ps, lr=1e-5, max_grad_norm=1.0 if k == "fused" else None,
                            gradient_accumulation_steps={"accum": 2 ** 30, "accum_close": 2}.get(k, 1)))

    def twopass():
        clip_grad_norm_(sets["twopass"][0], 1.0)
        sets["twopass"][1].step()

    def accum_close():
        # every call is the SECOND micro-step of a window of two: the first one is replaced by marking the window as holding one
        # micro-step in which every row contributed (host flags only; the accumulators keep whatever the last close left, the
        # kernels' time does not depend on the values)
        opt = sets["accum_close"][1]
        acc = opt._accum
        acc.seen, acc.k = [True] * len(acc.seen), 1
        opt.step()
    opt = sets["accum_close"][1]
    opt.step()
    opt.step()                                      # one whole window: the accumulators exist
    fns = {"off": sets["off"][1].step, "fused": sets["fused"][1].step, "twopass": twopass, "accum": sets["accum"][1].step,
           "accum_close": accum_close}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    opt = sets["fused"][1]
    n_par = sum(p.numel() for p in sets["off"][0])
    print(f"{len(shapes)} tensors, {n_par / 1e6:.1f} M parameters; fused: grad norm {float(opt.last_grad_norm):.4f}, "
          f"coefficient {float(opt.last_clip_coef):.6f}, {int(opt._clip_result[2])} gradient elements")
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_time(fn, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for k in fns:
        print(f"optimizer.step() {k}: {med[k]:.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f}) over {rounds} rounds of {iters} steps")
    print(f"fused - off = {med['fused'] - med['off']:.1f} us ({(med['fused'] / med['off'] - 1) * 100:.1f} %; bytes say "
          f"{med['off'] / 7:.1f} us + a one-block launch); twopass - off = {med['twopass'] - med['off']:.1f} us")
    # bytes: aptai_adam_multi reads p, m, v, g and writes p, m, v (28 B per parameter; these sets publish no compute copies),
    # aptai_grad_accum_multi reads acc, g and writes acc (12 B)
    tb = {"off": 28 * n_par / med["off"] / 1e6, "accum": 12 * n_par / med["accum"] / 1e6}
    print(f"accum = {med['accum']:.1f} us = {med['accum'] / med['off']:.3f} of off (bytes say 3/7 = 0.429); "
          f"{tb['accum']:.2f} TB/s against {tb['off']:.2f} TB/s of aptai_adam_multi ({(tb['accum'] / tb['off'] - 1) * 100:+.1f} %)")
    print(f"accum_close = {med['accum_close']:.1f} us; accum_close - off = {med['accum_close'] - med['off']:.1f} us "
          f"(the accumulate launch with scale 1/2 in front of the Adam launch)")
    print(json.dumps({"params_M": round(n_par / 1e6, 1), **{f"{k}_us": round(v, 1) for k, v in med.items()},
                      "fused_minus_off_us": round(med["fused"] - med["off"], 1), "twopass_minus_off_us": round(med["twopass"] - med["off"], 1),
                      "accum_close_minus_off_us": round(med["accum_close"] - med["off"], 1),
                      "off_TBps": round(tb["off"], 3), "accum_TBps": round(tb["accum"], 3)}))


if __name__ == "__main__":
    main()
