#!/usr/bin/env python3
"""Launch time of the forced alignment (aptai_ctc_viterbi) beside the CTC forward it shares a lattice with (run on the GPU box).

Shapes: 16 x 499 x 46 with 60 labels (the flagship batch) and 16 x 1499 x 46 with 200 labels (30 s utterances).  For each,
device events around `iters` back-to-back calls of the C entry point on preallocated buffers, warmed up, random logits and
transcripts, the two entry points alternating round by round so that clocks and neighbours hit them alike:
  aptai_ctc_viterbi           gather + max-plus recursion with backpointers + backtrace + spans / scores   (3 launches)
  aptai_ctc_fwd(want_beta=0)  log-softmax gather + sum-product alpha recursion + loss reduction            (3 launches)
The second is the yardstick: it walks the same lattice once with costlier arithmetic; the alignment adds one more sequential pass
(the backtrace), so it should come in at or under twice that figure.  Also prints where each shape kept its backpointers (LDS when
the utterance's frames x 64 lanes x word size fit 64 KB, else the workspace, staged back through LDS in chunks).  One line per
figure and a JSON summary line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aptai_amd import _lib, ops


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def case(name, B, T, V, L, res, rounds=7, iters=50):
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(B * T, V, generator=g) * 3).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32).to(dev)
    in_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    t_lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    L_ = _lib.lib()
    ws_v = torch.empty(L_.aptai_ctc_viterbi_workspace_bytes(B, T, L), device=dev, dtype=torch.uint8)
    ws_f = torch.empty(L_.aptai_ctc_workspace_bytes(B, T, L) // 4, device=dev, dtype=torch.float32)
    ft = torch.empty((B, T), device=dev, dtype=torch.int32)
    spans = torch.empty((B, L, 2), device=dev, dtype=torch.int32)
    score, nll, loss = (torch.empty(n, device=dev, dtype=torch.float32) for n in (B, B, 1))
    tsc = torch.empty((B, L), device=dev, dtype=torch.float32)
    stream = ops._stream()

    def viterbi():
        _lib.call("aptai_ctc_viterbi", logits.data_ptr(), V, T, targets.data_ptr(), L, in_lens.data_ptr(), t_lens.data_ptr(), None, B, T, V,
                  0, 0, ws_v.data_ptr(), ft.data_ptr(), spans.data_ptr(), score.data_ptr(), tsc.data_ptr(), stream)

    def ctc_fwd():
        _lib.call("aptai_ctc_fwd", logits.data_ptr(), V, T, targets.data_ptr(), L, in_lens.data_ptr(), t_lens.data_ptr(), None, B, T, V,
                  0, 1, 1, None, ws_f.data_ptr(), nll.data_ptr(), loss.data_ptr(), 0, stream)
    fns = {"viterbi": viterbi, "ctc_fwd": ctc_fwd}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.isfinite(score).all() and torch.isfinite(nll).all()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_time(fn, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    ns = (2 * L + 1 + 63) // 64
    word = 2 if ns > 4 else 1
    store = "LDS" if T * 64 * word <= 65536 else "workspace, staged through LDS"
    ratio = med["viterbi"] / med["ctc_fwd"]
    for k in fns:
        print(f"{name} aptai_{k}: {med[k]:.1f} us per call (min {min(t[k]):.1f}, max {max(t[k]):.1f})")
    print(f"{name} viterbi / ctc_fwd = {ratio:.2f} (target <= 2); backpointers: {store}")
    res[f"{name}_viterbi_us"], res[f"{name}_ctc_fwd_us"] = round(med["viterbi"], 1), round(med["ctc_fwd"], 1)
    res[f"{name}_ratio"], res[f"{name}_backpointers"] = round(ratio, 2), store


if __name__ == "__main__":
    res = {}
    case("16x499x46_L60", 16, 499, 46, 60, res)
    case("16x1499x46_L200", 16, 1499, 46, 200, res)
    print(json.dumps(res))
