#!/usr/bin/env python3
"""Launch time of the device CTC beam search (aptai_ctc_beam_search) beside the best-path decode it can replace (run on the GPU box).

Shape: the workload's own, 16 utterances x 499 frames x 46 tokens (pitch 64), random logits (randn * 3: nothing is peaked, so the
beam stays full and the floor prunes little - the costly end).  Device events around `iters` back-to-back calls of the C entry
point on preallocated buffers, warmed up, the entry points alternating round by round so that clocks and neighbours hit them alike:
  aptai_ctc_beam_search, beam 10   the reference's settings (threshold 50, max-merge, 1-best)
  aptai_ctc_beam_search, beam 32   the widest beam, log-add, 32-best
  aptai_ctc_greedy_decode          frame argmax, for scale
  aptai_ctc_beam_search_lm         with --lm ORDER (repeatable): both beams again with a random back-off n-gram of that order
                                   over the 46 tokens fused in (weight 0.8), figures beam10_lmN / beam32_lmN
The decode runs once per evaluation utterance, not in the train step: the figures say what `decoder = "beam"` costs validate().
One line per figure and a JSON summary line."""
import argparse
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


def random_lm(order, V, seed=0, keep=(1.0, 0.5, 0.2, 0.1, 0.05)):
    """A random back-off model read from generated ARPA text: every unigram, a `keep` share of the longer n-grams of listed
    contexts, back-off weights on three contexts in four; token 0 is the blank, 1 the silence."""
    import numpy as np
    from aptai_amd.ngram import NGramLM
    rs = np.random.RandomState(seed + order)
    names = ["(blank)", "(...)"] + [f"p{i}" for i in range(2, V)]
    level = [("<s>",)] + [(w,) for w in names[1:]] + [("</s>",)]
    text = ["\\data\\"]
    for k in range(order):
        text += ["", f"\\{k + 1}-grams:"]
        for g in level:
            row = f"{-99.0 if g[-1] == '<s>' else -(0.1 + 2.9 * rs.rand()):.6f}\t" + " ".join(g)
            if k + 1 < order and g[-1] != "</s>" and rs.rand() < 0.75:
                row += f"\t{-1.5 * rs.rand():.6f}"
            text.append(row)
        if k + 1 < order:
            level = [g + (w,) for g in level if g[-1] != "</s>" for w in names[1:] + ["</s>"] if rs.rand() < keep[k + 1]]
    return NGramLM.from_arpa("\n".join(text + ["", "\\end\\", ""]), names)


def main(B=16, T=499, V=46, ldl=64, rounds=7, iters=20, lm_orders=()):
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    logits = torch.zeros(B * T, ldl)
    logits[:, :V] = torch.randn(B * T, V, generator=g) * 3
    logits = logits.to(dev)
    L_ = _lib.lib()
    stream = ops._stream()
    max_n = T + 2
    fns, outs = {}, {}
    for name, beam, log_add, nbest in (("beam10", 10, 0, 1), ("beam32", 32, 1, 32)):
        ws = torch.empty(L_.aptai_ctc_beam_search_workspace_bytes(B, T, beam, nbest), device=dev, dtype=torch.uint8)
        tok, ts = (torch.empty((B, nbest, max_n), device=dev, dtype=torch.int32) for _ in range(2))
        n_tok = torch.empty((B, nbest), device=dev, dtype=torch.int32)
        score = torch.empty((B, nbest), device=dev, dtype=torch.float64)
        n_hyp = torch.empty(B, device=dev, dtype=torch.int32)
        outs[name] = (ws, tok, ts, n_tok, score, n_hyp)

        def beam_search(beam=beam, log_add=log_add, nbest=nbest, o=outs[name]):
            _lib.call("aptai_ctc_beam_search", logits.data_ptr(), ldl, T, None, B, T, V, 0, 1, beam, 0, 50.0, log_add, 0.0, nbest, max_n,
                      o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(), stream)
        fns[name] = beam_search
        for order in lm_orders:
            w, nxt, wf, n_states, start = random_lm(order, V).device_tables(0.8, dev)
            o = tuple(torch.empty_like(x) for x in outs[name])
            outs[f"{name}_lm{order}"] = o + (w, nxt, wf)            # the tables stay alive with the buffers

            def beam_search_lm(beam=beam, log_add=log_add, nbest=nbest, o=o, w=w, nxt=nxt, wf=wf, n_states=n_states, start=start):
                _lib.call("aptai_ctc_beam_search_lm", logits.data_ptr(), ldl, T, None, B, T, V, 0, 1, beam, 0, 50.0, log_add, 0.0, nbest,
                          max_n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(),
                          w.data_ptr(), nxt.data_ptr(), wf.data_ptr(), n_states, start, stream)
            fns[f"{name}_lm{order}"] = beam_search_lm
            print(f"{name}_lm{order}: {n_states} states, tables {(w.numel() * 12 + wf.numel() * 8) / 1024:.0f} KiB")
    ids = torch.empty((B, max_n), device=dev, dtype=torch.int32)
    n = torch.empty(B, device=dev, dtype=torch.int32)
    fns["greedy"] = lambda: _lib.call("aptai_ctc_greedy_decode", logits.data_ptr(), ldl, T, None, B, T, V, 0, -1, ids.data_ptr(), None, max_n,
                                      n.data_ptr(), stream)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # every row has a best hypothesis; with an LM the floor may leave fewer than nbest of them (their ranks score -inf)
    assert all(torch.isfinite(outs[k][4][:, 0]).all() and (outs[k][5] >= 1).all() for k in outs)
    assert all(torch.isfinite(outs[k][4]).all() for k in outs if "_lm" not in k)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_time(fn, iters))
    res = {"shape": f"{B}x{T}x{V}", "device": torch.cuda.get_device_name(0)}
    for k in fns:
        med = sorted(t[k])[len(t[k]) // 2]
        print(f"{k}: {med:.1f} us per call (min {min(t[k]):.1f}, max {max(t[k]):.1f}), {med / B:.1f} us per utterance")
        res[f"{k}_us"] = round(med, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lm", type=int, action="append", default=[], metavar="ORDER",
                    help="also time aptai_ctc_beam_search_lm with a random n-gram of this order, 1..5 (repeatable)")
    main(lm_orders=tuple(ap.parse_args().lm))
