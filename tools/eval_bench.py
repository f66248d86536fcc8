#!/usr/bin/env python3
"""Validation time per utterance of train_aptai.validate with the host metrics (default) and with `device_metrics=True` (run on
the GPU box).

The synthetic corpus at batch size 1 with 10 s items (T = 499 frames), as the reference evaluates; the same model, the same
loader, one process.  A round times one validate() call of each path, host first then device, wall clock around the call ending in a
device synchronise; the two paths alternate round by round so that clocks and neighbours hit them alike.  Both paths run the same
batch-1 forward, so the difference of the two figures is the metric work plus the per-utterance transfers the host path makes.
Prints the median, minimum and maximum over the rounds in ms per utterance, the final dictionaries' largest difference, and a JSON
summary line.

    python tools/eval_bench.py [--layers 12] [--items 16] [--rounds 7] [--seconds 10]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aptai_amd import hostlogic, train_aptai as T
from aptai_amd.config import W2V2Config
from aptai_amd.wav2vec2 import Wav2Vec2Model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--layers", type=int, default=12, help="transformer layers of the random-init base backbone")
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=10.0)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU (this measurement has no CPU form)")
    w2v = W2V2Config.base(vocab_size=T.VOCAB_SIZE, num_hidden_layers=a.layers)
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(0)
        Wav2Vec2Model(w2v).save_pretrained(tmp)
        cfg = T.default_cfg(huggingface_model_id=tmp, pretrain_cfg=w2v)
        model, _, _ = T.load_model_optimizer(cfg)
    model.eval()
    ds = T.SyntheticHPRC(a.items, a.seconds, vary_length=False, seed=2, cfg=w2v)
    items = [ds[i] for i in range(len(ds))]                              # built once: no generation in the timing
    dl = torch.utils.data.DataLoader(items, batch_size=1, shuffle=False, collate_fn=hostlogic.collate_aptai)

    def run(device_metrics):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic", dl, device_metrics=device_metrics)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.items, res

    res = {}
    for dm in (False, True):                                             # warm-up: code objects, weight copies, scratch buffers
        for _ in range(2):
            _, res[dm] = run(dm)
    diff = max(abs(res[True][k] - res[False][k]) for k in res[False])
    t = {False: [], True: []}
    for _ in range(a.rounds):
        for dm in (False, True):
            t[dm].append(run(dm)[0])
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for dm, name in ((False, "host metrics  "), (True, "device metrics")):
        print(f"validate, {name}: {med[dm]:.3f} ms per utterance (min {min(t[dm]):.3f}, max {max(t[dm]):.3f}; {a.rounds} rounds x {a.items} "
              f"utterances of {a.seconds:g} s, batch 1, {a.layers} layers)")
    print(f"largest |device - host| over the {len(res[False])} result entries: {diff:.2e}")
    print(json.dumps({"host_ms_per_utt": round(med[False], 3), "device_ms_per_utt": round(med[True], 3),
                      "host_over_device": round(med[False] / med[True], 2), "items": a.items, "rounds": a.rounds,
                      "seconds": a.seconds, "layers": a.layers, "max_abs_diff": diff}))


if __name__ == "__main__":
    main()
