"""Step time of the Force_APTAI train step at a given `max_phn_seq_len` on bench.py's force workload (same model, same synthetic
batch, same hipGraph runner), with the blank bias calibrated so that the decode yields transcripts of --lo..--hi phonemes.
Information only: bench.py itself measures the default cap.

    python tools/force_long_cap_step.py --cap 255 --lo 100 --hi 150 --steps 20 --warmup 5
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    import bench
    from aptai_amd.force_aptai import Force_APTAI
    from aptai_amd.graphed import GraphedForceStep
    from aptai_amd.optim import Adam
    from aptai_amd.w2v2_pr import Wav2Vec2_PR
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cap", type=int, default=255)
    ap.add_argument("--lo", type=int, default=100)
    ap.add_argument("--hi", type=int, default=150)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    device = "cuda:0"
    args = argparse.Namespace(model="base", no_regularisers=False)
    cfg = bench._cfg(args, 40, ctc_loss_reduction="mean", ctc_zero_infinity=True)
    vocab = bench._vocab40()
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:                 # bench.build_force with the cap passed on
        mdir = os.path.join(tmp, "w2v2")
        Wav2Vec2Model(cfg).save_pretrained(mdir)
        pr = Wav2Vec2_PR(cfg, None, mdir, vocab)
        ck = os.path.join(tmp, "pr", "best-model-ckpt")
        os.makedirs(ck)
        torch.save(pr.state_dict(), os.path.join(ck, "pytorch_model.bin"))
        with open(os.path.join(ck, "model_cfg.pkl"), "wb") as f:
            pickle.dump({"pretrain_cfg": cfg.to_dict(), "cache_dir": None, "huggingface_model_id": mdir}, f)
        model = Force_APTAI(os.path.join(tmp, "pr"), device, vocab, max_phn_seq_len=a.cap).to(device)
    batch = bench.synth_batch(cfg, a.batch, int(a.seconds * 16000), 9, 0, device, n_phn=40)
    batch["phoneme_labels"] = bench.synth_ctc_labels(a.batch, 40, 0, device)
    bias, counts = bench.calibrate_blank_bias(model, batch, lo=a.lo, hi=a.hi)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = Adam(params, lr=1e-5, betas=(0.9, 0.999), eps=1e-8)
    runner = GraphedForceStep(model, opt, batch)
    for _ in range(a.warmup):
        runner.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = runner.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    runner.close()
    print(json.dumps({"workload": "force", "max_phn_seq_len": a.cap, "batch": a.batch, "seconds": a.seconds,
                      "decoded_phonemes": [min(counts), max(counts)], "blank_bias": round(bias, 3),
                      "step_ms": round(dt / a.steps * 1e3, 3), "steps": a.steps, "warmup": a.warmup,
                      "loss": float(out["loss"].detach())}))


if __name__ == "__main__":
    main()
