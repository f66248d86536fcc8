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
figure and a JSON summary line.

`--wide` measures the wide kernel instead (aptai_ctc_viterbi_wide: long recordings against whole transcripts): 16 x 499 with 255
labels beside aptai_ctc_viterbi on the same problem (results compared first: they must be equal), 1 and 4 x 15 000 frames with 3 500
labels alone, and the eval-mode encoder forwards of the 38 windows of 499 frames such a recording is cut into."""
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


def _problem(B, T, V, L, dev="cuda"):
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(B * T, V, generator=g) * 3).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32).to(dev)
    return (logits, targets, torch.full((B,), T, dtype=torch.int32, device=dev), torch.full((B,), L, dtype=torch.int32, device=dev),
            torch.empty((B, T), device=dev, dtype=torch.int32), torch.empty((B, L, 2), device=dev, dtype=torch.int32),
            torch.empty(B, device=dev, dtype=torch.float32), torch.empty((B, L), device=dev, dtype=torch.float32))


def wide_case(name, B, T, V, L, res, narrow=False, rounds=7, iters=20):
    """aptai_ctc_viterbi_wide (lz pre-pass + one workgroup per recording + spans: 3 launches), beside aptai_ctc_viterbi where the
    shape fits it, the two alternating round by round.  Prints the time per call and per frame and the workspace of each."""
    logits, targets, in_lens, t_lens, ft, spans, score, tsc = _problem(B, T, V, L)
    L_ = _lib.lib()
    stream = ops._stream()
    names = ["viterbi_wide"] + (["viterbi"] if narrow else [])
    ws = {k: torch.empty(getattr(L_, f"aptai_ctc_{k}_workspace_bytes")(B, T, L), device="cuda", dtype=torch.uint8) for k in names}
    out = {}

    def make(k):
        def fn():
            _lib.call(f"aptai_ctc_{k}", logits.data_ptr(), V, T, targets.data_ptr(), L, in_lens.data_ptr(), t_lens.data_ptr(), None, B, T, V,
                      0, 0, ws[k].data_ptr(), ft.data_ptr(), spans.data_ptr(), score.data_ptr(), tsc.data_ptr(), stream)
        return fn
    fns = {k: make(k) for k in names}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        assert torch.isfinite(score).all()
        out[k] = (ft.clone(), spans.clone(), score.clone(), tsc.clone())
    if narrow:
        assert all(torch.equal(a, b) for a, b in zip(out["viterbi_wide"], out["viterbi"])), "wide and narrow results differ"
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_time(fn, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for k in fns:
        print(f"{name} aptai_ctc_{k}: {med[k]:.1f} us per call (min {min(t[k]):.1f}, max {max(t[k]):.1f}), {med[k] * 1e3 / T:.0f} ns per frame, "
              f"workspace {ws[k].numel() / 2 ** 20:.1f} MiB")
        res[f"{name}_{k}_us"], res[f"{name}_{k}_ws_mib"] = round(med[k], 1), round(ws[k].numel() / 2 ** 20, 1)
    if narrow:
        res[f"{name}_wide_over_narrow"] = round(med["viterbi_wide"] / med["viterbi"], 2)
        print(f"{name} wide / narrow = {res[f'{name}_wide_over_narrow']:.2f} (same bits; the wide kernel pays one barrier per frame)")


def encoder_windows(res, n_windows=38, per_forward=16, rounds=3):
    """What the windows of a 15 000-frame recording cost in front of the alignment: `n_windows` 10 s windows through the eval-mode,
    batch-invariant forward of a wav2vec2-base recogniser with random weights, `per_forward` at a time (Wav2Vec2_PR._long's loop)."""
    import tempfile

    from safetensors.torch import save_file

    from aptai_amd.config import W2V2Config
    from aptai_amd.w2v2_pr import Wav2Vec2_PR
    from oracle import synth
    cfg = W2V2Config.base(vocab_size=46)
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "config.json"), "w") as f:
            json.dump(cfg.to_dict(), f)
        save_file({k[len("wav2vec2."):]: v.contiguous() for k, v in sd.items() if k.startswith("wav2vec2.")},
                  os.path.join(tmp, "model.safetensors"))
        model = Wav2Vec2_PR(cfg, None, tmp, {f"p{i}": i for i in range(46)})
    model.load_state_dict(sd)
    model = model.cuda().eval()
    model.batch_invariant = True
    samples = 320 * 498 + 400                                            # 499 frames
    groups = [min(per_forward, n_windows - a) for a in range(0, n_windows, per_forward)]
    audio = {n: torch.randn(n, samples, generator=torch.Generator().manual_seed(n)).cuda() for n in set(groups)}
    lens = {n: torch.full((n,), samples, dtype=torch.long).cuda() for n in set(groups)}

    def run():
        with torch.no_grad():
            for n in groups:
                model._logits_eval(audio[n], lens[n])
    run()
    torch.cuda.synchronize()
    ms = sorted(_time(run, 2) / 1e3 for _ in range(rounds))[rounds // 2]
    print(f"encoder: {n_windows} windows of 499 frames, {per_forward} per forward (wav2vec2-base, eval, batch-invariant): {ms:.1f} ms")
    res["encoder_38_windows_ms"] = round(ms, 1)


if __name__ == "__main__":
    res = {}
    if "--wide" in sys.argv[1:]:                                          # profiles/ctc_viterbi_wide.txt
        wide_case("16x499x46_L255", 16, 499, 46, 255, res, narrow=True)
        wide_case("1x15000x46_L3500", 1, 15000, 46, 3500, res, iters=5)
        wide_case("4x15000x46_L3500", 4, 15000, 46, 3500, res, iters=5)
        encoder_windows(res)
    else:
        case("16x499x46_L60", 16, 499, 46, 60, res)
        case("16x1499x46_L200", 16, 1499, 46, 200, res)
    print(json.dumps(res))
