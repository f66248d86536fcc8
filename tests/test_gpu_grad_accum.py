"""GPU: gradient accumulation inside aptai_amd.optim.Adam (csrc/optim.hip: grad_accum_kernel) - windows of N micro-batches, the HF
Trainer's gradient_accumulation_steps.  The contract is arithmetic: one rounded fp32 add per element per micro-step in micro-step
order and one rounded fp32 multiply by (float)(1 / k) at the close, then the unchanged norm and Adam kernels.  So every comparison
with the project's plain Adam, fed the same sum-then-scale evaluated by torch on the device, is bit for bit."""
import functools
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

# tests/test_gpu_grad_clip.py: NORM_SHAPES (vector path, scalar path, one element, exactly one chunk, two chunks + odd tail), then a
# parameter whose gradient is a 4-byte-aligned slice and one that never gets a gradient
SHAPES = [(768, 768), (3072,), (46, 768), (13,), (1, 1, 128), (5, 7), (1,), (4096,), (8197,), (1001,), (300,)]
SLICE, NEVER = len(SHAPES) - 2, len(SHAPES) - 1
THIRD = torch.tensor(1 / 3, dtype=torch.float32)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in SHAPES]


def _groups(ps, **kw):
    from aptai_amd.optim import Adam
    return Adam([dict(params=ps[:4], lr=1e-3), dict(params=ps[4:], lr=3e-4)], weight_decay=0.01, **kw)


def _grads(ps, gen, absent=(), scale=1.0):
    """Freshly allocated gradients (new addresses every micro-step); None for NEVER and the indices in `absent`; SLICE's is a
    4-byte-aligned slice of a larger buffer (the scalar path)."""
    out = []
    for i, p in enumerate(ps):
        if i == NEVER or i in absent:
            out.append(None)
            continue
        gr = (torch.randn(p.shape, generator=gen) * scale).cuda()
        if i == SLICE:
            buf = torch.zeros(p.numel() + 8).cuda()
            buf[1:1 + p.numel()] = gr
            gr = buf[1:1 + p.numel()]
            assert gr.data_ptr() % 16 == 4 and gr.is_contiguous()
        out.append(gr)
    return out


def _assign(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g


def _mean(micro, factor):
    """The window's expected gradient per parameter: the present gradients added in micro-step order, times `factor`; None
    when no micro-step had one."""
    out = []
    for i in range(len(micro[0])):
        total = None
        for grads in micro:
            if grads[i] is not None:
                total = grads[i].clone() if total is None else total + grads[i]
        out.append(None if total is None else total * factor)
    return out


def _state(opt, ps):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["step"])
            for p in ps if len(opt.state[p])]


def _same_state(x, y):
    return len(x) == len(y) and all(a[3] == b[3] and all(torch.equal(s, t) for s, t in zip(a[:3], b[:3])) for a, b in zip(x, y))


def _assert_same_optimiser_state(oa, a, ob, b):
    for i, (pa, pb) in enumerate(zip(a, b)):
        assert torch.equal(pa, pb), i
        sa, sb = oa.state[pa], ob.state[pb]
        assert sa["step"] == sb["step"], (i, sa["step"], sb["step"])
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), i


# window 1: parameter 1 is missing in micro-steps 1 and 2 (its first contribution overwrites on the closing micro-step);
# window 2: parameter 2 is present in micro-step 1 only, parameter 3 in none
ABSENT = [[(1,), (1,), ()], [(3,), (2, 3), (2, 3)]]


def test_window_is_bit_exact_against_the_plain_step():
    a, b, c = _params(1), _params(1), _params(1)
    oa, ob = _groups(a, gradient_accumulation_steps=3), _groups(b)
    oc = torch.optim.Adam([dict(params=c[:4], lr=1e-3), dict(params=c[4:], lr=3e-4)], weight_decay=0.01)
    gen = torch.Generator().manual_seed(2)
    assert oa.micro_step == 0 and oa.accumulated_grad(a[0]) is None
    for w, absent in enumerate(ABSENT):
        micro = []
        for k, gone in enumerate(absent):
            grads = _grads(a, gen, gone)
            micro.append(grads)
            keep = [None if g is None else g.clone() for g in grads]
            before = _state(oa, a) if w or k else [p.detach().clone() for p in a]
            _assign(a, grads)
            oa.step()
            for p, g, kept in zip(a, grads, keep):                      # .grad is never written
                assert (p.grad is None and kept is None) or (p.grad.data_ptr() == g.data_ptr() and torch.equal(p.grad, kept))
            if k < 2:
                assert not oa.last_step_updated and oa.micro_step == k + 1
                after = _state(oa, a) if w or k else [p.detach().clone() for p in a]
                if w or k:
                    assert _same_state(before, after)                   # inside a window nothing moves
                else:
                    assert all(torch.equal(x, y) for x, y in zip(before, after))
                for i, p in enumerate(a):                                # the running sum, in micro-step order
                    part = _mean(micro, 1.0)[i]
                    got = oa.accumulated_grad(p)
                    assert (got is None and part is None) or torch.equal(got, part), (w, k, i)
        assert oa.last_step_updated and oa.micro_step == 0
        expect = _mean(micro, THIRD)
        assert expect[NEVER] is None and (w == 0 or expect[3] is None) and expect[1] is not None
        for i, p in enumerate(a):
            got = oa.accumulated_grad(p)
            assert (got is None and expect[i] is None) or (got.shape == p.shape and torch.equal(got, expect[i])), (w, i)
        _assign(b, expect)
        ob.step()
        _assign(c, expect)
        oc.step()
        _assert_same_optimiser_state(oa, a, ob, b)                      # the second window would show a stale accumulator
    assert oa.state[a[3]]["step"] == 1 and oa.state[a[0]]["step"] == 2 and oa.state[a[NEVER]]["step"] == 0
    # and the update rule itself against torch, at the bounds of test_gpu_optim.test_matches_torch_adam
    for pa, pc in zip(a, c):
        assert (pa - pc).abs().max().item() <= 1e-6 * pc.abs().max().item() + 1e-7
        if len(oc.state[pc]):
            assert (oa.state[pa]["exp_avg"] - oc.state[pc]["exp_avg"]).abs().max().item() <= 1e-6
            assert (oa.state[pa]["exp_avg_sq"] - oc.state[pc]["exp_avg_sq"]).abs().max().item() <= 1e-6


def test_window_with_clipping_is_the_clipped_step_on_the_mean():
    """Gradients of window 1 are N(0, 1), of window 2 four times that.  The norm of the mean of three is about sqrt(elements / 3):
    measured with max_grad_norm = inf first, then `c` sits between the two windows' norms so that one clips and one does not."""
    def run(c):
        a, b = _params(1), _params(1)
        oa, ob = _groups(a, gradient_accumulation_steps=3, max_grad_norm=c), _groups(b, max_grad_norm=c)
        gen = torch.Generator().manual_seed(4)
        out = []
        for w, absent in enumerate(ABSENT):
            micro = [_grads(a, gen, gone, scale=1.0 if w == 0 else 4.0) for gone in absent]
            for grads in micro:
                _assign(a, grads)
                oa.step()
            expect = _mean(micro, THIRD)
            _assign(b, expect)
            ob.step()
            _assert_same_optimiser_state(oa, a, ob, b)
            assert torch.equal(oa._clip_result, ob._clip_result)
            ref = math.sqrt(sum(float((g.double() ** 2).sum()) for g in expect if g is not None))
            norm = float(oa.last_grad_norm)
            print(f"window {w}: norm {norm!r} float64 {ref!r} rel {abs(norm - ref) / ref:.3e} coef {float(oa.last_clip_coef)!r}")
            assert abs(norm - ref) <= 2e-6 * ref
            out.append((norm, float(oa.last_clip_coef)))
        return out
    (n0, _), (n1, _) = run(float("inf"))
    assert n0 < n1
    (_, c0), (_, c1) = run(0.5 * (n0 + n1))
    assert c0 == 1.0 and c1 < 1.0, (c0, c1)                             # one window is not clipped, one is


def test_off_means_off(monkeypatch):
    """N = 1 launches exactly what the optimiser launched before the option existed and owns no accumulator; N = 2 launches the
    accumulate kernel alone inside a window and today's launches behind it at the close."""
    from aptai_amd import _lib
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    for n, clip in ((1, None), (2, None), (2, 1.0)):
        ps = _params(5)
        opt = _groups(ps, gradient_accumulation_steps=n, max_grad_norm=clip)
        gen = torch.Generator().manual_seed(6)
        per_step = []
        for step in range(4):
            grads = _grads(ps, gen)
            del calls[:]
            _assign(ps, grads)
            opt.step()
            per_step.append(list(calls))
        if n == 1:
            assert per_step == [["aptai_adam_multi"] * 2] * 4, per_step                     # 2 groups x 4 steps
            assert all(opt.accumulated_grad(p) is None for p in ps) and opt._accum is None
            assert opt.last_step_updated and opt.micro_step == 0
        else:
            tail = ["aptai_adam_multi"] * 2 if clip is None else ["aptai_grad_sqnorm_multi"] + ["aptai_adam_multi_scaled"] * 2
            assert per_step == [["aptai_grad_accum_multi"], ["aptai_grad_accum_multi"] + tail] * 2, per_step


def test_flush_closes_a_short_window():
    from aptai_amd import _lib
    a, b = _params(1), _params(1)
    oa, ob = _groups(a, gradient_accumulation_steps=3), _groups(b)
    gen = torch.Generator().manual_seed(8)
    micro = [_grads(a, gen, (1,)), _grads(a, gen)]
    for grads in micro:
        _assign(a, grads)
        oa.step()
    assert oa.micro_step == 2 and not oa.last_step_updated
    with pytest.raises(RuntimeError):
        oa.gradient_accumulation_steps = 2                               # not inside an open window
    assert oa.flush() is True and oa.last_step_updated and oa.micro_step == 0
    expect = _mean(micro, 0.5)                                           # (g1 + g2) * 0.5
    _assign(b, expect)
    ob.step()
    _assert_same_optimiser_state(oa, a, ob, b)
    calls = []
    orig = _lib.call
    _lib.call = lambda name, *args: (calls.append(name), orig(name, *args))[1]
    try:
        assert oa.flush() is False and not oa.last_step_updated
    finally:
        _lib.call = orig
    assert calls == []
    oa.gradient_accumulation_steps = 3                                   # allowed again
    # the next window is clean: a full one of three, parameter 2 in its first micro-step only
    micro = [_grads(a, gen), _grads(a, gen, (2,)), _grads(a, gen, (2,))]
    for grads in micro:
        _assign(a, grads)
        oa.step()
    _assign(b, _mean(micro, THIRD))
    ob.step()
    _assert_same_optimiser_state(oa, a, ob, b)
    # a window of one micro-step flushed: the mean is the gradient itself
    grads = _grads(a, gen)
    _assign(a, grads)
    oa.step()
    assert oa.flush() is True
    _assign(b, grads)
    ob.step()
    _assert_same_optimiser_state(oa, a, ob, b)


def test_no_allocation_after_the_first_window():
    a = _params(1)
    oa = _groups(a, gradient_accumulation_steps=2, max_grad_norm=1.0)
    gen = torch.Generator().manual_seed(9)
    windows = [[_grads(a, gen), _grads(a, gen, (1,))] for _ in range(2)]
    for grads in windows[0]:
        _assign(a, grads)
        oa.step()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for grads in windows[1]:
        _assign(a, grads)
        oa.step()
    assert torch.cuda.memory_allocated() == before
    assert oa.last_step_updated


# ------------------------------------------------------------------------------------------------------------------ model level
def _tiny(layerdrop=0.0):
    """The model of tests/test_gpu_grad_clip.py::_tiny: 3 layers, regularisers 0."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    cfg = W2V2Config.base(num_hidden_layers=3, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=layerdrop, apply_spec_augment=False, vocab_size=46)
    return cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)


def _reference_update(model, init, windows, lr, wd):
    """Plain Adam on clones of the initial parameters, stepping once per window on the expected means; returns name -> (parameter,
    step count)."""
    from aptai_amd.optim import Adam
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    ref = [torch.nn.Parameter(init[n].clone()) for n in names]
    opt = Adam(ref, lr=lr, weight_decay=wd)
    for micro in windows:
        _assign(ref, _mean([[m[n] for n in names] for m in micro], 0.5))
        opt.step()
    return {n: (p.detach(), opt.state[p].get("step", 0)) for n, p in zip(names, ref)}


def _copies_are_fresh(model, cfg):
    """The check of test_gpu_optim.test_publishes_fresh_bf16_copies_to_the_model."""
    plan, l0, H = model.wav2vec2._layer_plan(), model.wav2vec2.encoder.layers[0], cfg.hidden_size
    e = plan.entries[0]
    assert torch.equal(e.w1, l0.feed_forward.intermediate_dense.weight.detach().to(torch.bfloat16))
    assert torch.equal(e.wqkv[H:2 * H], l0.attention.k_proj.weight.detach().to(torch.bfloat16))
    assert torch.equal(e.bqkv[0:H], l0.attention.q_proj.bias.detach())


@pytest.mark.parametrize("mode", ["eager", "bucketed"])
def test_windows_through_the_eager_loop_and_the_bucketed_runner(mode):
    """Two batch lengths fed alternately, N = 2: in the bucketed runner a window spans the static gradient buffers of two runners."""
    from aptai_amd.graphed import BucketedGraphedStep
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_aptai import _build
    cfg, sd = _tiny()
    batches = [synth.synth_aptai_batch(cfg, 2, s, seed=3 + i) for i, s in enumerate((16000, 24000))]
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    init = {n: p.detach().clone() for n, p in named}
    opt = Adam([p for _, p in named], lr=1e-4, weight_decay=0.01, gradient_accumulation_steps=2).publish_to(model)
    plan = model.wav2vec2._layer_plan()
    runner = BucketedGraphedStep(model, opt, bucket_samples=[16000, 24000]) if mode == "bucketed" else None
    windows = []
    try:
        for w in range(2):
            micro = []
            for k in range(2):
                b = batches[k]
                if runner is None:
                    opt.zero_grad(set_to_none=True)
                    model(0, **{n: v.cuda() for n, v in b.items()})["loss"].backward()
                    opt.step()
                else:
                    runner.step(b)
                micro.append({n: None if p.grad is None else p.grad.detach().clone() for n, p in named})
                if k == 0:
                    assert not opt.last_step_updated
                    start = init if w == 0 else after
                    assert all(torch.equal(p, start[n]) for n, p in named)                  # inside a window nothing moves,
                    if w:
                        _copies_are_fresh(model, cfg)                                       # the published copies included
                else:
                    assert opt.last_step_updated and getattr(plan, "optimizer_synced", False)
                    _copies_are_fresh(model, cfg)
            after = {n: p.detach().clone() for n, p in named}
            windows.append(micro)
        if runner is not None:
            assert len(runner.runners) == 2
    finally:
        if runner is not None:
            runner.close()
    ref = _reference_update(model, init, windows, 1e-4, 0.01)
    for n, p in named:
        assert torch.equal(p, ref[n][0]), n
        assert opt.state[p].get("step", 0) == ref[n][1], n
    assert max(st for _, st in ref.values()) == 2
    assert not any(torch.equal(after[n], init[n]) for n, _ in named if n.endswith("intermediate_dense.weight"))


@functools.lru_cache(maxsize=None)
def _layerdrop_run(overlap):
    """Three windows of two micro-steps through GraphedAPTAIStep with LayerDrop 0.3.  Generator seed 12 keeps the layers
    [1,0,1] [1,1,0] | [1,0,1] [1,0,1] | [1,1,1] [0,1,1]: layers 1 and 2 are dropped in one micro-step of window 1, layer 1 in both of
    window 2, layer 0 in one of window 3.  (The caller has set APTAI_ADAM_OVERLAP to `overlap`.)"""
    from aptai_amd.graphed import GraphedAPTAIStep
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_aptai import _build
    cfg, sd = _tiny(layerdrop=0.3)
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 16000, seed=3).items()}
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    init = {n: p.detach().clone() for n, p in named}
    opt = Adam([p for _, p in named], lr=1e-4, weight_decay=0.01, gradient_accumulation_steps=2).publish_to(model)
    windows = []
    with GraphedAPTAIStep(model, opt, batch) as runner:
        assert runner.adam_overlap == (overlap == "1")
        model.wav2vec2._layerdrop_gen = torch.Generator().manual_seed(12)
        for w in range(3):
            micro = []
            for k in range(2):
                runner.step()
                micro.append({n: None if p.grad is None else p.grad.detach().clone() for n, p in named})
            windows.append(micro)
    torch.cuda.synchronize()
    final = {n: (p.detach().clone(), opt.state[p]["step"], opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
             for n, p in named if len(opt.state[p])}
    return model, init, windows, final


def test_layerdrop_inside_a_window(monkeypatch):
    monkeypatch.setenv("APTAI_ADAM_OVERLAP", "0")
    model, init, windows, final = _layerdrop_run("0")
    probe = [[n for n in final if n.endswith(f"layers.{i}.feed_forward.intermediate_dense.weight")][0] for i in range(3)]
    present = [[sum(m[n] is not None for m in micro) for n in probe] for micro in windows]
    print("micro-steps with a gradient per window and layer:", present)
    assert any(1 in row for row in present) and any(0 in row for row in present)          # dropped in one micro-step; in both
    ref = _reference_update(model, init, windows, 1e-4, 0.01)
    for n, (p, step, _, _) in final.items():
        assert torch.equal(p, ref[n][0]), n
        assert step == ref[n][1] == sum(any(m[n] is not None for m in micro) for micro in windows), n
    assert {final[n][1] for n in probe} != {3}                                              # some layer missed a whole window


def test_overlap_knob_changes_no_bit(monkeypatch):
    """The protocol of test_gpu_grad_clip.test_overlap_experiment_with_clipping_changes_no_bit: with N > 1 every row goes to
    finish(), launch_early() finds nothing to do."""
    rec = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("APTAI_ADAM_OVERLAP", flag)
        rec[flag] = _layerdrop_run(flag)[3]
    for n, (p, step, m, v) in rec["0"].items():
        p1, step1, m1, v1 = rec["1"][n]
        assert torch.equal(p, p1) and step == step1 and torch.equal(m, m1) and torch.equal(v, v1), n


@pytest.mark.parametrize("accum,max_grad_norm", [(2, None), (2, 1.0), (None, None)])
def test_phoneme_recognizer_loop_counts_the_updates(tmp_path, accum, max_grad_norm):
    from aptai_amd import hostlogic, train_phoneme_recognizer as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    vocab = T.default_vocab()
    w2v = W2V2Config.base(num_hidden_layers=2, layerdrop=0.0)
    torch.manual_seed(0)
    d = tmp_path / "w2v"
    Wav2Vec2Model(w2v).save_pretrained(str(d))
    cfg = T.default_cfg(num_epochs=1, batch_size=2, samples_per_epoch=6, learning_rate=2e-5, huggingface_model_id=str(d),
                        pretrain_cfg=w2v, num_warmup_epochs=2)
    if accum is not None:
        cfg.gradient_accumulation_steps = accum
    if max_grad_norm is not None:
        cfg.max_grad_norm = max_grad_norm
    model, opt, sched = T.load_model_optimizer(cfg, vocab)
    assert opt.gradient_accumulation_steps == (accum or 1)
    tr = torch.utils.data.DataLoader(T.SyntheticCommonPhone(6, 1.0, len(vocab), seed=1), batch_size=2, drop_last=True,
                                     collate_fn=hostlogic.collate_pr)
    va = torch.utils.data.DataLoader(T.SyntheticCommonPhone(2, 1.0, len(vocab), seed=2), batch_size=1, collate_fn=hostlogic.collate_pr)
    random.seed(7)
    hist = T.train(cfg, model, opt, sched, vocab, tr, va, tmp_path / "best-model-ckpt", tmp_path / "last-model-ckpt",
                   tmp_path / "model-ckpts", log=lambda s: None)
    assert len(hist) == 1 and hist[0]["trained_batches"] == 3
    if accum is None:
        assert "optimizer_updates" not in hist[0]
        return
    assert hist[0]["optimizer_updates"] == 2 and opt.micro_step == 0                     # one full window and a flushed remainder
    steps = {int(opt.state[p]["step"]) for g in opt.param_groups for p in g["params"] if len(opt.state[p])}      # (tensors once saved)
    assert steps - {0} == {2}, steps
    if max_grad_norm is not None:
        assert math.isfinite(hist[0]["mean_grad_norm"]) and hist[0]["mean_grad_norm"] > 0
        assert 0 <= hist[0]["clipped_steps"] <= hist[0]["optimizer_updates"]
