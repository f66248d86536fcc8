"""GPU: global-norm gradient clipping fused into aptai_amd.optim.Adam (csrc/optim.hip: grad_sqnorm_kernel, grad_norm_final_kernel,
adam_multi_kernel<true>, scale_multi_kernel) - `torch.nn.utils.clip_grad_norm_(params, max_norm)` before the `optimizer.step()` of
train/train_*.py.  The norm against float64, the update rule against torch, the fused step against clip-then-step bit for bit, the
default path launch for launch, non-finite norms, the graphed runner, the overlap experiment and the loops' logs."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(768, 768), (3072,), (46, 768), (13,), (1, 1, 128), (5, 7)]             # tests/test_gpu_optim.py
NORM_SHAPES = SHAPES + [(1,), (4096,), (8197,)]                                     # + one element, exactly one chunk, two chunks + odd tail


def _params(seed, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in shapes]


def _norm_setup(max_norm, scale=1.0, zero=False):
    """Two parameter groups over NORM_SHAPES + a 4-byte-aligned slice gradient + a parameter without a gradient; returns
    (optimiser, parameters, float64 reference norm)."""
    from aptai_amd.optim import Adam
    ps = _params(11, NORM_SHAPES + [(1001,), (300,)])
    g = torch.Generator().manual_seed(12)
    sq = 0.0
    buf = None
    for i, p in enumerate(ps):
        if i == len(ps) - 1:
            p.grad = None                                   # LayerDrop: contributes nothing
            continue
        gr = torch.zeros(p.shape) if zero else torch.randn(p.shape, generator=g) * scale
        if i == len(ps) - 2:                                # a slice of a larger buffer: 4-byte aligned only -> the scalar path
            buf = torch.zeros(p.numel() + 8).cuda()
            buf[1:1 + p.numel()] = gr.cuda()
            p.grad = buf[1:1 + p.numel()]
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = gr.cuda()
        sq += float((gr.double() ** 2).sum())
    opt = Adam([dict(params=ps[:4], lr=1e-3), dict(params=ps[4:], lr=3e-4)], max_grad_norm=max_norm)
    return opt, ps, math.sqrt(sq)


def _words(opt):
    return opt._clip_result.clone()


@pytest.mark.parametrize("scale,max_norm", [(1.0, 100.0), (1e-3, 1.0), (30.0, 0.5)])
def test_norm_and_coefficient_against_float64(scale, max_norm):
    """fp32 only inside a 4096-element chunk (about 24 sequential roundings: 1.4e-6 on the sum, 0.7e-6 on its root), double across
    chunks: 2e-6 relative against float64.  (torch's own fp32 norm is 4-5e-6 away on these shapes: not the reference.)"""
    opt, ps, ref = _norm_setup(max_norm, scale)
    opt.step()
    got = _words(opt)
    norm, coef, elems = (float(x) for x in got.double().cpu())
    ref_coef = min(1.0, max_norm / (ref + 1e-6))
    print(f"norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.3e}; coef {coef!r} ref {ref_coef!r} rel {abs(coef - ref_coef) / ref_coef:.3e}")
    assert abs(norm - ref) <= 2e-6 * ref
    assert abs(coef - ref_coef) <= 2e-6 * ref_coef
    assert elems == sum(p.numel() for p in ps[:-1])
    assert float(opt.last_grad_norm) == norm and float(opt.last_clip_coef) == coef
    assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda
    # the same gradients again: the same bits in all three words
    opt.step()
    assert torch.equal(_words(opt), got)
    # nothing was written to .grad, and the parameter without a gradient got no step count
    assert int(opt.state[ps[0]]["step"]) == 2 and int(opt.state[ps[-1]]["step"]) == 0


def test_zero_gradient_gives_norm_zero_and_coefficient_one():
    opt, ps, ref = _norm_setup(1.0, zero=True)
    before = [p.detach().clone() for p in ps]
    opt.step()
    assert ref == 0.0 and float(opt.last_grad_norm) == 0.0 and float(opt.last_clip_coef) == 1.0
    assert all(torch.equal(a, p) for a, p in zip(before, ps))


def _clip_grads(step, shapes_like, gen):
    """Gradients of one step of tests 2 / 3: randn * 0.5 on even steps (norm about 398: not clipped at 800), * 2 on odd steps (about
    1595: coefficient about 0.5); parameter 1 has no gradient on steps 1 and 2."""
    out = []
    for i, p in enumerate(shapes_like):
        if i == 1 and step in (1, 2):
            out.append(None)
            continue
        out.append(torch.randn(p.shape, generator=gen).cuda() * (0.5 if step % 2 == 0 else 2.0))
    return out


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipped_update_matches_torch_adam(wd):
    """The torch side scales its gradient copies by OUR coefficient (pinned by the norm test), then torch.optim.Adam steps: this
    isolates the application of the scale, so the bounds are those of test_gpu_optim.test_matches_torch_adam."""
    from aptai_amd.optim import Adam
    a, b = _params(1), _params(1)
    oa = Adam(a, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, max_grad_norm=800.0)
    ob = torch.optim.Adam(b, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    g = torch.Generator().manual_seed(2)
    coefs = []
    for step in range(6):
        grads = _clip_grads(step, a, g)
        for pa, gr in zip(a, grads):
            pa.grad = None if gr is None else gr.clone()
        oa.step()
        coef = oa.last_clip_coef.clone()
        coefs.append(float(coef))
        for pb, gr in zip(b, grads):
            pb.grad = None if gr is None else gr * coef
        ob.step()
    print("coefficients", coefs)
    assert all(c == 1.0 for c in coefs[0::2]) and all(0.45 < c < 0.55 for c in coefs[1::2]), coefs      # both cases occur
    for pa, pb in zip(a, b):
        assert (pa - pb).abs().max().item() <= 1e-6 * pb.abs().max().item() + 1e-7
    for pa, pb in zip(a, b):
        sa, sb = oa.state[pa], ob.state[pb]
        assert int(sa["step"]) == int(sb["step"].item())
        assert (sa["exp_avg"] - sb["exp_avg"]).abs().max().item() <= 1e-6
        assert (sa["exp_avg_sq"] - sb["exp_avg_sq"]).abs().max().item() <= 1e-6


def test_fused_step_equals_clip_then_step_bit_for_bit():
    from aptai_amd.optim import Adam, clip_grad_norm_
    a, b = _params(1), _params(1)
    oa = Adam(a, lr=3e-3, weight_decay=0.01, max_grad_norm=800.0)
    ob = Adam(b, lr=3e-3, weight_decay=0.01)
    g = torch.Generator().manual_seed(2)
    for step in range(4):
        grads = _clip_grads(step, a, g)
        for pa, pb, gr in zip(a, b, grads):
            pa.grad = None if gr is None else gr.clone()
            pb.grad = None if gr is None else gr.clone()
        oa.step()
        total = clip_grad_norm_(b, 800.0)
        ob.step()
        coef = oa.last_clip_coef
        assert torch.equal(total, oa.last_grad_norm) and total.dim() == 0
        for pa, pb, gr in zip(a, b, grads):
            if gr is None:
                assert pa.grad is None and pb.grad is None
                continue
            assert torch.equal(pa.grad, gr)                  # fused: .grad keeps the unclipped gradient
            assert torch.equal(pb.grad, gr * coef)           # two-pass: g * coef, one rounded multiply
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)
        sa, sb = oa.state[pa], ob.state[pb]
        assert sa["step"] == sb["step"] and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


def test_off_means_off(monkeypatch):
    """max_grad_norm=None launches exactly what the optimiser launched before the option existed; inf measures and changes no bit."""
    from aptai_amd import _lib
    from aptai_amd.optim import Adam
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    finals = {}
    for mode in (None, float("inf")):
        ps = _params(5)
        opt = Adam([dict(params=ps[:2]), dict(params=ps[2:4], lr=1e-2), dict(params=ps[4:])], lr=3e-3, weight_decay=0.01, max_grad_norm=mode)
        g = torch.Generator().manual_seed(6)
        del calls[:]
        for step in range(3):
            for i, p in enumerate(ps):
                p.grad = None if i >= 4 else torch.randn(p.shape, generator=g).cuda()     # the third group never has a gradient
            opt.step()
        if mode is None:
            assert calls == ["aptai_adam_multi"] * 6, calls                                # 2 groups with gradients x 3 steps
            assert opt.last_grad_norm is None
        else:
            assert calls == ["aptai_grad_sqnorm_multi", "aptai_adam_multi_scaled", "aptai_adam_multi_scaled"] * 3, calls
            n = float(opt.last_grad_norm)
            assert math.isfinite(n) and n > 0 and float(opt.last_clip_coef) == 1.0
        finals[mode] = ([p.detach().clone() for p in ps], [opt.state[p]["exp_avg_sq"].clone() for p in ps[:4]])
    for x, y in zip(finals[None][0] + finals[None][1], finals[float("inf")][0] + finals[float("inf")][1]):
        assert torch.equal(x, y)


def test_non_finite_norms():
    from aptai_amd.optim import Adam, clip_grad_norm_
    for bad in (float("inf"), float("nan")):
        ps = _params(7)
        for p in ps:
            p.grad = torch.randn(p.shape).cuda()
        ps[2].grad[17, 5] = bad
        opt = Adam(ps, lr=1e-3, max_grad_norm=1.0)
        opt.step()
        norm, coef = float(opt.last_grad_norm), float(opt.last_clip_coef)
        if math.isinf(bad):
            assert norm == float("inf") and coef == 0.0
        else:
            assert math.isnan(norm) and math.isnan(coef)
        keep = [p.grad.clone() for p in ps]
        with pytest.raises(RuntimeError, match="non-finite"):
            clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)
        # raised before anything was scaled: the same bits (torch.equal would call the NaN element unequal to itself)
        assert all(torch.equal(k.view(torch.int32), p.grad.view(torch.int32)) for k, p in zip(keep, ps))
        total = clip_grad_norm_(ps, 1.0)                                                   # torch's default: scale anyway
        assert float(total) == norm or (math.isnan(norm) and math.isnan(float(total)))


def test_groups_on_two_devices_are_refused():
    from aptai_amd import _lib
    from aptai_amd.optim import Adam
    if torch.cuda.device_count() < 2:
        a, b = _params(8, [(4,)])[0], torch.nn.Parameter(torch.randn(4))
        b.grad = torch.randn(4)
        a.grad = torch.randn(4).cuda()
        with pytest.raises(_lib.AptaiHipError):                                            # a CPU group with a gradient: no fallback
            Adam([dict(params=[a]), dict(params=[b])], max_grad_norm=1.0).step()
        return
    a = torch.nn.Parameter(torch.randn(4, device="cuda:0"))
    b = torch.nn.Parameter(torch.randn(4, device="cuda:1"))
    a.grad, b.grad = torch.randn(4, device="cuda:0"), torch.randn(4, device="cuda:1")
    with pytest.raises(_lib.AptaiHipError, match="one device"):
        Adam([dict(params=[a]), dict(params=[b])], max_grad_norm=1.0).step()


# ------------------------------------------------------------------------------------------------------------------ model level
def _tiny():
    """The model of tests/test_gpu_graphed.py::test_graphed_step_matches_eager: 3 layers, regularisers 0, 2 x 1 s."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    cfg = W2V2Config.base(num_hidden_layers=3, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 16000, seed=3).items()}
    return cfg, sd, batch


def test_model_norm_and_graphed_runner_match_the_eager_loop():
    from aptai_amd.graphed import GraphedAPTAIStep
    from aptai_amd.optim import Adam, ClipMonitor
    from test_gpu_aptai import _build
    cfg, sd, batch = _tiny()
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = Adam(params, lr=1e-4, max_grad_norm=float("inf"))
    model(0, **batch)["loss"].backward()
    opt.step()
    ref = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in params if p.grad is not None))
    norm0 = float(opt.last_grad_norm)
    print(f"model norm {norm0!r} ref {ref!r} rel {abs(norm0 - ref) / ref:.3e}")
    assert abs(norm0 - ref) <= 2e-6 * ref
    del model, opt, params

    losses, finals, clipped = {}, {}, {}
    for mode in ("eager", "graph"):
        model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
        model.train()
        opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, max_grad_norm=0.5 * ref)
        mon = ClipMonitor(opt)
        ls = []
        if mode == "eager":
            for _ in range(4):
                opt.zero_grad(set_to_none=True)
                out = model(0, **batch)
                out["loss"].backward()
                opt.step()
                mon.update()
                ls.append(out["loss"].item())
        else:
            runner = GraphedAPTAIStep(model, opt, batch)
            for _ in range(4):
                ls.append(runner.step()["loss"].item())
                mon.update()
            runner.close()
        log = mon.epoch_log()
        print(mode, ls, log)
        losses[mode], clipped[mode] = ls, log["clipped_steps"]
        assert math.isfinite(log["mean_grad_norm"]) and log["mean_grad_norm"] > 0
        finals[mode] = {n: p.detach().float().cpu().clone() for n, p in model.named_parameters()}
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 2e-3 * abs(a), (losses["eager"], losses["graph"])
    for n in finals["eager"]:
        d = (finals["eager"][n] - finals["graph"][n]).abs().max().item()
        assert d <= 2e-4, (n, d)
    assert clipped == {"eager": 4, "graph": 4}, clipped


def test_overlap_experiment_with_clipping_changes_no_bit(monkeypatch):
    """The protocol of test_gpu_graphed.test_optimiser_under_the_backward_pass_changes_no_bit with max_grad_norm set: every row goes to
    finish() (no global norm before the last gradient), launch_early() finds nothing, the step is the one-launch step."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedAPTAIStep
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=3, layerdrop=0.3, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 24000, seed=3).items()}
    rec = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("APTAI_ADAM_OVERLAP", flag)
        model = _build(cfg, sd, tv_drop=0.1, phn_drop=0.1)
        model.train()
        model.wav2vec2._layerdrop_gen = torch.Generator().manual_seed(5)
        opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0).publish_to(model)
        with GraphedAPTAIStep(model, opt, batch) as runner:
            assert runner.adam_overlap == (flag == "1")
            runner._salt_gen.seed(7)
            losses = [runner.step()["loss"].item() for _ in range(5)]
        torch.cuda.synchronize()
        rec[flag] = (losses, {n: p.detach().clone() for n, p in model.named_parameters()},
                     {n: (opt.state[p]["step"], opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                      for n, p in model.named_parameters() if p in opt.state and len(opt.state[p])},
                     opt._clip_result.clone())
    assert rec["0"][0] == rec["1"][0], (rec["0"][0], rec["1"][0])
    assert torch.equal(rec["0"][3], rec["1"][3]) and float(rec["0"][3][0]) > 0
    steps = set()
    for n, p in rec["0"][1].items():
        assert torch.equal(p, rec["1"][1][n]), n
    for n, (st, m, v) in rec["0"][2].items():
        st1, m1, v1 = rec["1"][2][n]
        assert st == st1 and torch.equal(m, m1) and torch.equal(v, v1), n
        steps.add(st)
    assert len(steps) > 1, steps          # LayerDrop did skip a layer in some step


@pytest.mark.parametrize("max_grad_norm", [1.0, None])
def test_phoneme_recognizer_loop_logs_the_norm(tmp_path, max_grad_norm):
    from aptai_amd import hostlogic, train_phoneme_recognizer as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    vocab = T.default_vocab()
    w2v = W2V2Config.base(num_hidden_layers=2, layerdrop=0.0)
    torch.manual_seed(0)
    d = tmp_path / "w2v"
    Wav2Vec2Model(w2v).save_pretrained(str(d))
    cfg = T.default_cfg(num_epochs=1, batch_size=2, samples_per_epoch=4, learning_rate=2e-5, huggingface_model_id=str(d),
                        pretrain_cfg=w2v, num_warmup_epochs=2)
    if max_grad_norm is not None:
        cfg.max_grad_norm = max_grad_norm
    model, opt, sched = T.load_model_optimizer(cfg, vocab)
    assert opt.max_grad_norm == max_grad_norm
    tr = torch.utils.data.DataLoader(T.SyntheticCommonPhone(6, 1.0, len(vocab), seed=1), batch_size=2, drop_last=True,
                                     collate_fn=hostlogic.collate_pr)
    va = torch.utils.data.DataLoader(T.SyntheticCommonPhone(2, 1.0, len(vocab), seed=2), batch_size=1, collate_fn=hostlogic.collate_pr)
    random.seed(7)
    hist = T.train(cfg, model, opt, sched, vocab, tr, va, tmp_path / "best-model-ckpt", tmp_path / "last-model-ckpt",
                   tmp_path / "model-ckpts", log=lambda s: None)
    assert len(hist) == 1 and hist[0]["trained_batches"] == 2
    if max_grad_norm is None:
        assert "mean_grad_norm" not in hist[0] and "clipped_steps" not in hist[0]
    else:
        assert math.isfinite(hist[0]["mean_grad_norm"]) and hist[0]["mean_grad_norm"] > 0
        assert 0 <= hist[0]["clipped_steps"] <= hist[0]["trained_batches"]
