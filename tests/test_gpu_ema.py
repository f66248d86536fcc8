"""GPU: the exponential moving average of the weights inside aptai_amd.optim.Adam (csrc/optim.hip: ema_multi_kernel,
swap_multi_kernel).  The arithmetic contract is three rounded fp32 operations per element, ema + w * (p - ema), so every comparison
is bit for bit with the same expression evaluated by torch on CPU fp32 tensors; the swap moves bits.  The model-level tests pin the
weight-copy coherence: inside `opt.ema_weights(model)` an eval forward is that of a fresh model loaded with the averaged tensors, and
the training step behind the scope is the step of a run that never entered it, eagerly and through the graph runner."""
import io
import random
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

# both paths (n % 4 != 0 is the scalar one), one element, the chunk edges of ADAM_CHUNK = 4096, three chunks - max_n far above most rows
ROWS = [1, 3, 4, 5, 4095, 4096, 4097, 4100, 8191, 12288]
MISALIGNED = 4104       # n % 4 == 0, but the parameter starts one element into its storage: the scalar path


def _w32(decay):
    """(float)(1.0 - decay): the double difference rounded once, as the launch argument is."""
    return torch.tensor(1.0 - decay, dtype=torch.float32)


def _lerp(e, p, w):
    """e + w * (p - e) on CPU fp32 tensors: three separately rounded operations."""
    assert e.device.type == p.device.type == "cpu" and e.dtype == p.dtype == w.dtype == torch.float32
    return e + w * (p - e)


def _table(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g).cuda() for n in ROWS]
    buf = torch.zeros(MISALIGNED + 8).cuda()
    buf[1:1 + MISALIGNED] = torch.randn(MISALIGNED, generator=g).cuda()
    ps.append(buf[1:1 + MISALIGNED])
    assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
    es = [torch.randn(p.numel(), generator=g).cuda() for p in ps]
    assert all(e.data_ptr() % 16 == 0 for e in es)
    table = torch.tensor([[p.data_ptr(), 0, 0, 0, p.numel(), 0] for p in ps], dtype=torch.int64).cuda()
    ema_dev = torch.tensor([e.data_ptr() for e in es], dtype=torch.int64).cuda()
    return ps, es, table, ema_dev, buf


@pytest.mark.parametrize("decay", [0.999, 0.9, 0.0])
def test_ema_kernel_is_bit_exact_against_three_rounded_operations(decay):
    from aptai_amd import ops
    ps, es, table, ema_dev, buf = _table(1)
    w = _w32(decay)
    p_cpu, expect = [p.cpu() for p in ps], [e.cpu() for e in es]
    for rep in range(3):
        ops.ema_multi(table.data_ptr(), ema_dev.data_ptr(), len(ps), max(ROWS), float(w))
        expect = [_lerp(e, p, w) for e, p in zip(expect, p_cpu)]
        for i, (e, x) in enumerate(zip(es, expect)):
            assert torch.equal(e.cpu(), x), (decay, rep, i, ps[i].numel())
    assert all(torch.equal(p.cpu(), q) for p, q in zip(ps, p_cpu))              # the parameters are read only
    assert buf[0] == 0 and torch.count_nonzero(buf[1 + MISALIGNED:]) == 0       # nothing beside the misaligned row was written


def test_swap_kernel_exchanges_and_restores():
    from aptai_amd import ops
    ps, es, table, ema_dev, buf = _table(2)
    p0, e0 = [p.clone() for p in ps], [e.clone() for e in es]
    ops.swap_multi(table.data_ptr(), ema_dev.data_ptr(), len(ps), max(ROWS))
    for i, (p, e) in enumerate(zip(ps, es)):
        assert torch.equal(p, e0[i]) and torch.equal(e, p0[i]), i
    assert buf[0] == 0 and torch.count_nonzero(buf[1 + MISALIGNED:]) == 0
    ops.swap_multi(table.data_ptr(), ema_dev.data_ptr(), len(ps), max(ROWS))
    for i, (p, e) in enumerate(zip(ps, es)):
        assert torch.equal(p, p0[i]) and torch.equal(e, e0[i]), i


# ------------------------------------------------------------------------------------------------------------------ optimiser
# tests/test_gpu_grad_accum.py: SHAPES (vector path, scalar path, one element, exactly one chunk, two chunks + odd tail), a parameter
# whose gradient is absent in some steps and one that never gets a gradient
SHAPES = [(768, 768), (3072,), (46, 768), (13,), (1, 1, 128), (5, 7), (1,), (4096,), (8197,), (300,)]
SOMETIMES, NEVER = 1, len(SHAPES) - 1


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in SHAPES]


def _groups(ps, **kw):
    from aptai_amd.optim import Adam
    return Adam([dict(params=ps[:4], lr=1e-2), dict(params=ps[4:], lr=3e-3)], weight_decay=0.01, **kw)


def _assign(ps, gen, absent=()):
    for i, p in enumerate(ps):
        p.grad = None if i == NEVER or i in absent else torch.randn(p.shape, generator=gen).cuda()


def _same_state(oa, a, ob, b):
    for i, (pa, pb) in enumerate(zip(a, b)):
        assert torch.equal(pa, pb), i
        sa, sb = oa.state[pa], ob.state[pb]
        assert sa["step"] == sb["step"], i
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), i


@pytest.mark.parametrize("warmup,max_grad_norm", [(False, None), (True, None), (False, 1.0)])
def test_five_steps_average_every_parameter_and_change_no_update(warmup, max_grad_norm):
    from aptai_amd.optim import ema_decay_at
    a, b = _params(1), _params(1)
    oa = _groups(a, ema_decay=0.9, ema_warmup=warmup, max_grad_norm=max_grad_norm)
    ob = _groups(b, max_grad_norm=max_grad_norm)
    ga, gb = torch.Generator().manual_seed(2), torch.Generator().manual_seed(2)
    expect = [p.detach().cpu() for p in a]                      # the average starts from the initial parameters
    assert oa.ema_updates == 0 and oa.ema_parameter(a[0]) is None
    for step in range(1, 6):
        absent = (SOMETIMES,) if step in (2, 4) else ()
        _assign(a, ga, absent)
        _assign(b, gb, absent)
        oa.step()
        ob.step()
        assert oa.ema_updates == step
        w = _w32(ema_decay_at(step, 0.9, warmup))
        expect = [_lerp(e, p.detach().cpu(), w) for e, p in zip(expect, a)]
        for i, (p, e) in enumerate(zip(a, expect)):
            got = oa.ema_parameter(p)
            assert got.shape == p.shape and torch.equal(got.cpu(), e), (step, i)
    _same_state(oa, a, ob, b)                                   # averaging changes no bit of the update
    assert oa.state[a[SOMETIMES]]["step"] == 3 and oa.state[a[NEVER]]["step"] == 0
    assert not torch.equal(oa.ema_parameter(a[SOMETIMES]), a[SOMETIMES])
    assert torch.equal(oa.ema_parameter(a[NEVER]), a[NEVER])    # it never moved: its average is itself
    assert ob.ema_parameter(b[0]) is None and ob._ema is None and ob.ema_updates == 0
    assert set(oa.state_dict()) == {"state", "param_groups"}


def test_off_means_off_and_on_adds_one_launch(monkeypatch):
    from aptai_amd import _lib
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    for decay in (None, 0.9):
        ps = _params(5)
        opt = _groups(ps, ema_decay=decay)
        gen = torch.Generator().manual_seed(6)
        per_step = []
        for step in range(3):
            _assign(ps, gen)
            del calls[:]
            opt.prepare(early=ps[:2])
            opt.launch_early(ps[:2])
            opt.finish()
            per_step.append(list(calls))
        if decay is None:
            assert per_step == [["aptai_adam_multi"] * 3] * 3, per_step         # group 0 early and late, group 1 late
            assert opt._ema is None and opt._accum is None and opt._clip_result is None
        else:
            assert per_step == [["aptai_adam_multi"] * 2 + ["aptai_ema_multi"]] * 3, per_step     # `early` is ignored
    # no allocation after the first averaged step
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    opt.step()
    assert torch.cuda.memory_allocated() == before
    # nothing had a gradient: nothing is updated, nothing is averaged
    for p in ps:
        p.grad = None
    del calls[:]
    opt.step()
    assert calls == [] and opt.ema_updates == 4


def test_accumulation_averages_once_per_update():
    a = _params(1)
    oa = _groups(a, ema_decay=0.9, gradient_accumulation_steps=3)
    gen = torch.Generator().manual_seed(3)
    w = _w32(0.9)
    expect = [p.detach().cpu() for p in a]
    for micro in range(1, 8):
        _assign(a, gen, (SOMETIMES,) if micro == 2 else ())
        before = None if oa._ema is None else [oa.ema_parameter(p).clone() for p in a]
        oa.step()
        if micro in (3, 6):
            assert oa.last_step_updated and oa.ema_updates == micro // 3
            expect = [_lerp(e, p.detach().cpu(), w) for e, p in zip(expect, a)]
        else:
            assert not oa.last_step_updated and oa.ema_updates == micro // 3
            if before is not None:
                assert all(torch.equal(oa.ema_parameter(p), x) for p, x in zip(a, before)), micro
        assert all(torch.equal(oa.ema_parameter(p).cpu(), e) for p, e in zip(a, expect)), micro
    with pytest.raises(RuntimeError):
        with oa.ema_weights():                                   # not while a window is open
            pass
    assert oa.flush() is True and oa.ema_updates == 3
    expect = [_lerp(e, p.detach().cpu(), w) for e, p in zip(expect, a)]
    assert all(torch.equal(oa.ema_parameter(p).cpu(), e) for p, e in zip(a, expect))
    assert oa.flush() is False and oa.ema_updates == 3


def _through_a_file(sd):
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, weights_only=True)


def test_ema_state_dict_round_trip_also_after_publish_to():
    from aptai_amd import ops
    a = _params(1)
    oa = _groups(a, ema_decay=0.9, ema_warmup=True)
    ga = torch.Generator().manual_seed(4)
    for step in range(3):
        _assign(a, ga, (SOMETIMES,) if step == 1 else ())
        oa.step()
    esd = oa.ema_state_dict()
    assert set(esd) == {"decay", "warmup", "updates", "ema"} and esd["updates"] == 3 and len(esd["ema"]) == len(a)
    assert all(torch.equal(t, oa.ema_parameter(p)) and t.data_ptr() != oa.ema_parameter(p).data_ptr() for t, p in zip(esd["ema"], a))
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = _groups(b)                                              # averaging off until the state says otherwise
    ob.load_ema_state_dict(_through_a_file(esd))
    ob.load_state_dict(_through_a_file(oa.state_dict()))         # rebuilds the job tables: the averages stay
    assert ob.ema_decay == 0.9 and ob.ema_warmup is True and ob.ema_updates == 3
    assert all(torch.equal(ob.ema_parameter(q), oa.ema_parameter(p)) for p, q in zip(a, b))
    # publish_to() rebuilds the tables as well: a stand-in model whose cast plan has two of the parameters as sources
    dst = [torch.zeros(b[i].shape, dtype=torch.bfloat16, device="cuda") for i in (0, 1)]
    plan = ops.CastPlan([(b[i].detach(), d) for i, d in zip((0, 1), dst)])
    moved = []
    ob.publish_to(SimpleNamespace(_layer_plan=lambda: plan, weights_moved=lambda: moved.append(1)))
    assert all(torch.equal(ob.ema_parameter(q), oa.ema_parameter(p)) for p, q in zip(a, b))
    gb = torch.Generator().manual_seed(9)
    ga.manual_seed(9)
    for step in range(2):
        _assign(a, ga)
        _assign(b, gb)
        oa.step()
        ob.step()
    _same_state(oa, a, ob, b)
    assert oa.ema_updates == ob.ema_updates == 5
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(oa.ema_parameter(p), ob.ema_parameter(q)), i
    assert all(torch.equal(d, b[i].detach().to(torch.bfloat16)) for i, d in zip((0, 1), dst))
    # the swap of a publishing optimiser tells the published model by default
    with ob.ema_weights():
        assert moved == [1] and torch.equal(b[0], oa.ema_parameter(a[0]))
        with pytest.raises(RuntimeError):
            ob.step()                                            # not on the averages
        with pytest.raises(RuntimeError):
            with ob.ema_weights():                               # does not nest
                pass
    assert moved == [1, 1] and torch.equal(b[0], a[0])


# ------------------------------------------------------------------------------------------------------------------ model level
def _two_layers():
    """The two-layer base configuration, regularisers 0 (so that two runs see the same numbers)."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0.0, apply_spec_augment=False, vocab_size=46)
    return cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)


def _eval_forward(model, batch):
    with torch.no_grad():
        out = model(0, **batch)
    return [out[k].clone() for k in ("loss", "tvs_pred", "phn_fc_pred")]


def _same(xs, ys):
    return all(torch.equal(x, y) for x, y in zip(xs, ys))


def _run(mode, scope):
    """Three training steps, then (scope) evaluation on the averaged weights - once through the context manager, once through two
    swap_ema() calls by hand - then one more training step.  Returns the final parameters by name."""
    from aptai_amd.graphed import BucketedGraphedStep
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_aptai import _build
    cfg, sd = _two_layers()
    host = synth.synth_aptai_batch(cfg, 2, 16000, seed=3)
    batch = {k: v.cuda() for k, v in host.items()}
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = Adam([p for _, p in named], lr=1e-3, weight_decay=0.01, ema_decay=0.5).publish_to(model)
    runner = BucketedGraphedStep(model, opt, bucket_samples=[16000]) if mode == "bucketed" else None

    def train_step():
        if runner is not None:
            return runner.step(host)
        opt.zero_grad(set_to_none=True)
        model(0, **batch)["loss"].backward()
        opt.step()
    try:
        for _ in range(3):
            train_step()
        assert opt.ema_updates == 3
        if scope:
            model.eval()
            before = {k: v.clone() for k, v in model.state_dict().items()}
            averaged = {n: opt.ema_parameter(p).clone() for n, p in named}
            with opt.ema_weights(model):
                inside_sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
                inside = _eval_forward(model, batch)
            for n, _ in named:
                assert torch.equal(inside_sd[n], averaged[n].cpu()), n
            assert not torch.equal(inside_sd["wav2vec2.encoder.layers.0.feed_forward.intermediate_dense.weight"],
                                   before["wav2vec2.encoder.layers.0.feed_forward.intermediate_dense.weight"].cpu())
            after = model.state_dict()
            assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
            outside = _eval_forward(model, batch)
            assert not _same(inside, outside)
            fresh = _build(cfg, inside_sd, tv_drop=0.0, phn_drop=0.0)
            fresh.eval()
            assert _same(_eval_forward(fresh, batch), inside)                    # no stale weight copy anywhere in the forward
            raw = _build(cfg, {k: v.cpu() for k, v in before.items()}, tv_drop=0.0, phn_drop=0.0)
            raw.eval()
            assert _same(_eval_forward(raw, batch), outside)                     # nor behind the scope
            del fresh, raw
            opt.swap_ema(model)                                                  # the same by hand
            assert _same(_eval_forward(model, batch), inside)
            opt.swap_ema(model)
            assert all(torch.equal(model.state_dict()[k], before[k]) for k in before)
            assert _same(_eval_forward(model, batch), outside)
            for n, p in named:
                assert torch.equal(opt.ema_parameter(p), averaged[n]), n
            model.train()
        train_step()
        assert opt.ema_updates == 4
        torch.cuda.synchronize()
    finally:
        if runner is not None:
            runner.close()
    return {n: p.detach().clone() for n, p in named}, {n: opt.ema_parameter(p).clone() for n, p in named}


@pytest.mark.parametrize("mode", ["eager", "bucketed"])
def test_scope_is_coherent_and_leaves_no_trace_in_training(mode):
    (p_in, e_in), (p_out, e_out) = _run(mode, True), _run(mode, False)
    for n in p_out:
        assert torch.equal(p_in[n], p_out[n]), n
        assert torch.equal(e_in[n], e_out[n]), n


# ------------------------------------------------------------------------------------------------------------------ training loops
def _aptai_epoch(tmp_path, ema_decay):
    from aptai_amd import hostlogic, train_aptai as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    w2v = W2V2Config.base(vocab_size=T.VOCAB_SIZE, num_hidden_layers=2, layerdrop=0.0)
    torch.manual_seed(0)
    tmp_path.mkdir(parents=True, exist_ok=True)
    d = tmp_path / "w2v"
    Wav2Vec2Model(w2v).save_pretrained(str(d))
    cfg = T.default_cfg(num_epochs=1, batch_size=2, learning_rate=2e-4, huggingface_model_id=str(d), pretrain_cfg=w2v, num_warmup_epochs=2)
    if ema_decay is not None:
        cfg.ema_decay = ema_decay
    model, opt, sched = T.load_model_optimizer(cfg)
    tr = torch.utils.data.DataLoader(T.SyntheticHPRC(6, 1.0, vary_length=True, seed=1, cfg=w2v), batch_size=2, drop_last=True,
                                     collate_fn=hostlogic.collate_aptai)
    va = torch.utils.data.DataLoader(T.SyntheticHPRC(2, 1.0, seed=2, cfg=w2v), batch_size=1, collate_fn=hostlogic.collate_aptai)
    hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lambda s: None)
    return model, opt, hist


def test_aptai_loop_saves_the_averaged_weights_and_keeps_training_on_the_raw_ones(tmp_path):
    model, opt, hist = _aptai_epoch(tmp_path / "on", 0.5)
    assert len(hist) == 1 and hist[0]["saved"] and hist[0]["ema_updates"] == 3 and opt.ema_updates == 3
    sd = torch.load(tmp_path / "on" / "best" / "pytorch_model.bin", weights_only=True)
    assert set(sd) == set(model.state_dict())
    moved = []
    for n, p in model.named_parameters():
        e = opt.ema_parameter(p)
        if e is None:                                                           # the float64 low-pass taps: never trained, no average
            assert p.dtype != torch.float32 and torch.equal(sd[n].cuda(), p), n
            continue
        assert torch.equal(sd[n].cuda(), e), n                                  # the best checkpoint holds the averages
        if not torch.equal(e, p):
            moved.append(n)
    assert len([n for n in moved if "encoder.layers" in n]) == 2 * 16, moved    # and the model does not (any more)
    twin, topt, thist = _aptai_epoch(tmp_path / "off", None)
    assert "ema_updates" not in thist[0] and topt.ema_parameter(next(twin.parameters())) is None
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n                                             # it holds the raw weights of a run without averaging
    tsd = torch.load(tmp_path / "off" / "best" / "pytorch_model.bin", weights_only=True)
    assert all(torch.equal(tsd[n].cuda(), q) for n, q in twin.named_parameters())


def test_phoneme_recognizer_loop_writes_the_averages_beside_the_optimiser_state(tmp_path):
    from aptai_amd import hostlogic, train_phoneme_recognizer as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    vocab = T.default_vocab()
    w2v = W2V2Config.base(num_hidden_layers=2, layerdrop=0.0)
    torch.manual_seed(0)
    d = tmp_path / "w2v"
    Wav2Vec2Model(w2v).save_pretrained(str(d))
    cfg = T.default_cfg(num_epochs=1, batch_size=2, samples_per_epoch=6, learning_rate=2e-4, huggingface_model_id=str(d),
                        pretrain_cfg=w2v, num_warmup_epochs=2, ema_decay=0.5, ema_warmup=True)
    model, opt, sched = T.load_model_optimizer(cfg, vocab)
    assert opt.ema_decay == 0.5 and opt.ema_warmup is True
    tr = torch.utils.data.DataLoader(T.SyntheticCommonPhone(6, 1.0, len(vocab), seed=1), batch_size=2, drop_last=True,
                                     collate_fn=hostlogic.collate_pr)
    va = torch.utils.data.DataLoader(T.SyntheticCommonPhone(2, 1.0, len(vocab), seed=2), batch_size=1, collate_fn=hostlogic.collate_pr)
    random.seed(7)
    hist = T.train(cfg, model, opt, sched, vocab, tr, va, tmp_path / "best-model-ckpt", tmp_path / "last-model-ckpt",
                   tmp_path / "model-ckpts", log=lambda s: None)
    assert hist[0]["ema_updates"] == 3
    last = tmp_path / "last-model-ckpt"
    assert {f.name for f in last.iterdir()} == {"optimizer.pt", "scheduler.pt", "pytorch_model.bin", "model_cfg.pkl", "ema.pt"}
    esd = torch.load(last / "ema.pt", weights_only=True)
    assert esd["decay"] == 0.5 and esd["warmup"] is True and esd["updates"] == 3
    params = [p for g in opt.param_groups for p in g["params"]]
    assert len(esd["ema"]) == len(params)
    best = torch.load(tmp_path / "best-model-ckpt" / "pytorch_model.bin", weights_only=True)
    lastw = torch.load(last / "pytorch_model.bin", weights_only=True)
    for (n, p), t in zip(model.named_parameters(), esd["ema"]):
        assert torch.equal(t.cuda(), opt.ema_parameter(p)) and torch.equal(best[n].cuda(), t.cuda()), n     # best: the averages
        assert torch.equal(lastw[n].cuda(), p), n                                                           # last: the raw weights
    fresh = T.load_model_optimizer(cfg, vocab)[1]
    fresh.load_ema_state_dict(esd)
    assert fresh.ema_updates == 3 and all(torch.equal(fresh.ema_parameter(q), t.cuda())
                                          for q, t in zip((p for g in fresh.param_groups for p in g["params"]), esd["ema"]))
