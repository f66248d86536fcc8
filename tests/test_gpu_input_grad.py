"""GPU: gradients w.r.t. the INPUT WAVEFORM (`audio_inputs.requires_grad_()`, then `backward()` fills `audio_inputs.grad`), through
aptai_conv0_bwd_data (the data gradient of the first conv layer) and the layer 6 -> 1 dgrad GEMMs of the conv stack.

Bars: the kernel against fp64 autograd with the kernels' own GELU: max error / max |ref| < 2e-5.  Model level (bf16 product against the
fp32 oracle / reference): the gradient bar of test_gpu_aptai.py, relative L2 < 8e-2 and |norm ratio - 1| < 5e-2.  Measured on one
MI355X (relL2 / norm ratio): APTAI large 24 layers 0.041 / 0.999 (reference and oracle), base 3 layers 0.056 / 0.999, trainable conv
stack 0.064 / 0.999, get_embeddings_grad 0.016 / 0.999, its features_hidden 0.010 / 1.000, Wav2Vec2Model with a mask 0.014 / 1.000.
Switching the input gradient on changes neither the loss nor any parameter gradient (bit equality)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
A1, A3, A5 = 1.59499531, 7.40885562e-2, -7.23764583e-4
TV = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")
NOREG = dict(hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0., final_dropout=0., layerdrop=0.,
             apply_spec_augment=False)


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _check_grad(got, ref, name):
    r = _rel(got, ref)
    ratio = got.double().norm().item() / (ref.double().norm().item() + 1e-30)
    print(f"[input-grad] {name}: relL2 {r:.4f}  norm ratio {ratio:.4f}")
    assert r < 8e-2 and abs(ratio - 1) < 5e-2, (name, r, ratio)


def _frames(lengths):
    from aptai_amd import hostlogic
    return hostlogic.feat_extract_output_lengths(torch.as_tensor(lengths).reshape(-1).long(), (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))


# ------------------------------------------------------------------------------------------------ (a) the kernel
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,S,ragged", [(2, 16000, False), (3, 20483, True)])
def test_conv0_bwd_data_against_fp64_autograd(mode, B, S, ragged):
    from aptai_amd import ops
    g = torch.Generator().manual_seed(13 + mode)
    audio = torch.randn(B, S, generator=g)
    w = torch.randn(512, 1, 10, generator=g) * 0.3
    bias = 0.1 * torch.randn(512, generator=g) if mode == 1 else None
    gamma = 1.0 + 0.1 * torch.randn(512, generator=g)
    beta = 0.1 * torch.randn(512, generator=g)
    T = (S - 10) // 5 + 1                                   # ragged: not a multiple of 16 (the matrix-pipe block) or 256 (a chunk)
    Ta = (T + 63) // 64 * 64
    dy = (torch.randn(B, Ta, 512, generator=g) * 0.5).to(torch.bfloat16)
    dy[:, T:] = 7.0                                         # rows beyond T_real must not reach the result
    dev = "cuda"
    P = [None if t is None else t.to(dev) for t in (audio, w, bias, gamma, beta)]
    out = torch.empty(B, Ta, 512, device=dev, dtype=torch.bfloat16)
    stats = ops.conv0_fwd(P[0], P[1], P[2], P[3], P[4], mode, out, T, Ta, want_stats=True)
    args = (P[0], P[1], P[2], P[3], P[4], mode, dy.to(dev), T, Ta, stats)
    got = ops.conv0_bwd_data(*args)
    again = ops.conv0_bwd_data(*args)
    torch.cuda.synchronize()
    assert got.shape == (B, S) and got.dtype == torch.float32
    assert torch.equal(got, again)                          # no atomics: bit-identical run to run
    x = audio.double().requires_grad_()
    v = torch.nn.functional.conv1d(x[:, None], w.double(), bias=None if bias is None else bias.double(), stride=5)
    if mode == 0:
        xh = (v - v.mean(-1, keepdim=True)) / torch.sqrt(v.var(-1, unbiased=False, keepdim=True) + 1e-5)
    else:
        xh = (v - v.mean(1, keepdim=True)) / torch.sqrt(v.var(1, unbiased=False, keepdim=True) + 1e-5)
    z = xh * gamma.double()[None, :, None] + beta.double()[None, :, None]
    y = z * torch.sigmoid(z * (A1 + A3 * z * z + A5 * z ** 4))
    (y * dy[:, :T].double().transpose(1, 2)).sum().backward()
    ref = x.grad
    err = (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 2e-5, err
    last = 5 * (T - 1) + 10                                 # samples past the last window: exactly 0
    if last < S:
        assert (got[:, last:] == 0).all()


def test_conv0_bwd_data_rejects_cpu_tensors():
    from aptai_amd import _lib, ops
    t = torch.zeros(1, 400)
    with pytest.raises(_lib.AptaiHipError):
        ops.conv0_bwd_data(t, torch.zeros(512, 1, 10), None, torch.ones(512), torch.zeros(512), 1, torch.zeros(1, 79, 512), 79, 79, None)


# ------------------------------------------------------------------------------------------------ (b) APTAI, frozen conv stack
def _aptai_oracle_grad(cfg, sd, batch, **kw):
    from oracle import heads_ref
    a = batch["audio_inputs"].clone().requires_grad_(True)
    ref = heads_ref.aptai_forward(sd, cfg, a, batch["audio_lengths"], batch["phn_frames_49hz"], [batch[n] for n in TV], training=True,
                                  tv_drop=0.0, phn_drop=0.0, **kw)
    ref["loss"].backward()
    return a.grad


def _aptai_grad(model, batch):
    cb = {k: v.cuda() for k, v in batch.items()}
    a = cb["audio_inputs"].clone().requires_grad_(True)
    cb["audio_inputs"] = a
    out = model(0, **cb)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert a.grad is not None
    return a.grad.cpu(), out


def test_aptai_large_24_layers_frozen_conv_waveform_gradient():
    """APTAI as shipped (LayerNorm conv stack, frozen), train mode with regularisers at 0: audio.grad against the reference fixture and
    the oracle; zero beyond each utterance's receptive field."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_aptai import _build
    z, meta = load_golden("inputgrad_2x1s")
    m = meta["layer"]
    cfg = W2V2Config.from_any(m["cfg"])
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), m["seed"])
    batch = {k[len("layer/in/"):]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith("layer/in/")}
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    got, _ = _aptai_grad(model, batch)
    _check_grad(got, torch.from_numpy(z["layer/audio_grad"]), "large-24 vs reference")
    _check_grad(got, _aptai_oracle_grad(cfg, sd, batch), "large-24 vs oracle")
    for n, p in model.named_parameters():
        if "feature_extractor" in n:
            assert p.grad is None
    S = got.shape[1]
    T0 = (S - 10) // 5 + 1
    for b, Tb in enumerate(_frames(batch["audio_lengths"]).tolist()):
        edge = min(320 * (Tb - 1) + 400, 5 * (T0 - 1) + 10)
        assert (got[b, edge:] == 0).all(), (b, edge)
        assert got[b, :edge].abs().max() > 0


def test_aptai_base_arch_frozen_conv_waveform_gradient():
    """GroupNorm conv stack (wav2vec2-base shape), 3 layers: against the oracle (the reference cannot run APTAI on the base arch)."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=3, vocab_size=46, **NOREG)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = synth.synth_aptai_batch(cfg, 2, 20800, seed=1234)
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    got, _ = _aptai_grad(model, batch)
    _check_grad(got, _aptai_oracle_grad(cfg, sd, batch), "base-3 vs oracle")
    T0 = (got.shape[1] - 10) // 5 + 1
    assert (got[:, 5 * (T0 - 1) + 10:] == 0).all()


# ------------------------------------------------------------------------------------------------ (c) trainable conv stack
def test_trainable_conv_stack_waveform_gradient_against_the_oracle():
    """freeze_feature_encoder=False, train mode: the reference raises here (HF sets requires_grad on a view of the input); we compute it."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.large(num_hidden_layers=2, vocab_size=46, **NOREG)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = synth.synth_aptai_batch(cfg, 2, 16000, seed=1234)
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0, freeze_feature_encoder=False)
    model.train()
    got, _ = _aptai_grad(model, batch)
    _check_grad(got, _aptai_oracle_grad(cfg, sd, batch), "large-2 trainable conv vs oracle")
    assert model.wav2vec2.feature_extractor.conv_layers[0].conv.weight.grad is not None


def _step_pair(model, batch, reset):
    """One step without and one with audio.requires_grad_() from the same (seed, step): (loss, tvs_pred, every parameter gradient)."""
    res = []
    for want in (False, True):
        reset()
        model.zero_grad(set_to_none=True)
        cb = {k: v.cuda() for k, v in batch.items()}
        if want:
            cb["audio_inputs"] = cb["audio_inputs"].clone().requires_grad_(True)
        out = model(0, **cb)
        out["loss"].backward()
        torch.cuda.synchronize()
        assert (cb["audio_inputs"].grad is not None) == want
        res.append((out["loss"].detach().clone(), out["tvs_pred"].detach().clone(),
                    {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    (l0, tv0, g0), (l1, tv1, g1) = res
    assert torch.equal(l0, l1)
    assert torch.equal(tv0, tv1)
    assert set(g0) == set(g1) and len(g0) > 10
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, bad
    return g0


@pytest.mark.parametrize("frozen", [False, True])
def test_input_gradient_changes_no_loss_or_parameter_gradient(frozen):
    """(c) trainable conv stack with the reference's regularisers ON and (d) frozen conv stack: loss, tvs_pred and every parameter gradient
    are bit-equal with and without audio.requires_grad_() (the saving conv forward runs the same kernels as the scratch path)."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_aptai import _build
    if frozen:
        cfg = W2V2Config.large(num_hidden_layers=3, vocab_size=46, **NOREG)
        model = _build(cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0), tv_drop=0.0, phn_drop=0.0)
    else:
        cfg = W2V2Config.large(num_hidden_layers=3, vocab_size=46, layerdrop=0.3)
        model = _build(cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0), freeze_feature_encoder=False)
    model.train()
    batch = synth.synth_aptai_batch(cfg, 2, 24000, seed=7)
    w = model.wav2vec2

    def reset():
        w._step = 11
        w._layerdrop_gen.manual_seed(0x1A7E)
        np.random.seed(5)
    g = _step_pair(model, batch, reset)
    assert any("feature_extractor" in n for n in g) != frozen


def test_base_arch_frozen_conv_input_gradient_changes_nothing_else():
    """(d) in group mode: the GroupNorm conv stack's saving forward (pre-activations kept) against the scratch path."""
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=2, vocab_size=46, **NOREG)
    model = _build(cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0), tv_drop=0.0, phn_drop=0.0)
    model.train()
    w = model.wav2vec2

    def reset():
        w._step = 3
    _step_pair(model, synth.synth_aptai_batch(cfg, 2, 17600, seed=2), reset)


# ------------------------------------------------------------------------------------------------ (e) get_embeddings_grad
def test_get_embeddings_grad_waveform_gradient():
    from aptai_amd.config import W2V2Config
    from oracle import heads_ref, synth
    from test_gpu_ctc_pr import _build_pr
    z, meta = load_golden("inputgrad_2x1s")
    m = meta["group"]
    cfg = W2V2Config.from_any(m["cfg"])
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), m["seed"])
    model = _build_pr(cfg, sd)
    model.eval()
    x0, lens = torch.from_numpy(z["group/in/input_values"]), torch.from_numpy(z["group/in/input_lengths"])
    x = x0.cuda().requires_grad_(True)
    out = model.get_embeddings_grad(x, lens.cuda(), model.vocab, m["intermediate_hidden"], m["latter_hidden"])
    (out["phoneme_logits_inter"].float().pow(2).sum() + out["phoneme_logits_last"].float().pow(2).sum()).backward()
    got = x.grad.cpu()
    _check_grad(got, torch.from_numpy(z["group/audio_grad"]), "get_embeddings_grad vs reference")
    xo = x0.clone().requires_grad_(True)
    ro = heads_ref.pr_get_embeddings_grad(sd, cfg, xo, lens, m["intermediate_hidden"], m["latter_hidden"])
    (ro["phoneme_logits_inter"].pow(2).sum() + ro["phoneme_logits_last"].pow(2).sum()).backward()
    _check_grad(got, xo.grad, "get_embeddings_grad vs oracle")
    # features_hidden carries the gradient to the waveform too (the reference's separate feature_extractor pass)
    x2 = x0.cuda().requires_grad_(True)
    out = model.get_embeddings_grad(x2, lens.cuda(), model.vocab, m["intermediate_hidden"], m["latter_hidden"])
    R = torch.randn(out["features_hidden"].shape, generator=torch.Generator().manual_seed(4))
    (out["features_hidden"].float() * R.cuda()).sum().backward()
    xo2 = x0.clone().requires_grad_(True)
    ro = heads_ref.pr_get_embeddings_grad(sd, cfg, xo2, lens, m["intermediate_hidden"], m["latter_hidden"])
    (ro["features_hidden"] * R).sum().backward()
    _check_grad(x2.grad.cpu(), xo2.grad, "features_hidden vs oracle")


# ------------------------------------------------------------------------------------------------ (f) Wav2Vec2Model, (g) determinism
def test_wav2vec2_model_waveform_gradient_with_explicit_mask():
    from aptai_amd import hostlogic
    from aptai_amd.config import W2V2Config
    from oracle import synth, w2v2_ref
    from test_gpu_ctc_pr import _build_pr
    cfg = W2V2Config.base(num_hidden_layers=2, vocab_size=40, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=True, mask_time_prob=0.05)
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    w = _build_pr(cfg, sd).wav2vec2
    w.train()
    sb = synth.synth_aptai_batch(cfg, 2, 16000, seed=21)
    x0, lens = sb["audio_inputs"], sb["audio_lengths"].reshape(-1)
    fl = _frames(lens)
    T = (16000 - 400) // 320 + 1
    np.random.seed(3)
    mask = hostlogic.compute_mask_indices((2, T), 0.05, 10, attention_mask=torch.arange(T)[None] < fl[:, None], min_masks=2)
    assert mask.any()
    x = x0.cuda().requires_grad_(True)
    h = w(x, attention_mask=lens.cuda()[:, None], mask_time_indices=torch.from_numpy(mask)).last_hidden_state
    R = torch.randn(h.shape, generator=torch.Generator().manual_seed(8))
    (h.float() * R.cuda()).sum().backward()
    xo = x0.clone().requires_grad_(True)
    ro = w2v2_ref.wav2vec2_forward(sd, cfg, xo, lens, "wav2vec2.", True, torch.from_numpy(mask))
    (ro["last_hidden_state"] * R).sum().backward()
    _check_grad(x.grad.cpu(), xo.grad, "Wav2Vec2Model (masked) vs oracle")


def test_eval_waveform_gradient_is_bit_reproducible():
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=2, vocab_size=46, **NOREG)
    model = _build(cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0))
    model.eval()
    batch = synth.synth_aptai_batch(cfg, 3, 24000, seed=5)
    grads = []
    for _ in range(2):
        got, _ = _aptai_grad(model, batch)
        grads.append(got)
    assert grads[0].abs().max() > 0
    assert torch.equal(grads[0], grads[1])
