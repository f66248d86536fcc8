"""GPU: batch-invariant inference (`batch_invariant`, aptai_conv0_fwd_lens, aptai_lowpass_fir_lens): every row of a batch returns what
the utterance returns at batch size 1.

One batch for every test: 4 waveforms padded to 16000 samples, lengths 16000 / 5125 / 5130 / 4321 = 3199 / 1024 / 1025 / 863
first-layer frames (several moment chunks of 1024 frames, exactly one, one frame into the second, plain shorter) and 49 / 15 / 15 / 13
encoder frames, all within ntaps / 2 = 25 of one another, so every window of the low-pass filter crosses a length boundary.

Bounds.
 * The two kernels, operator level: bit for bit the row alone (B = 1, S = its own length); exact zeros beyond the length.
 * conv0 against an fp64 GroupNorm over the row's own frames (with the kernels' own GELU fit, as tests/test_gpu_conv0_bwd.py does):
   the statistics at that test's 2e-5 of the block's largest entry; the bf16 outputs at |err| <= 2^-8 |ref| + 1e-4 - a bf16 rounding is
   2^-9 relative, the other 2^-9 and the absolute term hold the fp32 arithmetic in front of it (10 products, v_exp / v_rcp at 1 ulp).
 * End to end, batched against alone: TOL below.  It was MEASURED, not derived from the code under test: the layer-norm (large-mini)
   encoder has no batch-dependent statistics, so what its rows differ by between a batch and alone - on the parent commit, and with the
   switch off here, the same figures - is what the batch size does to the GEMM plans.  Measured in front of the low-pass filter (the plain filter
   mixes the padded frames into the last 25 valid ones, which is the very thing this feature removes, not a GEMM effect; through it
   the same rows differ by 0.25 for APTAI and 0.06 for Force_APTAI): head logits, the unfiltered trajectories, the recogniser's
   logits and Force_APTAI's unfiltered trajectories in its default precision and in f32x3, on exactly this batch (DESIGN section
   "Batch-invariant inference").  APTAI and the recogniser: 0.0 - the bf16 GEMMs walk K in one order per output row whatever M is -
   so those tests demand bit-equality and equal integer outputs.  Force_APTAI: 4.2e-7 / 4.8e-7 from its fp32 head GEMMs, whose
   split of K follows M; its tests demand at most twice that, times the sum of the filter's |taps| for the filtered trajectories
   (|sum_j taps_j d_j| <= max|d| sum|taps|; the fp64 accumulate adds nothing at this scale).
 * Each row against the CPU oracle run on that utterance alone: the bounds tests/test_gpu_aptai.py and tests/test_gpu_force_base.py use.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = (16000, 5125, 5130, 4321)
S = 16000
FRAMES0 = tuple((n - 10) // 5 + 1 for n in LENS)           # 3199, 1024, 1025, 863
FRAMES = (49, 15, 15, 13)
TV = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")
A1, A3, A5 = 1.59499531, 7.40885562e-2, -7.23764583e-4     # the kernels' GELU fit (csrc/common.h)
# measured maximum |batched - alone| of the layer-norm encoder on this batch, parent commit (module docstring); 0.0 -> bit-equality
TOL = {"aptai_logits": 0.0, "aptai_tv_raw": 0.0, "pr_logits": 0.0,
       "force_tv_raw": 4.172325134277344e-07, "force_tv_raw_f32x3": 4.76837158203125e-07}


def make_audio():
    g = torch.Generator().manual_seed(2024)
    audio = torch.randn(4, S, generator=g)
    lens = torch.tensor(LENS, dtype=torch.long)
    return audio * (torch.arange(S)[None, :] < lens[:, None]), lens


def mini_cfg(kind, **kw):
    from aptai_amd.config import W2V2Config
    make = W2V2Config.base if kind == "base" else W2V2Config.large
    return make(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0.,
                final_dropout=0., layerdrop=0., apply_spec_augment=False, **kw)


def build_aptai(kind):
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = mini_cfg(kind, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    return _build(cfg, sd, tv_drop=0.0, phn_drop=0.0).eval(), cfg, sd


def build_pr(kind):
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg = mini_cfg(kind, vocab_size=40, ctc_loss_reduction="mean", ctc_zero_infinity=True)
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    return _build_pr(cfg, sd).eval(), cfg, sd


def build_force(kind):
    from oracle import synth
    from test_gpu_force import _build
    cfg = mini_cfg(kind, vocab_size=40, ctc_loss_reduction="mean", ctc_zero_infinity=True, blank=0)
    sd = synth.make_state_dict(synth.force_aptai_param_shapes(cfg, 40), 3)
    model, _ = _build(dict(pr_cfg=cfg.to_dict(), vocab_len=40, seed=3), sd)
    return model.eval(), cfg, sd


def phn_lists():
    """A random-weight recogniser decodes next to nothing: Force_APTAI gets its phoneme lists handed in, as in test_gpu_force_base."""
    g = torch.Generator().manual_seed(2)
    return [torch.randint(2, 40, (n,), generator=g).numpy() for n in (12, 5, 6, 4)]


def aptai_batch(audio, lens, rows):
    """Eval-mode APTAI batch of the given rows (targets: padding everywhere; the predictions do not depend on them)."""
    n = int(lens[rows].max())
    T = FRAMES[rows[0]] if len(rows) == 1 else max(FRAMES[r] for r in rows)
    b = {"audio_inputs": audio[rows, :n].contiguous().cuda(), "audio_lengths": lens[rows].cuda(),
         "phn_frames_49hz": torch.zeros(len(rows), T, dtype=torch.long).cuda()}
    for name in TV:
        b[name] = torch.full((len(rows), T), -100.0, dtype=torch.float64).cuda()
    return b


def aptai_eval(model, audio, lens, rows):
    """(tvs_pred [B][T][9], head logits [B][T][n_phn], phn_fc_pred [B][T]) of an eval-mode forward."""
    with torch.no_grad():
        b = aptai_batch(audio, lens, rows)
        w = model.wav2vec2
        from aptai_amd.wav2vec2 import batch_invariant_scope
        with batch_invariant_scope(w, model.batch_invariant):
            enc = w(b["audio_inputs"], attention_mask=b["audio_lengths"][:, None], return_dict=True, output_hidden_states=True)
        _, _, _, tvs, pred, logits = model._heads(enc, None, None)
        g = enc._geom
        return tvs.clone(), logits.view(g.B, g.Tp, -1)[:, :g.T, :model.n_phn].clone(), pred.clone()


def same(a, b, tol, what):
    """|a - b| <= 2 tol, bit-equality when the measured tolerance is 0."""
    if tol == 0.0:
        assert torch.equal(a, b), (what, (a.double() - b.double()).abs().max().item())
    else:
        assert (a.double() - b.double()).abs().max().item() <= 2 * tol, what


ALL = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def data():
    return make_audio()


@pytest.fixture(scope="module")
def aptai_base():
    return build_aptai("base")


@pytest.fixture(scope="module")
def aptai_alone(aptai_base, data):
    """The batch-1 forwards of the four utterances (switch off: at batch 1 it changes nothing, which test 4 also checks)."""
    model = aptai_base[0]
    assert model.batch_invariant is False
    return [aptai_eval(model, data[0], data[1], [r]) for r in ALL]


# ------------------------------------------------------------------------------------------------ 1. conv0, operator level
def _conv0_params(with_bias):
    g = torch.Generator().manual_seed(11)
    w = torch.randn(512, 1, 10, generator=g) * 0.3
    gamma = 1.0 + 0.1 * torch.randn(512, generator=g)
    beta = 0.1 * torch.randn(512, generator=g)
    bias = 0.1 * torch.randn(512, generator=g) if with_bias else None
    return [None if t is None else t.cuda() for t in (w, bias, gamma, beta)]


def _alloc(T, form):
    # "mfma": a multiple of 64 as the model allocates (the matrix-pipe write pass); "vector": not a multiple of 16, which sends the
    # group mode through the all-vector write pass (the APTAI_CONV0_MFMA=0 form)
    return (T + 63) // 64 * 64 if form == "mfma" else T + 3


def _conv0(audio, P, mode, T, Ta, lens0=None):
    from aptai_amd import ops
    out = torch.full((audio.shape[0], Ta, 512), 7.0, device="cuda", dtype=torch.bfloat16)
    stats = ops.conv0_fwd(audio, P[0], P[1], P[2], P[3], mode, out, T, Ta, want_stats=True,
                          frame_lens0=None if lens0 is None else torch.tensor(lens0, dtype=torch.int32).cuda())
    return out, stats


@pytest.mark.parametrize("form", ["mfma", "vector"])
def test_conv0_group_mode_rows_equal_the_row_alone(data, form):
    audio, lens = data
    P = _conv0_params(False)
    T, Ta = FRAMES0[0], _alloc(FRAMES0[0], form)
    assert (Ta % 16 == 0) == (form == "mfma")
    out, stats = _conv0(audio.cuda(), P, 0, T, Ta, FRAMES0)
    poisoned = audio.clone()
    for b, n in enumerate(LENS):
        poisoned[b, n:] = float("nan")
    out_n, stats_n = _conv0(poisoned.cuda(), P, 0, T, Ta, FRAMES0)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out_n.view(torch.int16)) and torch.equal(stats, stats_n)      # padding never read into a result
    assert not torch.isnan(out_n.float()).any() and not torch.isnan(stats_n).any()
    for b, n in enumerate(LENS):
        Tb = FRAMES0[b]
        Tab = _alloc(Tb, form)
        assert (Tab % 16 == 0) == (form == "mfma")
        one, stats1 = _conv0(audio[b:b + 1, :n].contiguous().cuda(), P, 0, Tb, Tab, [Tb])
        assert torch.equal(out[b, :Tb].view(torch.int16), one[0, :Tb].view(torch.int16)), b
        assert torch.equal(stats[b], stats1[0]), b
        assert not out[b, Tb:].float().any() and not one[0, Tb:].float().any(), b                            # exact zeros up to T_alloc
        # fp64 GroupNorm over the row's OWN frames
        v = torch.nn.functional.conv1d(audio[b:b + 1, None, :n].double(), P[0].double().cpu(), stride=5)[0]       # [512][Tb]
        mean, var = v.mean(-1), v.var(-1, unbiased=False)
        ref_stats = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-5)])
        err = (stats[b].double().cpu() - ref_stats).abs().amax(-1) / ref_stats.abs().amax(-1)
        assert (err < 2e-5).all(), (b, err)
        z = (v - mean[:, None]) * ref_stats[1][:, None] * P[2].double().cpu()[:, None] + P[3].double().cpu()[:, None]
        ref = (z * torch.sigmoid(z * (A1 + A3 * z * z + A5 * z ** 4))).t()
        d = (out[b, :Tb].double().cpu() - ref).abs()
        assert (d <= 2.0 ** -8 * ref.abs() + 1e-4).all(), (b, d.max().item())


def test_conv0_layer_mode_zeros_beyond_and_todays_bits_below(data):
    audio, _ = data
    P = _conv0_params(True)
    T, Ta = FRAMES0[0], _alloc(FRAMES0[0], "mfma")
    plain, _ = _conv0(audio.cuda(), P, 1, T, Ta)
    out, stats = _conv0(audio.cuda(), P, 1, T, Ta, FRAMES0)
    assert stats is None
    for b, Tb in enumerate(FRAMES0):
        assert torch.equal(out[b, :Tb].view(torch.int16), plain[b, :Tb].view(torch.int16)), b
        assert not out[b, Tb:].float().any(), b
    assert plain[1, FRAMES0[1]:T].float().any()                                                              # the plain call does write there


# ------------------------------------------------------------------------------------------------ 2. FIR, operator level
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lowpass_fir_rows_equal_the_row_alone(dtype):
    from aptai_amd import ops
    from aptai_amd.modules import LowPassFilterLayer
    taps = LowPassFilterLayer("cuda", 10, 49, 9).taps()
    assert taps.numel() // 2 == 25
    g = torch.Generator().manual_seed(4)
    B, T, Tp, C, ldx, T_out, ldy = 4, 49, 64, 9, 16, 52, 12
    x = torch.randn(B, Tp, ldx, generator=g)
    for b, n in enumerate(FRAMES):
        x[b, n:] = float("nan")                                                                              # frames that do not exist
    x = x.cuda()
    lens = torch.tensor(FRAMES, dtype=torch.int32).cuda()
    y = torch.full((B, T_out, ldy), 5.0, device="cuda", dtype=dtype)
    ops.lowpass_fir(x, ldx, Tp, taps, y, ldy, T_out, B, T, T_out, C, ldy, frame_lens=lens)
    raw = torch.int32 if dtype == torch.float32 else torch.int16
    for b, n in enumerate(FRAMES):
        one = torch.full((1, n, ldy), 5.0, device="cuda", dtype=dtype)
        ops.lowpass_fir(x[b:b + 1].contiguous(), ldx, Tp, taps, one, ldy, n, 1, n, n, C, ldy)                  # today's call, T = its length
        assert torch.equal(y[b, :n].view(raw), one[0].view(raw)), b
        assert not torch.isnan(y[b].float()).any() and not y[b, n:].float().any() and not y[b, :, C:].float().any(), b
        assert y[b, :n, :C].float().abs().max().item() > 0.0


# ------------------------------------------------------------------------------------------------ 3. power check
def test_without_the_switch_a_short_row_differs_from_its_batch_1_result(aptai_base, aptai_alone, data):
    model = aptai_base[0]
    tvs, logits, _ = aptai_eval(model, data[0], data[1], ALL)
    n = FRAMES[3]
    d_tv = (tvs[3, :n] - aptai_alone[3][0][0]).abs().max().item()
    d_lg = (logits[3, :n] - aptai_alone[3][1][0]).abs().max().item()
    print(f"[bands] switch off, 4321-sample row vs alone: tvs_pred {d_tv:.3e}, logits {d_lg:.3e}")
    assert d_tv > 2 * TOL["aptai_tv_raw"] and d_lg > 2 * TOL["aptai_logits"]


# ------------------------------------------------------------------------------------------------ 4. models, end to end
def test_aptai_rows_equal_batch_1_and_meet_the_oracle(aptai_base, aptai_alone, data):
    from oracle import heads_ref
    from test_gpu_aptai import _check_close
    model, cfg, sd = aptai_base
    audio, lens = data
    model.batch_invariant = True
    try:
        tvs, logits, pred = aptai_eval(model, audio, lens, ALL)
        one_on = aptai_eval(model, audio, lens, [3])
    finally:
        model.batch_invariant = False
    assert model.wav2vec2.batch_invariant is False
    for a, b in zip(one_on, aptai_alone[3]):
        assert torch.equal(a, b)                                                                             # batch 1: the switch changes nothing
    l1 = float(model.tv_lowpass.taps().abs().sum())
    for r, n in enumerate(FRAMES):
        tv1, lg1, pr1 = aptai_alone[r]
        same(tvs[r, :n], tv1[0], TOL["aptai_tv_raw"] * l1, f"tvs_pred row {r}")
        same(logits[r, :n], lg1[0], TOL["aptai_logits"], f"logits row {r}")
        assert torch.equal(pred[r, :n], pr1[0]), r
        assert not tvs[r, n:].any(), r
        b1 = aptai_batch(audio, lens, [r])
        ref = heads_ref.aptai_forward(sd, cfg, b1["audio_inputs"].cpu(), b1["audio_lengths"].cpu(), b1["phn_frames_49hz"].cpu(),
                                      [b1[k].cpu() for k in TV], training=False)
        _check_close(tvs[r, :n], ref["tvs_pred"][0], f"tvs_pred row {r} vs oracle", tol_max=4e-2, tol_l2=2.5e-2)


def test_recogniser_logits_equal_batch_1(data):
    audio, lens = data
    model, _, _ = build_pr("base")
    model.batch_invariant = True
    with torch.no_grad():
        emb = model.get_embeddings(audio.cuda(), lens.cuda())
        for r, n in enumerate(FRAMES):
            one = model.get_ctc_logits(audio[r, :LENS[r]].numpy())
            got = emb["phoneme_logits"][r].T[:n]
            same(torch.from_numpy(got.copy()), torch.from_numpy(one), TOL["pr_logits"], f"row {r}")
            e1 = model.get_embeddings(audio[r:r + 1, :LENS[r]].contiguous().cuda(), lens[r:r + 1].cuda())
            assert list(emb["phn_pred_seq_idx"][r]) == list(e1["phn_pred_seq_idx"][0]), r                     # decoded ids stop at the row's end
    assert model.batch_invariant is True and model.wav2vec2.batch_invariant is False


@pytest.mark.parametrize("precision", ["bf16_f32res", "f32x3"])
def test_force_aptai_rows_equal_batch_1_and_meet_the_oracle(data, precision):
    from oracle import heads_ref
    audio, lens = data
    model, cfg, sd = build_force("base")
    model.set_encoder_precision(precision)
    lists = phn_lists()
    tol = TOL["force_tv_raw" if precision == "bf16_f32res" else "force_tv_raw_f32x3"] * float(model.tv_lowpass.taps().abs().sum())
    model.batch_invariant = True
    with torch.no_grad():
        res, g, dec = model._run(audio.cuda(), lens.cuda(), phn_pred_list=lists)
        tvs = res[3].clone()
        frame_phns = res[4].clone()
        for r, n in enumerate(FRAMES):
            a1 = audio[r:r + 1, :LENS[r]].contiguous()
            res1, g1, _ = model._run(a1.cuda(), lens[r:r + 1].cuda(), phn_pred_list=lists[r:r + 1])
            print(f"[bands] {precision} row {r}: |batched - alone| = {(tvs[r, :n] - res1[3][0]).abs().max().item():.3e} (bound {2 * tol:.3e})")
            same(tvs[r, :n], res1[3][0], tol, f"tvs_pred row {r}")
            assert torch.equal(frame_phns[r, :n], res1[4][0, :n]), r
            assert not tvs[r, n:].any(), r
            dummy = [torch.full((1, n), -100.0, dtype=torch.float64)] * 9
            ref = heads_ref.force_aptai_forward(sd, cfg, a1, lens[r:r + 1], dummy, phn_pred_list=lists[r:r + 1])
            ref_tv = ref["tvs_pred"][0]
            assert (tvs[r, :n].cpu() - ref_tv).abs().max().item() <= 4e-2 * ref_tv.abs().max().item(), r
    assert model.w2v2_pr.batch_invariant is False and model.w2v2_pr.wav2vec2.batch_invariant is False


# ------------------------------------------------------------------------------------------------ 5. get_aptai_outputs
def test_get_aptai_outputs_equals_the_per_utterance_helper(aptai_base, data):
    model = aptai_base[0]
    audio, _ = data
    wavs = [audio[r, :n].numpy() for r, n in enumerate(LENS)]
    many = model.get_aptai_outputs(wavs)
    assert model.batch_invariant is False and model.wav2vec2.batch_invariant is False
    l1 = float(model.tv_lowpass.taps().abs().sum())
    assert len(many) == 4
    for r, w in enumerate(wavs):
        one = model.get_aptai_output(w)
        assert set(one) == set(many[r])
        for k in ("phn_fc_probs", "phn_fc_logits", "phn_fc_pred"):
            assert one[k].shape == many[r][k].shape and one[k].dtype == many[r][k].dtype, (r, k)
        same(torch.from_numpy(many[r]["phn_fc_logits"].copy()), torch.from_numpy(one["phn_fc_logits"].copy()), TOL["aptai_logits"], (r, "logits"))
        same(torch.from_numpy(many[r]["phn_fc_probs"].copy()), torch.from_numpy(one["phn_fc_probs"].copy()), TOL["aptai_logits"], (r, "probs"))
        assert np.array_equal(many[r]["phn_fc_pred"], one["phn_fc_pred"]), r
        assert list(many[r]["tvs_pred"]) == list(one["tvs_pred"])
        for name in one["tvs_pred"]:
            a, b = np.asarray(many[r]["tvs_pred"][name]), np.asarray(one["tvs_pred"][name])
            assert a.shape == b.shape == (FRAMES[r],)
            same(torch.from_numpy(a), torch.from_numpy(b), TOL["aptai_tv_raw"] * l1, (r, name))


# ------------------------------------------------------------------------------------------------ 6. loops
def test_validate_at_batch_size_four_equals_batch_size_one(tmp_path):
    from aptai_amd import hostlogic
    from test_gpu_device_metrics import INT_KEYS, _aptai_model, _bound
    T, cfg, w2v, model = _aptai_model(tmp_path)
    cfg.batch_invariant_eval = True
    ds = torch.utils.data.ConcatDataset([T.SyntheticHPRC(1, sec, vary_length=False, seed=9 + i, cfg=w2v)
                                         for i, sec in enumerate((1.0, 0.8, 0.6, 0.45))])

    def run(bs):
        dl = torch.utils.data.DataLoader(ds, batch_size=bs, collate_fn=hostlogic.collate_aptai)
        return T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic", dl, device_metrics=True, batch_invariant=cfg.batch_invariant_eval)
    four, one = run(4), run(1)
    assert model.batch_invariant is False
    assert set(four) == set(one)
    for k, v in one.items():
        if k == "val_mean_loss":                      # a mean over batches of the batch loss: one batch of 4 is not four batches of 1
            continue
        if any(k.endswith(s) for s in INT_KEYS):
            assert four[k] == v, (k, four[k], v)      # measured tolerance 0: the same predicted labels
        else:
            # the prediction tolerance through the means, plus what the fp64 means over utterances may differ by when one batch of
            # four and four batches of one associate their sums differently (the bound of tests/test_gpu_device_metrics.py)
            slack = 2 * TOL["aptai_tv_raw"] * float(model.tv_lowpass.taps().abs().sum()) + _bound(49) * max(1.0, abs(v))
            print(f"[bands] {k}: |bs4 - bs1| = {abs(four[k] - v):.2e} (bound {slack:.2e})")
            assert abs(four[k] - v) <= slack, (k, four[k], v)
    plain = T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic",
                       torch.utils.data.DataLoader(ds, batch_size=4, collate_fn=hostlogic.collate_aptai), device_metrics=True)
    assert plain["val_mean_rmse"] != one["val_mean_rmse"]                                                    # without the switch it does differ


# ------------------------------------------------------------------------------------------------ 7. refusals and no-ops
def test_gradients_and_unknown_precisions_are_refused_before_any_launch(aptai_base, data):
    w = aptai_base[0].wav2vec2
    audio = data[0][:2, :4000].contiguous().cuda()
    w.batch_invariant = True
    try:
        step = w._step
        with pytest.raises(NotImplementedError, match="waveform"):
            w(audio.clone().requires_grad_(), attention_mask=torch.tensor([[4000], [3000]]).cuda())
        prec = w._encoder_precision if hasattr(w, "_encoder_precision") else None
        w._encoder_precision = "fp8_e5m2"             # a precision whose first layer nobody taught the per-utterance statistics
        try:
            with pytest.raises(NotImplementedError, match="fp8_e5m2"):
                with torch.no_grad():
                    w(audio, attention_mask=torch.tensor([[4000], [3000]]).cuda())
        finally:
            if prec is None:
                del w._encoder_precision
            else:
                w._encoder_precision = prec
        assert w._step == step                        # refused before the forward began
    finally:
        w.batch_invariant = False


def test_training_mode_ignores_the_switch(aptai_base, data):
    model = aptai_base[0]
    audio, lens = data
    b = aptai_batch(audio, lens, ALL)
    b["phn_frames_49hz"] = torch.ones_like(b["phn_frames_49hz"])            # valid targets: a finite loss to compare
    for name in TV:
        b[name] = torch.zeros_like(b[name])
    try:
        model.train()
        outs = []
        for on in (False, True):
            model.batch_invariant = on
            model.wav2vec2._step = 100                # same dropout / SpecAugment counters (all probabilities are 0 here anyway)
            with torch.no_grad():
                outs.append(model(0, **b))
    finally:
        model.batch_invariant = False
        model.eval()
    for k in ("loss", "tvs_pred", "phn_fc_pred"):
        assert torch.equal(outs[0][k], outs[1][k]), k
