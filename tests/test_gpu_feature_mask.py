"""GPU: SpecAugment along the feature axis (mask_feature_prob; HF `_mask_hidden_states`, second half): for a row b and channel c

    h0[b, t, c] = 0 if t >= min(len[b], T), else 0 if feat[b, c], else masked_spec_embed[c] if spec[b, t], else the projection output.

Operator level (aptai_frame_feature_mask_fwd / _bwd against a torch reference on bf16 bit patterns, dembed against its fp64 sum within
n 2^-24 sum |x|), the span sampler on the feature axis against HF's span-count rule, the model with an explicit mask against a surrogate
model whose masked projection rows are zero (bit equality) and against the fp32 oracle on that surrogate (the waveform-gradient bar of
test_gpu_input_grad.py), the model with a sampled mask, the refusals, and the hipGraph-captured step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F64 = torch.bfloat16, torch.float64
EPS24 = 2.0 ** -24
NODROP = dict(hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0., final_dropout=0., layerdrop=0.)
SETTING = dict(mask_feature_prob=0.01, mask_feature_length=512, mask_feature_min_masks=1)     # one span of 512 channels per row


def _bits(x):
    return x.contiguous().view(torch.int16)


def _feature_entry_fwd(h, lens, spec, embed, feat, B, Tp, T, H):
    """aptai_frame_feature_mask_fwd: through ops.frame_mask_fwd with a feature mask, called directly with a null one (the wrapper
    launches the time-only entry then)."""
    from aptai_amd import _lib, ops
    if feat is not None:
        return ops.frame_mask_fwd(h, lens, spec, embed, B, Tp, T, H, feat_mask_u8=feat)
    _lib.call("aptai_frame_feature_mask_fwd", h.data_ptr(), lens.data_ptr(), ops._ptr(spec), ops._ptr(embed), None, B, Tp, T, H,
              ops._stream())


def _feature_entry_bwd(dy, lens, spec, feat, B, Tp, T, H):
    """aptai_frame_feature_mask_bwd with want_dembed, reached as in _feature_entry_fwd; returns dembed (None without a time mask)."""
    from aptai_amd import _lib, ops
    if feat is not None:
        return ops.frame_mask_bwd(dy, lens, spec, B, Tp, T, H, want_dembed=True, feat_mask_u8=feat)
    dembed = ws = None
    if spec is not None:
        dembed = torch.empty(H, device=dy.device, dtype=torch.float32)
        ws = ops._ws(_lib.lib().aptai_frame_mask_bwd_workspace_bytes(B, Tp, H), dy.device)
    _lib.call("aptai_frame_feature_mask_bwd", dy.data_ptr(), lens.data_ptr(), ops._ptr(spec), None, ops._ptr(dembed), ops._ptr(ws),
              B, Tp, T, H, ops._stream())
    return dembed


# ------------------------------------------------------------------------------------------------ 1. operator
@pytest.mark.parametrize("case", ["time+feature", "feature", "neither"])
@pytest.mark.parametrize("H", [768, 1024])
def test_frame_feature_mask_forward_and_backward(H, case):
    from aptai_amd import ops
    with_spec, with_feat = case == "time+feature", case != "neither"
    B, Tp, T = 5, 256, 199
    lens = [0, 1, T, 230, 120]                                            # empty, one frame, full, above T (clamped to T), ragged
    g = torch.Generator().manual_seed(H + 3 * with_spec + with_feat)
    spec = (torch.rand(B, T, generator=g) < 0.3).to(torch.uint8)
    spec[4, 120:] = 1                                                     # set on padded frames: must contribute nothing
    spec[2, 0] = spec[2, T - 1] = spec[1, 0] = 1
    feat = (torch.rand(B, H, generator=g) < 0.3).to(torch.uint8)
    feat[3] = 1                                                           # a row with every channel masked
    feat[2] = 0                                                           # a row with none, apart from the two edge channels below
    feat[:, 0] = feat[:, H - 1] = 1                                       # first and last channel, masked in every row
    embed = torch.randn(H, generator=g)
    t = torch.arange(Tp)
    valid = t[None, :] < torch.tensor(lens).clamp(max=T)[:, None]         # [B][Tp]
    masked = torch.zeros(B, Tp, dtype=torch.bool)
    if with_spec:
        masked[:, :T] = spec.bool()
    masked &= valid
    fzero = valid[:, :, None] & feat.bool()[:, None, :] if with_feat else torch.zeros(B, Tp, H, dtype=torch.bool)
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    spec_d = spec.cuda() if with_spec else None
    feat_d = feat.cuda() if with_feat else None
    embed_d = embed.cuda() if with_spec else None
    # ---- forward (in place): zeros beyond min(len, T); on valid frames 0 on masked channels, else bf16(embed) on time-masked frames,
    # else untouched
    h = torch.randn(B * Tp, H, generator=g).to(BF16)
    want = h.clone().view(B, Tp, H)
    want[masked] = embed.to(BF16)
    want[fzero] = 0
    want[~valid] = 0
    h_d = h.cuda()
    _feature_entry_fwd(h_d, lens_d, spec_d, embed_d, feat_d, B, Tp, T, H)
    torch.cuda.synchronize()
    assert torch.equal(_bits(h_d.cpu()), _bits(want.view(B * Tp, H)))
    # ---- backward (in place): dy zeroed on padded and time-masked rows and on masked channels, bit-unchanged elsewhere
    dy = torch.randn(B * Tp, H, generator=g).to(BF16)
    want = dy.clone().view(B, Tp, H)
    want[masked | ~valid] = 0
    want[fzero] = 0
    dy_d = dy.cuda()
    dembed = _feature_entry_bwd(dy_d, lens_d, spec_d, feat_d, B, Tp, T, H)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dy_d.cpu()), _bits(want.view(B * Tp, H)))
    if case == "neither":
        # today's entry points, bit for bit
        assert dembed is None
        h0, dy0 = h.cuda(), dy.cuda()
        ops.frame_mask_fwd(h0, lens_d, None, None, B, Tp, T, H)
        assert ops.frame_mask_bwd(dy0, lens_d, None, B, Tp, T, H, want_dembed=True) is None
        assert torch.equal(_bits(h0), _bits(h_d)) and torch.equal(_bits(dy0), _bits(dy_d))
        # and with a time mask but no feature mask: the shared kernel with a null feature mask, dembed included
        h0, h1, dy0, dy1 = h.cuda(), h.cuda(), dy.cuda(), dy.cuda()
        ops.frame_mask_fwd(h0, lens_d, spec.cuda(), embed.cuda(), B, Tp, T, H)
        _feature_entry_fwd(h1, lens_d, spec.cuda(), embed.cuda(), None, B, Tp, T, H)
        de0 = ops.frame_mask_bwd(dy0, lens_d, spec.cuda(), B, Tp, T, H, want_dembed=True)
        de1 = _feature_entry_bwd(dy1, lens_d, spec.cuda(), None, B, Tp, T, H)
        assert torch.equal(_bits(h0), _bits(h1)) and torch.equal(_bits(dy0), _bits(dy1))
        assert torch.equal(de0.view(torch.int32), de1.view(torch.int32))
        return
    if not with_spec:
        assert dembed is None
        return
    # dembed[c] = sum of dy over the time-masked valid rows whose channel c is not feature-masked
    rows = dy.view(B, Tp, H).to(F64) * (masked[:, :, None] & ~fzero).to(F64)
    rows = rows.view(B * Tp, H)
    n = int(masked.sum())
    assert n > 100
    err = (dembed.cpu().to(F64) - rows.sum(0)).abs()
    bound = n * EPS24 * rows.abs().sum(0)
    live = bound > 0
    assert live.sum() > H // 2
    r = (err[live] / bound[live]).max().item()
    print(f"[feature-mask] frame_feature_mask_bwd H={H}: dembed over {n} rows, max |err| / bound = {r:.4f}")
    assert r <= 1.0, r
    assert (err[~live] == 0).all()
    got = dembed.cpu()
    assert got[0].item() == 0.0 and got[H - 1].item() == 0.0            # masked in every row: exactly zero
    assert (got[feat.bool().all(0)] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. sampler on the feature axis
def _span_counts(H, p, L, min_masks):
    """The span counts HF `_compute_mask_indices` can give a row of length H: int(p H / L + eps) for the smallest and the largest
    epsilon in [0, 1), each through the min_masks and the two length clamps."""
    out = set()
    for eps in (0.0, 1.0 - 2.0 ** -24):
        n = int(p * H / L + eps)
        n = max(n, min_masks)
        if n * L > H:
            n = H // L
        if H - (L - 1) < n:
            n = max(H - (L - 1), 0)
        out.add(n)
    return sorted(out)


def _union_of_n_spans(row, L, n):
    """Is the masked set of `row` a union of exactly n spans of L consecutive channels with distinct starts?  Each maximal run of
    r masked channels needs r >= L, at least ceil(r / L) spans and at most r - L + 1."""
    idx = np.flatnonzero(row)
    if len(idx) == 0:
        return n == 0
    runs = np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1)
    r = np.array([len(x) for x in runs])
    if (r < L).any():
        return False
    return int(np.ceil(r / L).sum()) <= n <= int((r - L + 1).sum())


@pytest.mark.parametrize("p,L,min_masks", [(0.01, 512, 1), (0.25, 10, 0), (0.5, 16, 0), (0.05, 64, 2)])
@pytest.mark.parametrize("H", [768, 1024])
def test_feature_axis_sampler_follows_the_hf_rule(H, p, L, min_masks):
    from aptai_amd import ops
    from aptai_amd.wav2vec2 import _FEATURE_MASK_STREAM, _TIME_MASK_STREAM, _seed
    B = 4
    lens = torch.full((B,), H, dtype=torch.int32).cuda()
    allowed = _span_counts(H, p, L, min_masks)
    assert 1 <= len(allowed) <= 2 and allowed[-1] - allowed[0] <= 1 and allowed[-1] >= 1
    seen = set()
    masks = []
    for call in range(6):
        m = ops.spec_augment_mask(lens, B, H, p, L, min_masks, _seed(1234 + call, _FEATURE_MASK_STREAM)).cpu().numpy()
        assert m.shape == (B, H) and set(np.unique(m)) <= {0, 1}
        # one epsilon per call: the same n explains every row of the call
        fits = [n for n in allowed if all(_union_of_n_spans(m[b], L, n) for b in range(B))]
        assert fits, (call, allowed, m.sum(1))
        seen.update(fits)
        assert any((m[b] != m[0]).any() for b in range(1, B))             # rows differ from one another
        masks.append(m)
    assert seen <= set(allowed)
    assert any((masks[i] != masks[0]).any() for i in range(1, 6))        # seeds differ
    again = ops.spec_augment_mask(lens, B, H, p, L, min_masks, _seed(1234, _FEATURE_MASK_STREAM)).cpu().numpy()
    assert np.array_equal(again, masks[0])                                # the same seed gives the same mask
    other = ops.spec_augment_mask(lens, B, H, p, L, min_masks, _seed(1234, _TIME_MASK_STREAM)).cpu().numpy()
    assert _FEATURE_MASK_STREAM != _TIME_MASK_STREAM and (other != masks[0]).any()   # a stream of its own


# ------------------------------------------------------------------------------------------------ 3./4./5. model
def _pr_cfg(**kw):
    from aptai_amd.config import W2V2Config
    return W2V2Config.base(num_hidden_layers=2, vocab_size=40, apply_spec_augment=True, mask_time_prob=0.05, **NODROP, **kw)


def _inputs():
    """2 x 1 s, ragged lengths, and a time mask drawn by the host sampler over each row's valid frames."""
    from aptai_amd import hostlogic
    from oracle import synth
    from test_gpu_input_grad import _frames
    x0 = synth.synth_aptai_batch(_pr_cfg(), 2, 16000, seed=21)["audio_inputs"].clone()
    lens = torch.tensor([16000, 11111])
    x0[1, 11111:] = 0                                                    # zero padding behind the shorter utterance, as a collate pads
    fl = _frames(lens)
    T = (16000 - 400) // 320 + 1
    assert fl.min() < T                                                  # ragged
    tmask = hostlogic.compute_mask_indices((2, T), 0.05, 10, attention_mask=torch.arange(T)[None] < fl[:, None], min_masks=2,
                                           rng=np.random.RandomState(3))
    assert tmask.any()
    return x0, lens, torch.from_numpy(tmask)


def _run(w, x0, lens, tmask, R, **kw):
    """Forward + fixed random linear loss + backward: (out, last_hidden_state, waveform gradient, parameter gradients)."""
    w.zero_grad(set_to_none=True)
    x = x0.cuda().requires_grad_(True)
    out = w(x, attention_mask=lens.cuda()[:, None], mask_time_indices=tmask, **kw)
    h = out.last_hidden_state
    (h.float() * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out, h.detach().clone(), x.grad.detach().clone(), {n: p.grad.detach().clone() for n, p in w.named_parameters()
                                                             if p.grad is not None}


def test_explicit_feature_mask_equals_the_zeroed_row_surrogate():
    from oracle import synth, w2v2_ref
    from test_gpu_ctc_pr import _build_pr
    from test_gpu_input_grad import _check_grad
    cfg = _pr_cfg()
    H = cfg.hidden_size
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    x0, lens, tmask = _inputs()
    g = torch.Generator().manual_seed(5)
    frow = torch.rand(H, generator=g) < 0.3
    frow[0] = frow[H - 1] = True
    frow[300:340] = True
    assert 100 < int(frow.sum()) < H - 100
    fmask = torch.stack([frow, frow])                                     # two equal rows: one surrogate serves both
    PW, PB, EM = ("feature_projection.projection.weight", "feature_projection.projection.bias", "masked_spec_embed")
    sd2 = {k: v.clone() for k, v in sd.items()}
    for k in (PW, PB, EM):
        sd2["wav2vec2." + k][frow] = 0
    wa = _build_pr(cfg, sd).wav2vec2.train()
    wb = _build_pr(cfg, sd2).wav2vec2.train()
    T = tmask.shape[1]
    R = torch.randn(2, T, H, generator=torch.Generator().manual_seed(8))
    oa, ha, xa, ga = _run(wa, x0, lens, tmask, R, mask_feature_indices=fmask)
    ob, hb, xb, gb = _run(wb, x0, lens, tmask, R)
    assert ob._feature_mask is None
    assert oa._feature_mask.dtype == torch.uint8 and torch.equal(oa._feature_mask.cpu().bool(), fmask)
    assert torch.equal(ha, hb)
    assert torch.equal(xa, xb) and xa.abs().max() > 0
    assert set(ga) == set(gb) and {PW, PB, EM} <= set(ga) and len(ga) > 30
    bad = [n for n in ga if n not in (PW, PB, EM) and not torch.equal(ga[n], gb[n])]
    assert not bad, bad
    keep = (~frow).cuda()
    for n in (PW, PB, EM):
        assert torch.equal(ga[n][keep], gb[n][keep]), n                   # unmasked rows / entries: the surrogate's
        assert ga[n][keep].abs().max() > 0, n
        assert (ga[n][~keep] == 0).all(), n                               # masked ones: exactly zero
    assert gb[EM][~keep].abs().max() > 0                                   # where the surrogate's own are not
    # uint8 instead of bool, and eval mode: an explicit mask is applied in either mode
    wa.eval(); wb.eval()
    with torch.no_grad():
        he = wa(x0.cuda(), attention_mask=lens.cuda()[:, None], mask_time_indices=tmask,
                mask_feature_indices=fmask.to(torch.uint8).cuda()).last_hidden_state
        hs = wb(x0.cuda(), attention_mask=lens.cuda()[:, None], mask_time_indices=tmask).last_hidden_state
    assert torch.equal(he, hs)
    # the fp32 oracle on the surrogate weights
    xo = x0.clone().requires_grad_(True)
    ro = w2v2_ref.wav2vec2_forward(sd2, cfg, xo, lens, "wav2vec2.", True, tmask)
    (ro["last_hidden_state"] * R).sum().backward()
    _check_grad(xa.cpu(), xo.grad, "Wav2Vec2Model (time + feature mask) vs oracle on the surrogate")


def test_sampled_feature_mask_in_the_model():
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg_on, cfg_off = _pr_cfg(**SETTING), _pr_cfg()
    H = cfg_on.hidden_size
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg_on), 0)
    x0, lens, tmask = _inputs()
    won = _build_pr(cfg_on, sd).wav2vec2.train()
    woff = _build_pr(cfg_off, sd).wav2vec2.train()
    R = torch.randn(2, tmask.shape[1], H, generator=torch.Generator().manual_seed(8))
    won._step = 100                                                       # with base_seed this fixes the seeds of the two forwards
    masks = []
    for _ in range(2):
        out, _, _, grads = _run(won, x0, lens, tmask, R)
        m = out._feature_mask
        assert m is not None and m.dtype == torch.uint8 and tuple(m.shape) == (2, H) and m.is_cuda
        assert m[:, 256:512].all()                                        # one span of 512 starting in [0, H - 511): by construction
        assert (m.long().sum(1) == 512).all()
        gw, gb = grads["feature_projection.projection.weight"], grads["feature_projection.projection.bias"]
        assert (gw[256:512] == 0).all() and (gb[256:512] == 0).all()
        live = (~m.bool()).all(0).nonzero().flatten()                     # channels masked in no row
        assert len(live) > 0 and gw[live].abs().max() > 0 and gb[live].abs().max() > 0
        masks.append(m.cpu())
    assert (masks[0] != masks[1]).any() or (masks[0][0] != masks[0][1]).any()
    # a sampled time mask next to it (no explicit one): both are drawn, neither disturbs the other's shape
    out = won(x0.cuda(), attention_mask=lens.cuda()[:, None])
    assert (out._feature_mask.long().sum(1) == 512).all()
    # eval mode never samples: the model without the feature mask, bit for bit
    won.eval(); woff.eval()
    with torch.no_grad():
        a = won(x0.cuda(), attention_mask=lens.cuda()[:, None])
        b = woff(x0.cuda(), attention_mask=lens.cuda()[:, None])
    assert a._feature_mask is None and b._feature_mask is None
    assert torch.equal(a.last_hidden_state, b.last_hidden_state)
    # apply_spec_augment = False, train mode: the same
    won.train(); woff.train()
    won.config.apply_spec_augment = woff.config.apply_spec_augment = False
    _, ha, xa, ga = _run(won, x0, lens, None, R)
    oa = won(x0.cuda(), attention_mask=lens.cuda()[:, None])
    _, hb, xb, gb = _run(woff, x0, lens, None, R)
    assert oa._feature_mask is None
    oe = won(x0.cuda(), attention_mask=lens.cuda()[:, None], mask_feature_indices=torch.ones(2, H, dtype=torch.bool))
    assert oe._feature_mask is None and torch.equal(oe.last_hidden_state, hb)      # an explicit mask too, as mask_time_indices
    assert torch.equal(ha, hb) and torch.equal(xa, xb)
    assert set(ga) == set(gb) and all(torch.equal(ga[n], gb[n]) for n in ga)


def test_feature_mask_refusals():
    from aptai_amd import ops
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg = _pr_cfg()
    H = cfg.hidden_size
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    w = _build_pr(cfg, sd).wav2vec2.train()
    x = torch.randn(2, 16000, generator=torch.Generator().manual_seed(1)).cuda()
    step = w._step
    for shape in ((2, H - 4), (1, H), (H,), (2, 1, H)):
        with pytest.raises(ValueError, match="mask_feature_indices"):
            w(x, mask_feature_indices=torch.zeros(shape, dtype=torch.bool))
    # more spans than the sampler draws per row: refused on the host, before anything is launched
    w.config.mask_feature_prob, w.config.mask_feature_length = 0.5, 1
    with pytest.raises(ValueError, match=str(ops.SPEC_MAX_SPANS)):
        w(x)
    assert w._step == step                                                # neither refusal got as far as the step counter
    w.config.mask_feature_prob, w.config.mask_feature_length = 0.0, 10
    # the exact inference pass takes no SpecAugment mask
    w.eval()
    w.set_encoder_precision("f32x3")
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            w(x, mask_feature_indices=torch.zeros(2, H, dtype=torch.bool))
        out = w(x)
    assert out._feature_mask is None


# ------------------------------------------------------------------------------------------------ 6. graphed step
def test_graphed_step_samples_a_fresh_feature_mask_per_replay():
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedAPTAIStep
    from oracle import synth
    from test_gpu_aptai import _build

    def cfg_for(**kw):
        return W2V2Config.base(num_hidden_layers=2, vocab_size=46, apply_spec_augment=True, mask_time_prob=0.0, **NODROP, **kw)
    cfg = cfg_for(**SETTING)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 16000, seed=3).items()}
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    proj = model.wav2vec2.feature_projection.projection
    w0, b0 = proj.weight.detach().clone(), proj.bias.detach().clone()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0, fused=True)
    runner = GraphedAPTAIStep(model, opt, batch)
    assert runner.feat is not None and tuple(runner.feat.shape) == (2, cfg.hidden_size) and runner.feat.dtype == torch.uint8
    masks, losses = [], []
    for _ in range(4):
        losses.append(runner.step()["loss"].item())
        m = runner.feat.clone()
        assert m[:, 256:512].all() and (m.long().sum(1) == 512).all()
        masks.append(m.cpu())
    runner.close()
    assert len({m.numpy().tobytes() for m in masks}) >= 2                 # fresh spans on the replays
    assert all(np.isfinite(losses)), losses
    # channels 256..511 are masked in every row of every step: zero gradient from zero moments is a zero Adam update
    assert torch.equal(proj.weight.detach()[256:512], w0[256:512]) and torch.equal(proj.bias.detach()[256:512], b0[256:512])
    moved = (proj.weight.detach() != w0).any(1)
    assert not moved[256:512].any() and moved.any()
    assert (proj.bias.detach() != b0).any()
    # mask_feature_prob = 0: nothing new is captured, and the first step is the eager step
    cfg0 = cfg_for()
    sd0 = synth.make_state_dict(synth.aptai_param_shapes(cfg0), 0)        # no masked_spec_embed: both probabilities are 0
    first = {}
    for mode in ("eager", "graph"):
        model = _build(cfg0, sd0, tv_drop=0.0, phn_drop=0.0)
        model.train()
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0, fused=True)
        if mode == "eager":
            opt.zero_grad(set_to_none=True)
            out = model(0, **batch)
            out["loss"].backward()
            opt.step()
            first[mode] = out["loss"].item()
        else:
            runner = GraphedAPTAIStep(model, opt, batch)
            assert runner.feat is None and runner.feat_lens is None
            first[mode] = runner.step()["loss"].item()
            runner.close()
    assert abs(first["eager"] - first["graph"]) <= 2e-3 * abs(first["eager"]), first
