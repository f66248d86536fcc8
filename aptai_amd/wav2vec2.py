"""MI355X-native ``Wav2Vec2Model``: same module surface and state-dict keys as the HuggingFace class the
reference instantiates (models/aptai.py:33-40, models/w2v2_pr.py:28-33), computed by hand-written HIP
kernels (libaptai_hip.so) through ``aptai_amd.ops``.  No ``transformers`` import, no CPU fallback.

Layout: activations are channels-last bf16 ``[B*Tp][C]`` with ``Tp`` = frames per utterance padded to a
multiple of 128 (>= T+2); frames in [T, Tp) are treated exactly like the reference's padded frames (zeroed
before the encoder, masked as attention keys, never touched by a loss), so they cannot influence valid
frames.  Parameters stay fp32 ``nn.Parameter``s (drop-in for ``torch.optim.Adam`` and ``state_dict``); bf16
compute copies are cached per parameter version.  "HF:n" cites modeling_wav2vec2.py (transformers 5.15.0).
"""
from __future__ import annotations

import contextlib
import json
import math
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import hostlogic, ops
from .config import W2V2Config


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _rows_with_zero_slack(rows: int, C: int, dev, slack: int = 8) -> torch.Tensor:
    """[rows][C] bf16 whose last `slack` rows are zero and whose other rows are about to be written whole by a kernel: the
    overlapping-row GEMM of the next conv layer (and the dgrad accumulation of the previous one) reads a few rows past the last
    utterance, and 0 x NaN must not reach a weight gradient.  A full torch.zeros of these buffers (up to 537 MB each, ~20 per
    Wav2Vec2_PR step) cost 0.39 ms per step (rocprofv3, profiles/r03_pr_kernel_stats.csv)."""
    t = torch.empty((rows, C), device=dev, dtype=torch.bfloat16)
    t[rows - slack:].zero_()
    return t


class _Holder(nn.Module):
    """Parameter container (the arithmetic lives in the HIP kernels, not in module forwards)."""


def _linear(out_f: int, in_f: int, std: float = 0.02) -> _Holder:
    m = _Holder()
    m.weight = nn.Parameter(torch.randn(out_f, in_f) * std)
    m.bias = nn.Parameter(torch.zeros(out_f))
    return m


def _norm(c: int) -> _Holder:
    m = _Holder()
    m.weight = nn.Parameter(torch.ones(c))
    m.bias = nn.Parameter(torch.zeros(c))
    return m


class Wav2Vec2BaseModelOutput(dict):
    """Minimal stand-in for HF's ModelOutput: attribute, key and integer access (``outputs[0]``)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __getitem__(self, k):
        if isinstance(k, int):
            return [v for v in self.values() if v is not None][k]
        return dict.__getitem__(self, k)


# =================================================================================== generic autograd glue
class _OpFn(torch.autograd.Function):
    """forward(impl, x, *params): impl.fwd(x, params) -> (outputs tuple, saved); backward -> impl.bwd(saved, grads)."""

    @staticmethod
    def forward(ctx, impl, need, x, *params):
        outs, saved = impl.fwd(x, params, need)          # grad mode is off in here: `need` is decided by the caller
        ctx.impl, ctx.saved = impl, saved
        if len(outs) > 1 and getattr(impl, "want_attn", False):
            ctx.set_materialize_grads(False)             # a map no loss touches arrives as None, not as 200 MB of zeros
        return outs if len(outs) > 1 else outs[0]

    @staticmethod
    def backward(ctx, *grads):
        dx, pgrads = ctx.impl.bwd(ctx.saved, grads, ctx.needs_input_grad[2])
        ctx.saved = None
        return (None, None, dx) + tuple(pgrads)


def _run(impl, x, *params):
    need = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params if p is not None))
    return _OpFn.apply(impl, need, x, *params)


class _ConvStackFn(torch.autograd.Function):
    """Feature encoder under autograd: trainable conv stack (Wav2Vec2_PR fine-tuning, train/train_phoneme_recognizer.py) and/or a
    waveform that requires grad.  Forward saves the layer outputs / pre-activations, backward = Wav2Vec2Model._conv_backward."""

    @staticmethod
    def forward(ctx, audio, model, g, *params):
        feats, sv = model._conv_forward(audio, g, save=True)
        ctx.model, ctx.g, ctx.sv = model, g, sv
        return feats

    @staticmethod
    def backward(ctx, dfeats):
        want_audio = ctx.needs_input_grad[0]
        want_params = any(ctx.needs_input_grad[3:])
        daudio, grads = ctx.model._conv_backward(ctx.sv, ctx.g, dfeats.contiguous(), want_params=want_params, want_audio=want_audio)
        ctx.sv = None
        if not want_params:
            grads = [None] * (len(ctx.needs_input_grad) - 3)
        return (daudio, None, None) + tuple(grads)


def _seed(base: int, *ids: int) -> int:
    s = base & 0xFFFFFFFFFFFF
    for i in ids:
        s = (s * 1000003 + i + 1) & 0xFFFFFFFFFFFFFFFF
    # splitmix64 finaliser: the kernels use the two 32-bit halves as independent stream keys (csrc/common.h rng_hash)
    s = ((s ^ (s >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    s = ((s ^ (s >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return s ^ (s >> 31)


# The seed streams, as ids of _seed(parent seed, id); the values are part of every recorded run and never change.  Inside one layer
# (parent: the layer's seed), inside the front end (the front's seed), then below the step seed: the two SpecAugment masks of the device
# sampler (drawn independently of each other), layer i = base + i, and the heads of Wav2Vec2_PR, APTAI and Force_APTAI.
_ATTN_DROPOUT_STREAM, _OUT_PROJ_DROPOUT_STREAM, _ACT_DROPOUT_STREAM, _FFN2_DROPOUT_STREAM = 1, 2, 3, 4
_PROJ_DROPOUT_STREAM, _FRONT_DROPOUT_STREAM = 11, 12
_TIME_MASK_STREAM, _FEATURE_MASK_STREAM = 77, 78
_LAYER_STREAM_BASE = 100
_PR_HEAD_STREAM, _APTAI_HEADS_STREAM, _FORCE_HEADS_STREAM = 777, 999, 4242


# =================================================================================== encoder layer
class _LayerImpl:
    """One transformer layer (HF:575-654).  post-LN (base) or pre-LN (do_stable_layer_norm, large).  ``mx``: MXFP8 weight copies (the
    inference-only _fwd_mxfp8); ``want_attn`` (output_attentions): fwd returns the layer's attention map as a second output;
    ``attn_state``: shared by the layers of one forward call (.seen = a layer above got a gradient on its map)."""

    def __init__(self, cfg: W2V2Config, geom, lens_i32, w, training: bool, seed: int, *, mx=None, want_attn=False, attn_state=None):
        self.cfg, self.g, self.lens, self.w, self.training, self.seed = cfg, geom, lens_i32, w, training, seed
        self.mx, self.want_attn, self.attn_state = mx, want_attn, attn_state

    # params: ln1.w ln1.b ln2.w ln2.b, then the 12 fp32 linear parameters (q,k,v weights; q,k,v biases; out w,b;
    # ffn1 w,b; ffn2 w,b).  The forward reads their cached bf16 copies in `w`; the backward returns their gradients.
    def fwd(self, x, params, need):
        cfg, g, w = self.cfg, self.g, self.w
        M, H, I = g.M, cfg.hidden_size, cfg.intermediate_size
        ln1w, ln1b, ln2w, ln2b = params[0], params[1], params[2], params[3]
        tr = self.training
        p_h = cfg.hidden_dropout if tr else 0.0
        p_a = cfg.activation_dropout if tr else 0.0
        p_att = cfg.attention_dropout if tr else 0.0
        s = SimpleNamespace(x=x)
        pre = cfg.do_stable_layer_norm
        if self.mx is not None and not need:
            return self._fwd_mxfp8(x, params, self.mx)
        if pre:
            n1, s.m1, s.r1 = ops.layernorm_fwd(x, ln1w, ln1b, cfg.layer_norm_eps, save_stats=need)
            attn_in = n1
            s.n1 = n1
        else:
            attn_in = x
        # the projection's epilogue hands Q over as q * head_dim^-0.5 * log2(e) (rounded once): the attention kernels then see
        # their exp2 arguments directly (q_prescaled)
        s.qkv = ops.gemm(attn_in, w.wqkv, M, 3 * H, H, bias=w.bqkv, colscale=(H, ops.attention_qscale(H, cfg.num_attention_heads)))
        s.ctx, s.lse = ops.attention_fwd(s.qkv, self.lens, g.B, g.Tp, H, cfg.num_attention_heads, q_prescaled=True, dropout_p=p_att,
                                         seed=_seed(self.seed, _ATTN_DROPOUT_STREAM), save_lse=need or self.want_attn)
        probs = None
        if self.want_attn:          # HF eager attention's second result: the softmax after dropout, with the fused kernel's own mask
            probs = ops.attention_probs_fwd(s.qkv, self.lens, s.lse[0], g.B, g.Tp, H, cfg.num_attention_heads, q_prescaled=True,
                                            dropout_p=p_att, seed=_seed(self.seed, _ATTN_DROPOUT_STREAM))
        s.s1 = ops.gemm(s.ctx, w.wo, M, H, H, bias=w.bo, residual=x, dropout_p=p_h, seed=_seed(self.seed, _OUT_PROJ_DROPOUT_STREAM))
        if pre:
            ffn_in, s.m2, s.r2 = ops.layernorm_fwd(s.s1, ln2w, ln2b, cfg.layer_norm_eps, save_stats=need)
            s.n2 = ffn_in
        else:
            ffn_in, s.m1, s.r1 = ops.layernorm_fwd(s.s1, ln1w, ln1b, cfg.layer_norm_eps, save_stats=need)
            s.x1 = ffn_in
        s.u = torch.empty((M, I), device=x.device, dtype=torch.bfloat16) if need else None
        # with gradients: s.u holds dropmask/(1-p) * gelu'(pre-activation), the factor the dgrad epilogue multiplies by
        s.hact = ops.gemm(ffn_in, w.w1, M, I, H, bias=w.b1, gelu=True, out_pre=s.u, pre_dgelu=need, dropout_p=p_a,
                          seed=_seed(self.seed, _ACT_DROPOUT_STREAM))
        res2 = s.s1 if pre else ffn_in
        s.s2 = ops.gemm(s.hact, w.w2, M, H, I, bias=w.b2, residual=res2, dropout_p=p_h, seed=_seed(self.seed, _FFN2_DROPOUT_STREAM))
        if pre:
            y = s.s2
        else:
            y, s.m2, s.r2 = ops.layernorm_fwd(s.s2, ln2w, ln2b, cfg.layer_norm_eps, save_stats=need)
        s.p = (p_h, p_a, p_att)
        s.ln = (ln1w, ln1b, ln2w, ln2b)
        return ((y,) if probs is None else (y, probs)), (s if need else None)

    def fwd_f32res(self, x, x32, params):
        """Inference only, opt-in (set_encoder_precision("bf16_f32res")): the residual stream stays in fp32 - out-proj and FFN2 write
        fp32 and add the fp32 residual in their epilogues, LayerNorm reads fp32 and hands the next GEMM a bf16 copy and the next residual
        add an fp32 one.  GEMM operands and attention stay bf16.  Returns (y_bf16 | None for pre-LN, y_f32, attention map | None)."""
        cfg, g, w = self.cfg, self.g, self.w
        M, H, I = g.M, cfg.hidden_size, cfg.intermediate_size
        ln1w, ln1b, ln2w, ln2b = params[:4]
        heads, eps, pre = cfg.num_attention_heads, cfg.layer_norm_eps, cfg.do_stable_layer_norm
        attn_in = ops.layernorm_fwd_f32in(x32, ln1w, ln1b, eps, want_f32=False)[0] if pre else x
        qkv = ops.gemm(attn_in, w.wqkv, M, 3 * H, H, bias=w.bqkv, colscale=(H, ops.attention_qscale(H, heads)))
        ctx, st = ops.attention_fwd(qkv, self.lens, g.B, g.Tp, H, heads, save_lse=self.want_attn, q_prescaled=True)
        probs = ops.attention_probs_fwd(qkv, self.lens, st[0], g.B, g.Tp, H, heads, q_prescaled=True) if self.want_attn else None
        s1 = ops.gemm(ctx, w.wo, M, H, H, bias=w.bo, out_f32=True, residual_f32=x32, tile=128)
        if pre:             # FFN2 adds the un-normalised s1
            ffn_in, res2 = ops.layernorm_fwd_f32in(s1, ln2w, ln2b, eps, want_f32=False)[0], s1
        else:               # post-LN: FFN2 adds the normalised rows
            ffn_in, res2 = ops.layernorm_fwd_f32in(s1, ln1w, ln1b, eps)
        u = ops.gemm(ffn_in, w.w1, M, I, H, bias=w.b1, gelu=True)
        s2 = ops.gemm(u, w.w2, M, H, I, bias=w.b2, out_f32=True, residual_f32=res2, tile=128)
        if pre:
            return None, s2, probs
        y, y32 = ops.layernorm_fwd_f32in(s2, ln2w, ln2b, eps)
        return y, y32, probs

    def _fwd_mxfp8(self, x, params, mx):
        """Inference-only forward with MX block-scaled FP8 operands in the Linear layers where they pay (BASELINE configs[4];
        csrc/mxgemm.hip): q|k|v, FFN1 and FFN2.  Their inputs are quantised on the fly (E4M3 elements, E8M0 scale per 32 k; FFN1 hands its
        GELU output to FFN2 as MXFP8 straight from the GEMM epilogue), the frozen weights were quantised once.  The attention output
        projection stays bf16: at [rows] x 768 x 768 the quantiser's launch costs more than the fp8 product saves (tools/mx_bench.py).
        LayerNorm, attention, biases, residual stream and accumulation are as in the bf16 path."""
        cfg, g, w = self.cfg, self.g, self.w
        M, H, I = g.M, cfg.hidden_size, cfg.intermediate_size
        ln1w, ln1b, ln2w, ln2b = params[0], params[1], params[2], params[3]
        pre = cfg.do_stable_layer_norm
        if pre:             # the normalised rows feed the q|k|v GEMM only: they leave the LayerNorm kernel as MXFP8
            _, aq, a_s = ops.layernorm_fwd_mx(x, ln1w, ln1b, cfg.layer_norm_eps)
        else:
            aq, a_s = ops.mx_quantize(x)
        qkv = ops.gemm_mxfp8(aq, a_s, mx.wqkv[0], mx.wqkv[1], M, 3 * H, H, bias=w.bqkv)
        ctx, _ = ops.attention_fwd(qkv, self.lens, g.B, g.Tp, H, cfg.num_attention_heads, save_lse=False)
        s1 = ops.gemm(ctx, w.wo, M, H, H, bias=w.bo, residual=x)
        if pre:             # FFN1's input only
            ffn_in, fq, f_s = ops.layernorm_fwd_mx(s1, ln2w, ln2b, cfg.layer_norm_eps)
        else:               # post-LN: also the residual of FFN2
            ffn_in, fq, f_s = ops.layernorm_fwd_mx(s1, ln1w, ln1b, cfg.layer_norm_eps, want_bf16=True)
        hq, h_s = ops.gemm_mxfp8_mxout(fq, f_s, mx.w1[0], mx.w1[1], M, I, H, bias=w.b1, gelu=True)
        s2 = ops.gemm_mxfp8(hq, h_s, mx.w2[0], mx.w2[1], M, H, I, bias=w.b2, residual=s1 if pre else ffn_in)
        y = s2 if pre else ops.layernorm_fwd(s2, ln2w, ln2b, cfg.layer_norm_eps, save_stats=False)[0]
        return (y,), None

    def bwd(self, s, grads, x_needs):
        """The dgrad chain, then every weight and bias gradient of the layer in one grouped launch."""
        cfg, g, w = self.cfg, self.g, self.w
        M, H, I = g.M, cfg.hidden_size, cfg.intermediate_size
        heads = cfg.num_attention_heads
        p_h, p_a, p_att = s.p
        ln1w, ln1b, ln2w, ln2b = s.ln
        dprobs = grads[1] if len(grads) > 1 else None          # gradient of a loss on the attention map (output_attentions)
        # (a loss that reaches this layer through its map alone leaves the hidden state's gradient undefined: zero)
        dy = grads[0].contiguous() if grads[0] is not None else torch.zeros_like(s.x)
        pre = cfg.do_stable_layer_norm
        # ---- FFN block
        if pre:
            ds2 = dy                                             # y = s1 + D(ffn)
            d_ffn_out = ops.dropout(ds2, p_h, _seed(self.seed, _FFN2_DROPOUT_STREAM)) if p_h > 0 else ds2
            ffn_in = s.n2
        else:
            ds2, d_ffn_out, dg2, db2 = ops.layernorm_bwd(dy, s.s2, s.m2, s.r2, ln2w, dropout_p=p_h, seed=_seed(self.seed, _FFN2_DROPOUT_STREAM))
            if d_ffn_out is None:
                d_ffn_out = ds2
            ffn_in = s.x1
        du = ops.gemm(d_ffn_out, w.w2, M, I, H, b_kmajor=True, mul_aux=s.u)
        if pre:
            dn2 = ops.gemm(du, w.w1, M, H, I, b_kmajor=True)
            ds1, d_att_out, dg2, db2 = ops.layernorm_bwd(dn2, s.s1, s.m2, s.r2, ln2w, dres=ds2, dropout_p=p_h,
                                                         seed=_seed(self.seed, _OUT_PROJ_DROPOUT_STREAM))
        else:
            dx1 = ops.gemm(du, w.w1, M, H, I, b_kmajor=True, residual=ds2)
            ds1, d_att_out, dg1, db1 = ops.layernorm_bwd(dx1, s.s1, s.m1, s.r1, ln1w, dropout_p=p_h,
                                                         seed=_seed(self.seed, _OUT_PROJ_DROPOUT_STREAM))
        if d_att_out is None:
            d_att_out = ds1
        # ---- attention block
        dctx = ops.gemm(d_att_out, w.wo, M, H, H, b_kmajor=True)
        # no loss term of the models touches padded frames, so their context gradient is exactly zero and the kernel skips them - unless
        # a layer above had a gradient on its map: the maps' padded QUERY rows are part of the returned tensor (as in the reference), and
        # what a loss puts on them reaches the padded frames of every layer below
        st = self.attn_state
        dqkv = ops.attention_bwd(s.qkv, self.lens, s.ctx, dctx, s.lse, g.B, g.Tp, H, heads, q_prescaled=True, dropout_p=p_att,
                                 seed=_seed(self.seed, _ATTN_DROPOUT_STREAM), dctx_zero_beyond_len=st is None or not st.seen)
        if dprobs is not None:      # dQ and dK of the map's gradient, summed into what the fused backward wrote
            ops.attention_probs_bwd(s.qkv, self.lens, s.lse[0], dprobs.contiguous(), g.B, g.Tp, H, heads, q_prescaled=True,
                                    dropout_p=p_att, seed=_seed(self.seed, _ATTN_DROPOUT_STREAM), dqkv=dqkv)
            if st is not None:
                st.seen = True
        attn_in = s.n1 if pre else s.x
        if pre:
            dn1 = ops.gemm(dqkv, w.wqkv, M, H, 3 * H, b_kmajor=True)
            dx, _, dg1, db1 = ops.layernorm_bwd(dn1, s.x, s.m1, s.r1, ln1w, dres=ds1)
        else:
            dx = ops.gemm(dqkv, w.wqkv, M, H, 3 * H, b_kmajor=True, residual=ds1)
        # all weight and bias gradients of the layer in ONE launch (aptai_gemm_bf16_grouped_rowsum): 4 x (dY^T X), each with the row sums
        # of its dY = the bias gradient, formed by the tiles of the first tile column from the dY fragments they hold anyway:
        # 432 full-K tiles for wav2vec2-base inside one round of the 512 block slots, no split-K slabs, no reduce kernels, no ones problems
        tn = dict(a_kmajor=True, b_kmajor=True, out_f32=True, rowsum=True)
        dw2, dw1, dwo, dwqkv, dbias2, dbias1, dbo, dbqkv = ops.gemm_grouped([
            (d_ffn_out, s.hact, H, I, M, tn), (du, ffn_in, I, H, M, tn), (d_att_out, s.ctx, H, H, M, tn),
            (dqkv, attn_in, 3 * H, H, M, tn)])
        return dx, (dg1, db1, dg2, db2, dwqkv[0:H], dwqkv[H:2 * H], dwqkv[2 * H:3 * H], dbqkv[0:H], dbqkv[H:2 * H],
                    dbqkv[2 * H:3 * H], dwo, dbo, dw1, dbias1, dw2, dbias2)


_SPEC_ON_DEVICE = os.environ.get("APTAI_SPEC_ON_DEVICE", "1") != "0"      # =0: numpy sampler with HF's RNG order (host round trip)

def _host_spec_masks(cfg, B, T, frame_lens, want_time, want_feat):
    """The numpy sampler path (_SPEC_ON_DEVICE off): the time mask [B][T] over each row's valid frames (`frame_lens`, a host tensor, or
    None for full rows), then the feature mask [B][H] with every row of length H - HF's order in `_mask_hidden_states`, so one
    `np.random.seed` gives the reference's two masks.  Returns (time or None, feature or None), bool arrays."""
    m_time = m_feat = None
    if want_time:
        am = None if frame_lens is None else (torch.arange(T)[None, :] < frame_lens[:, None])
        m_time = hostlogic.compute_mask_indices((B, T), cfg.mask_time_prob, cfg.mask_time_length, attention_mask=am,
                                                min_masks=cfg.mask_time_min_masks)
    if want_feat:
        m_feat = hostlogic.compute_mask_indices((B, cfg.hidden_size), cfg.mask_feature_prob, cfg.mask_feature_length,
                                                min_masks=cfg.mask_feature_min_masks)
    return m_time, m_feat


# =================================================================================== front end of the encoder
# The front end's parameters (Wav2Vec2Model._front_params), in the order _FrontImpl.bwd returns their gradients.  embed: masked_spec_embed
# or None; pc_gain, pc_v: original0 / original1 of the positional conv's weight norm; enc_ln_*: encoder.layer_norm (post-LN models only)
_FrontParams = namedtuple("_FrontParams", "fp_ln_w fp_ln_b proj_w proj_b embed pc_gain pc_v pc_bias enc_ln_w enc_ln_b")


class _FrontImpl:
    """Feature projection (HF:422-434) -> SpecAugment fill + padded-frame zeroing (HF:1292-1295, 678-681) ->
    h + GELU(grouped positional conv(h)) (HF:326-379, 689-692) -> [LayerNorm for post-LN models] -> dropout.
    ``feat`` is the SpecAugment mask along the hidden axis ([B][H] uint8, HF `_mask_hidden_states`: `mask_feature_prob`), applied
    in the same pass as the time fill; None launches the kernels of the time-only path.  ``params`` of fwd: a _FrontParams."""

    def __init__(self, cfg, geom, lens_i32, spec, training, seed, model, feat=None):
        self.cfg, self.g, self.lens, self.spec, self.training, self.seed, self.model = cfg, geom, lens_i32, spec, training, seed, model
        self.feat = feat

    def _packed(self, key, dev):
        cfg, g = self.cfg, self.g
        Cg = cfg.hidden_size // cfg.num_conv_pos_embedding_groups
        pad = cfg.num_conv_pos_embeddings // 2
        rows_p = g.Tp + 2 * pad
        n = cfg.num_conv_pos_embedding_groups * g.B * rows_p * Cg + Cg * 8
        buf = self.model._scratch(key, n, dev)
        return buf, rows_p, Cg, pad

    def _posconv_batch(self, Cg, rows_p, K, a_off=0):
        cfg, g = self.cfg, self.g
        G = cfg.num_conv_pos_embedding_groups
        H = cfg.hidden_size
        return dict(outer=g.B, inner=G, a=(rows_p * Cg, g.B * rows_p * Cg), b=(0, Cg * K), c=(g.Tp * H, Cg),
                    bias=(0, Cg), res=(g.Tp * H, Cg), aux=(g.Tp * H, Cg))

    def fwd(self, feats, params, need):
        cfg, g = self.cfg, self.g
        p = _FrontParams(*params)
        M, H, C = g.M, cfg.hidden_size, feats.shape[1]
        tr = self.training
        s = SimpleNamespace(feats=feats, params=p)
        s.n0, s.m0, s.r0 = ops.layernorm_fwd(feats, p.fp_ln_w, p.fp_ln_b, cfg.layer_norm_eps, save_stats=need)
        s.p_fp = cfg.feat_proj_dropout if tr else 0.0
        h0 = ops.gemm(s.n0, self.model._proj_weight(), M, H, C, bias=p.proj_b, dropout_p=s.p_fp,
                      seed=_seed(self.seed, _PROJ_DROPOUT_STREAM))
        ops.frame_mask_fwd(h0, self.lens, self.spec, p.embed, g.B, g.Tp, g.T, H, feat_mask_u8=self.feat)
        s.h0 = h0
        # positional conv as ONE batched implicit GEMM over (utterance, group) on a zero-gapped group-major copy
        G, Kw = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
        xg, rows_p, Cg, pad = self._packed("pc_x", feats.device)
        ops.posconv_pack(h0, xg, g.B, g.Tp, H, G, pad)
        s.wf, s.wd, s.norm = self.model._posconv_weights()
        K = Kw * Cg
        s.u = torch.empty((M, H), device=feats.device, dtype=torch.bfloat16) if need else None
        s.s = torch.empty((M, H), device=feats.device, dtype=torch.bfloat16)
        if ops.posconv_kernel_fits(H, G, Kw):            # wav2vec2-base: dedicated Toeplitz-window kernel (csrc/posconv.hip)
            ops.posconv_gemm(xg, s.wf, s.s, g.B, g.Tp, H, G, Kw, pad, bias=p.pc_bias, gelu=True, residual=h0, out_pre=s.u)
        else:
            ops.gemm(xg, s.wf, g.Tp, Cg, K, lda=Cg, ldb=K, out=s.s, ldc=H, bias=p.pc_bias, gelu=True, residual=h0, ldr=H, out_pre=s.u,
                     batch=self._posconv_batch(Cg, rows_p, K))
        s.xg_key = "pc_x"
        self.model._scratch_owner["pc_x"] = s
        if cfg.do_stable_layer_norm:
            y = s.s
        else:
            y, s.m1, s.r1 = ops.layernorm_fwd(s.s, p.enc_ln_w, p.enc_ln_b, cfg.layer_norm_eps, save_stats=need)
        s.p_h = cfg.hidden_dropout if tr else 0.0
        if s.p_h > 0:
            y = ops.dropout(y, s.p_h, _seed(self.seed, _FRONT_DROPOUT_STREAM))
        return (y,), (s if need else None)

    def bwd(self, s, grads, x_needs):
        cfg, g = self.cfg, self.g
        p = s.params
        M, H, C = g.M, cfg.hidden_size, s.feats.shape[1]
        G, Kw = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
        dy = grads[0].contiguous()
        if s.p_h > 0:
            dy = ops.dropout(dy, s.p_h, _seed(self.seed, _FRONT_DROPOUT_STREAM))
        delw = delb = None
        if cfg.do_stable_layer_norm:
            ds = dy
        else:
            ds, _, delw, delb = ops.layernorm_bwd(dy, s.s, s.m1, s.r1, p.enc_ln_w)
        # ---- positional conv backward
        dug, rows_p, Cg, pad = self._packed("pc_du", dy.device)
        K = Kw * Cg
        du_rm = torch.empty((M, H), device=dy.device, dtype=torch.bfloat16)
        ops.posconv_pack(ds, dug, g.B, g.Tp, H, G, pad, u=s.u, rowmajor_out=du_rm)
        dpcb = ops.colsum(du_rm, M, H)
        dh0 = torch.empty((M, H), device=dy.device, dtype=torch.bfloat16)
        if ops.posconv_kernel_fits(H, G, Kw):
            ops.posconv_gemm(dug, s.wd, dh0, g.B, g.Tp, H, G, Kw, pad, first_row=1, residual=ds)
        else:
            ops.gemm(dug[Cg:], s.wd, g.Tp, Cg, K, lda=Cg, ldb=K, out=dh0, ldc=H, residual=ds, ldr=H,
                     batch=self._posconv_batch(Cg, rows_p, K))
        xg, _, _, _ = self._packed(s.xg_key, dy.device)
        if self.model._scratch_owner.get(s.xg_key) is not s:
            ops.posconv_pack(s.h0, xg, g.B, g.Tp, H, G, pad)         # another forward reused the scratch: repack
        kred = g.B * rows_p - 2 * pad
        dwf = torch.empty((G, Cg, K), device=dy.device, dtype=torch.float32)
        if ops.posconv_kernel_fits(H, G, Kw, wgrad=True):
            ops.posconv_wgrad(dug, xg, dwf, g.B, g.Tp, H, G, Kw, pad)
        else:
            ops.gemm(dug[pad * Cg:], xg, Cg, K, kred, a_kmajor=True, b_kmajor=True, out_f32=True, lda=Cg, ldb=Cg, out=dwf, ldc=K,
                     batch=dict(outer=1, inner=G, a=(0, g.B * rows_p * Cg), b=(0, g.B * rows_p * Cg), c=(0, Cg * K)))
        # weight-norm backward (parameter-sized fp32 math): w = g * v / ||v||
        dpcv, dgain = ops.posconv_weight_bwd(dwf, p.pc_v.detach().contiguous(), p.pc_gain.detach().reshape(-1).contiguous(), s.norm, G)
        dpcg = dgain.reshape(p.pc_gain.shape)
        # ---- mask + projection + LN
        dembed = ops.frame_mask_bwd(dh0, self.lens, self.spec, g.B, g.Tp, g.T, H, want_dembed=p.embed is not None,
                                    feat_mask_u8=self.feat)
        if s.p_fp > 0:
            dh0 = ops.dropout(dh0, s.p_fp, _seed(self.seed, _PROJ_DROPOUT_STREAM))
        sk = max(1, min(8, M // 2048))
        dpw = ops.gemm(dh0, s.n0, H, C, M, a_kmajor=True, b_kmajor=True, out_f32=True, split_k=sk)
        dpb = ops.colsum(dh0, M, H)
        dn0 = ops.gemm(dh0, self.model._proj_weight(), M, C, H, b_kmajor=True)
        dfeats, _, dfplw, dfplb = ops.layernorm_bwd(dn0, s.feats, s.m0, s.r0, p.fp_ln_w)
        return (dfeats if x_needs else None), (dfplw, dfplb, dpw, dpb, dembed, dpcg, dpcv, dpcb, delw, delb)


class _FinalLNImpl:
    """encoder.layer_norm after the last layer of pre-LN models (HF:791)."""

    def __init__(self, cfg, geom):
        self.cfg, self.g = cfg, geom

    def fwd(self, x, params, need):
        y, m, r = ops.layernorm_fwd(x, params[0], params[1], self.cfg.layer_norm_eps, save_stats=need)
        return (y,), (SimpleNamespace(x=x, m=m, r=r, w=params[0]) if need else None)

    def bwd(self, s, grads, x_needs):
        dx, _, dg, db = ops.layernorm_bwd(grads[0].contiguous(), s.x, s.m, s.r, s.w)
        return dx, (dg, db)


# =================================================================================== the model
# encoder precisions whose first conv layer reads the statistics block of aptai_conv0_fwd(_lens): all five that exist
_BATCH_INVARIANT_PRECISIONS = ("bf16", "bf16_f32res", "f32x3", "f32x6", "mxfp8")


@contextlib.contextmanager
def batch_invariant_scope(encoder, on: bool):
    """Sets ``encoder.batch_invariant`` for the duration of one call of a model built on it and puts the old value back."""
    prev = encoder.batch_invariant
    encoder.batch_invariant = bool(on)
    try:
        yield
    finally:
        encoder.batch_invariant = prev


def _copies_stale(mode, training, any_trainable, version_equal, synced=False, after_training=False) -> bool:
    """Must a compute copy be rebuilt from its fp32 parameters?  The one rule behind Wav2Vec2Model._cached and _refresh_layer_copies.
    ``mode`` is the model's _cache_mode (graph capture): "frozen" = never (replayed steps read the copies without asking), "build" =
    always.  Otherwise Tensor._version (``version_equal``: the key of _versions is the one the copy was built from) is trusted only
    where no optimiser can have stepped unseen: those with kernels of their own (torch's fused Adam, aptai_amd.optim.Adam) update
    parameters in place WITHOUT bumping it.  So a training-mode forward rebuilds the copies of trainable parameters every time, and so
    does the first eval forward after one (``after_training``) - unless the optimiser writes the copies itself (``synced``)."""
    if mode in ("frozen", "build"):
        return mode == "build"
    return bool(((training and any_trainable) or after_training) and not synced or not version_equal)


class Wav2Vec2Model(nn.Module):
    """Drop-in for ``transformers.Wav2Vec2Model`` on the reference's call pattern."""

    # Opt-in, eval-mode forwards only (every encoder precision): what a row returns on its valid frames depends on that utterance's
    # samples, its length and the weights alone - not on the batch size, the padded length, the other rows or the padding samples.
    # wav2vec2-base takes its first layer's GroupNorm statistics over the row's own frames (aptai_conv0_fwd_lens) instead of the
    # collated length (HF:317-323 on a padded batch), so at batch > 1 it deliberately differs from the reference and equals the
    # reference's batch-1 result.  Train-mode forwards ignore it; gradients through it are refused.
    batch_invariant = False

    _encoder_precision = "bf16"     # set_encoder_precision
    _cache_mode = None              # graph capture: "build" = every compute copy is rebuilt, "frozen" = every copy hits (_copies_stale)
    _train_marker = 0               # training steps of this model so far: part of the eval-mode version key (_versions)
    _lplan = _feat_lens = None      # _layer_plan, _feature_axis_lens

    def __init__(self, config):
        super().__init__()
        cfg = W2V2Config.from_any(config)
        self.config = cfg
        H, I = cfg.hidden_size, cfg.intermediate_size
        if cfg.head_dim != 64:
            raise ValueError("the attention kernels are built for head_dim 64 (wav2vec2 base/large)")
        if any(c != 512 for c in cfg.conv_dim) or cfg.conv_kernel[0] != 10 or cfg.conv_stride[0] != 5:
            raise ValueError("the feature-encoder kernels are built for conv_dim=512, first layer k=10/s=5")
        # ---- feature encoder (HF:382-419)
        fe = _Holder()
        layers = []
        cin = 1
        for i, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
            l = _Holder()
            l.conv = _Holder()
            w = torch.empty(c, cin, k)
            nn.init.kaiming_normal_(w)
            l.conv.weight = nn.Parameter(w)
            if cfg.conv_bias:
                bound = math.sqrt(1.0 / (cin * k))
                l.conv.bias = nn.Parameter(torch.empty(c).uniform_(-bound, bound))
            if cfg.feat_extract_norm == "layer" or i == 0:
                l.layer_norm = _norm(c)
            layers.append(l)
            cin = c
        fe.conv_layers = nn.ModuleList(layers)
        self.feature_extractor = fe
        self._fe_requires_grad = True
        # ---- feature projection (HF:422-434)
        fp = _Holder()
        fp.layer_norm = _norm(cin)
        fp.projection = _linear(H, cin)
        self.feature_projection = fp
        if cfg.mask_time_prob > 0.0 or cfg.mask_feature_prob > 0.0:
            self.masked_spec_embed = nn.Parameter(torch.empty(H).uniform_())
        # ---- encoder (HF:657-802)
        enc = _Holder()
        pc = _Holder()
        pc.conv = _Holder()
        k, grp = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
        pc.conv.bias = nn.Parameter(torch.zeros(H))
        pc.conv.parametrizations = _Holder()
        pc.conv.parametrizations.weight = _Holder()
        v = torch.randn(H, H // grp, k) * (2 * math.sqrt(1 / (k * H)))
        pc.conv.parametrizations.weight.original0 = nn.Parameter(v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
        pc.conv.parametrizations.weight.original1 = nn.Parameter(v)
        enc.pos_conv_embed = pc
        enc.layer_norm = _norm(H)
        ls = []
        for _ in range(cfg.num_hidden_layers):
            l = _Holder()
            l.attention = _Holder()
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                setattr(l.attention, n, _linear(H, H))
            l.layer_norm = _norm(H)
            l.feed_forward = _Holder()
            l.feed_forward.intermediate_dense = _linear(I, H)
            l.feed_forward.output_dense = _linear(H, I)
            l.final_layer_norm = _norm(H)
            ls.append(l)
        enc.layers = nn.ModuleList(ls)
        self.encoder = enc
        self._cache = {}
        self._scratch_pool = ops.ScratchPool()
        self._scratch_owner = {}
        self._step = 0
        self.base_seed = 0x5EED
        # LayerDrop coins come from a dedicated generator so that data-parallel ranks (same seed) drop the same layers
        self._layerdrop_gen = torch.Generator().manual_seed(0x1A7E)

    # ------------------------------------------------------------------ reference-facing helpers
    @classmethod
    def from_pretrained(cls, model_id_or_path, config=None, cache_dir=None, **kw):
        """Loads a LOCAL HuggingFace checkpoint directory (config.json + model.safetensors | pytorch_model.bin).
        Hub names cannot be resolved offline and raise."""
        path = str(model_id_or_path)
        if not os.path.isdir(path):
            raise FileNotFoundError(
                f"{path!r} is not a local checkpoint directory; hub downloads are not available to this build")
        cfg = W2V2Config.from_any(config) if config is not None else W2V2Config.from_pretrained_dir(path)
        model = cls(cfg)
        sd = None
        st = os.path.join(path, "model.safetensors")
        pb = os.path.join(path, "pytorch_model.bin")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        elif os.path.exists(pb):
            sd = torch.load(pb, map_location="cpu", weights_only=True)
        if sd is None:
            raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {path}")
        sd = {(k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k): v for k, v in sd.items()}
        own = model.state_dict()
        # legacy weight-norm names (weight_g / weight_v) -> parametrizations
        ren = {"encoder.pos_conv_embed.conv.weight_g": "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
               "encoder.pos_conv_embed.conv.weight_v": "encoder.pos_conv_embed.conv.parametrizations.weight.original1"}
        sd = {ren.get(k, k): v for k, v in sd.items()}
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError(f"checkpoint {path} lacks {len(missing)} tensors, e.g. {missing[:3]}")
        model.load_state_dict({k: sd[k] for k in own})
        return model

    def save_pretrained(self, path):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config.to_dict(), f, indent=1)
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(path, "model.safetensors"))

    def set_encoder_precision(self, precision: str = "bf16"):
        """"bf16" (default) or "mxfp8": the latter runs the Linear layers of the transformer stack with OCP MXFP8 operands on the
        block-scaled matrix instruction - INFERENCE ONLY (eval mode, no gradients: the frozen recogniser inside Force_APTAI,
        BASELINE configs[4]); any forward that needs gradients keeps the bf16 kernels."""
        # "bf16_f32res": bf16 GEMM operands and attention, but the RESIDUAL STREAM of the transformer stack in fp32 (LayerNorm reads
        # fp32, out-proj / FFN2 add the fp32 residual in their epilogues) and an fp32 last hidden state for the heads - inference
        # only; shrinks the bf16 noise band of the integer outputs downstream (forced-alignment indices) at ~+10 % encoder time
        # "f32x3" / "f32x6": every matrix product of the encoder (conv stack, projection, the four Linear layers, attention, positional
        # conv) at fp32-class accuracy - bf16 split-operand products with fp32 accumulation on the bf16 matrix pipe (3 or 6 bf16 x bf16
        # products per fp32 product, csrc/exact.hip) and the fp32 matrix instruction for attention / positional conv - with fp32
        # LayerNorm, softmax and erf GELU in between: INFERENCE ONLY, ~3-6 x the bf16 encoder time.  For outputs that must equal the
        # reference's INDEX for index (Force_APTAI's alignment argmax, the best-path decode).
        if precision not in ("bf16", "mxfp8", "bf16_f32res", "f32x3", "f32x6"):
            raise ValueError("encoder precision must be 'bf16', 'mxfp8', 'bf16_f32res', 'f32x3' or 'f32x6'")
        self._encoder_precision = precision
        return self

    encoder_precision = property(lambda self: self._encoder_precision)      # read-only, for the other modules

    def _mx_layer_weights(self, i: int):
        """MXFP8 copies (elements, scales) of layer i's four weight matrices, quantised from the bf16 compute copies; rebuilt only
        when the parameters moved (eval mode trusts Tensor._version, see _cached)."""
        e = self._layer_plan().entries[i]

        def build():
            return SimpleNamespace(wqkv=ops.mx_quantize(e.wqkv), wo=ops.mx_quantize(e.wo), w1=ops.mx_quantize(e.w1),
                                   w2=ops.mx_quantize(e.w2))
        return self._cached(("mx", i), self._layer_params(i), build)

    def gradient_checkpointing_enable(self, *a, **kw):
        """Accepted for drop-in compatibility (models/aptai.py:38): 288 GB of HBM make recomputation unnecessary."""
        return None

    def freeze_feature_encoder(self):
        """HF:1265-1270."""
        for p in self.feature_extractor.parameters():
            p.requires_grad = False
        self._fe_requires_grad = False

    def _get_feat_extract_output_lengths(self, input_lengths, add_adapter=None):
        return hostlogic.feat_extract_output_lengths(input_lengths, self.config.conv_kernel, self.config.conv_stride)

    # ------------------------------------------------------------------ bf16 compute copies of the parameters
    def _versions(self, params):
        # `_train_marker` counts training steps of this model (training-mode forwards under autograd, replayed graph steps, weights_moved),
        # so a copy built in eval mode is rebuilt by the first eval forward after any: validation sees the LAST update (_copies_stale)
        return (0 if self.training else self._train_marker,) + tuple((p.data_ptr(), p._version) for p in params)

    def _cached(self, key, params, build):
        """The compute copy `key` of `params`, rebuilt by `build` when _copies_stale says so (the layers' copies: _refresh_layer_copies)."""
        mode = self._cache_mode
        ver = None if mode == "frozen" else self._versions(params)
        hit = self._cache.get(key)
        if not _copies_stale(mode, self.training, any(p.requires_grad for p in params), hit is not None and hit[0] == ver):
            return self._cache[key][1]
        with torch.no_grad():
            val = build()
        self._cache[key] = (ver, val)
        return val

    def _proj_weight(self):                                  # bf16 copy of the feature projection's weight
        pw = self.feature_projection.projection.weight
        return self._cached(("proj",), [pw], lambda: ops.cast_bf16(pw))

    def _posconv_weights(self):                              # (forward, data-gradient) bf16 weights of the positional conv, norm of v
        wn = self.encoder.pos_conv_embed.conv.parametrizations.weight
        gain, v = wn.original0, wn.original1
        return self._cached(("posconv",), [gain, v],
                            lambda: ops.posconv_weight(v, gain.reshape(-1), self.config.num_conv_pos_embedding_groups))

    def _front_params(self, with_embed: bool):               # with_embed=False (no time mask in this forward) leaves masked_spec_embed out
        fp, pc, enc = self.feature_projection, self.encoder.pos_conv_embed.conv, self.encoder
        return _FrontParams(fp.layer_norm.weight, fp.layer_norm.bias, fp.projection.weight, fp.projection.bias,
                            getattr(self, "masked_spec_embed", None) if with_embed else None,
                            pc.parametrizations.weight.original0, pc.parametrizations.weight.original1, pc.bias,
                            enc.layer_norm.weight, enc.layer_norm.bias)

    def _layer_ln_params(self, i: int):
        """The four LayerNorm parameters of layer i; followed by _layer_params(i) they are the parameter list of _LayerImpl."""
        l = self.encoder.layers[i]
        return [l.layer_norm.weight, l.layer_norm.bias, l.final_layer_norm.weight, l.final_layer_norm.bias]

    def _layer_params(self, i: int):
        l = self.encoder.layers[i]
        at, ff = l.attention, l.feed_forward
        return [at.q_proj.weight, at.k_proj.weight, at.v_proj.weight, at.q_proj.bias, at.k_proj.bias, at.v_proj.bias,
                at.out_proj.weight, at.out_proj.bias, ff.intermediate_dense.weight, ff.intermediate_dense.bias,
                ff.output_dense.weight, ff.output_dense.bias]

    def _layer_plan(self):
        """Persistent bf16 copies of every transformer-layer weight (+ packed fp32 q/k/v biases) and the ONE-launch cast
        plan (ops.CastPlan) that refreshes them: 12 layers x 9 jobs instead of ~90 separate cast / cat kernels."""
        plan = self._lplan
        if plan is not None and not plan.stale():
            return plan
        H, I = self.config.hidden_size, self.config.intermediate_size
        jobs, entries = [], []
        for i in range(len(self.encoder.layers)):
            p = self._layer_params(i)
            dev = p[0].device
            bf = lambda *shape: torch.empty(shape, device=dev, dtype=torch.bfloat16)
            e = SimpleNamespace(wqkv=bf(3 * H, H), bqkv=torch.empty(3 * H, device=dev, dtype=torch.float32),
                                wo=bf(H, H), w1=bf(I, H), w2=bf(H, I), bo=p[7].detach(), b1=p[9].detach(), b2=p[11].detach())
            for j in range(3):
                jobs.append((p[j].detach(), e.wqkv[j * H:(j + 1) * H]))
                jobs.append((p[3 + j].detach(), e.bqkv[j * H:(j + 1) * H]))
            jobs += [(p[6].detach(), e.wo), (p[8].detach(), e.w1), (p[10].detach(), e.w2)]
            entries.append(e)
        plan = ops.CastPlan(jobs)
        plan.entries = entries
        self._lplan = plan
        return plan

    def _refresh_layer_copies(self, force: bool = False):
        """Runs the cast plan when the copies may be stale (_copies_stale) or on `force`; a frozen cache outranks both."""
        if self._cache_mode == "frozen":
            return
        plan = self._layer_plan()
        params = [p for i in range(len(self.encoder.layers)) for p in self._layer_params(i)]
        ver = self._versions(params)
        trainable = any(p.requires_grad for p in params)
        if force or _copies_stale(self._cache_mode, self.training, trainable, plan.version == ver, plan.optimizer_synced, plan.after_training):
            with torch.no_grad():
                plan.run()
            plan.version = ver
            plan.after_training = self.training and trainable and not plan.optimizer_synced

    def weights_moved(self) -> None:
        """Something other than a training step rewrote the parameters in place (aptai_amd.optim.Adam.swap_ema: averaged weights
        in, training weights back).  Every `_cached` copy misses in eval mode from here on, and the layer copies are re-cast NOW,
        also when the optimiser publishes them (`optimizer_synced`) and when a graph runner froze the cache: a replayed step reads
        them without asking."""
        self._train_marker += 1
        if self._cache_mode == "frozen":       # as BucketedGraphedStep.suspend(): the graphs keep their own copies
            self._cache_mode = None
            self._cache.clear()
        plan = self._lplan
        if plan is not None and not plan.stale():
            with torch.no_grad():
                plan.run()
            plan.version = None

    def _layer_weights(self, i: int):
        return self._layer_plan().entries[i], self._layer_params(i)

    def _scratch(self, key, numel, dev):
        """Persistent zero-initialised bf16 scratch (the zero gap rows of the packed positional-conv operands are
        written once here and never again)."""
        # one buffer per (key, size), whatever the stream, that dies with the model (ops.ScratchPool: NEVER replaced or freed before) -
        # captured hipGraphs (the graph runners, Force_APTAI's encoder pass ahead) hold its address, and a forward with another batch
        # shape in between (validation at batch 1 between training epochs) used to swap it out from under them: the next replays read
        # freed memory
        return self._scratch_pool.get(key, numel, dev, None, torch.bfloat16, exact=True, zero=True)

    # ------------------------------------------------------------------ geometry of one batch
    def _feature_axis_lens(self, B: int, dev) -> torch.Tensor:
        """[B] int32 filled with hidden_size: the row lengths of the span sampler on the feature axis (a cached constant)."""
        c = self._feat_lens
        if c is None or c.shape[0] != B or c.device != dev:
            c = self._feat_lens = torch.full((B,), self.config.hidden_size, device=dev, dtype=torch.int32)
        return c

    def _geometry(self, B: int, S: int) -> SimpleNamespace:
        cfg = self.config
        Tl = hostlogic.conv_layer_lengths(S, cfg.conv_kernel, cfg.conv_stride)
        T = Tl[-1]
        if T < 1:
            raise ValueError(f"input of {S} samples is shorter than the receptive field of the feature encoder")
        Tp = _round_up(T + 2, 128)
        alloc = [0] * len(Tl)
        alloc[-1] = Tp
        for i in range(len(Tl) - 2, -1, -1):
            alloc[i] = alloc[i + 1] * cfg.conv_stride[i + 1]
        return SimpleNamespace(B=B, S=S, T=T, Tp=Tp, M=B * Tp, Tl=Tl, alloc=alloc)

    # ------------------------------------------------------------------ feature encoder (conv stack)
    def _conv_weights(self):
        cl = self.feature_extractor.conv_layers
        params = [l.conv.weight for l in cl[1:]]
        return self._cached(("convw",), params, lambda: [ops.conv_weight_bf16(p) for p in params])

    def _conv_params(self):
        """Flat parameter list of the conv stack in a fixed order: per layer weight, [bias], [norm weight, norm bias]."""
        cfg = self.config
        out = []
        for i, l in enumerate(self.feature_extractor.conv_layers):
            out.append(l.conv.weight)
            if cfg.conv_bias:
                out.append(l.conv.bias)
            if cfg.feat_extract_norm == "layer" or i == 0:
                out += [l.layer_norm.weight, l.layer_norm.bias]
        return out

    def _conv_forward(self, audio, g, save):
        """7-layer feature encoder (HF:382-419).  Returns (features [M][512] bf16, saved-for-backward | None)."""
        cfg = self.config
        cl = self.feature_extractor.conv_layers
        dev = audio.device
        C = 512
        layer_mode = cfg.feat_extract_norm == "layer"
        sv = SimpleNamespace(bufs=[], pre=[None], stats=[None], audio=audio) if save else None

        def new_buf(i, rows):
            # frozen path: persistent scratch (its slack rows were zeroed once); trainable path: fresh buffers (saved)
            if save:
                return _rows_with_zero_slack(rows, C, dev)
            if i == len(cl) - 1:          # the features outlive this call (saved by the projection's backward): own storage
                return torch.empty((rows, C), device=dev, dtype=torch.bfloat16)
            return self._scratch(("conv", i, rows), rows * C, dev).view(rows, C)
        buf = new_buf(0, g.B * g.alloc[0] + 8)
        l0 = cl[0]
        # batch-invariant inference (forward): the first layer normalises every row over its own frames; never on the saving path
        lens0 = None if save else getattr(g, "lens0", None)
        stats0 = ops.conv0_fwd(audio, l0.conv.weight, l0.conv.bias if cfg.conv_bias else None, l0.layer_norm.weight,
                               l0.layer_norm.bias, 1 if layer_mode else 0, buf, g.Tl[0], g.alloc[0], want_stats=save,
                               frame_lens0=lens0)
        if save:
            sv.bufs.append(buf)
            sv.stats0 = stats0
        ws = self._conv_weights()
        for i in range(1, len(cl)):
            k, s = cfg.conv_kernel[i], cfg.conv_stride[i]
            Mi = g.B * g.alloc[i]
            out = new_buf(i, Mi + 8)
            bias = cl[i].conv.bias if cfg.conv_bias else None
            if layer_mode:
                u = _rows_with_zero_slack(Mi + 8, C, dev) if save else out
                ops.gemm(buf, ws[i - 1], Mi, C, k * C, lda=s * C, out=u, ldc=C, bias=bias)
                _, m, r = ops.layernorm_fwd(u[:Mi], cl[i].layer_norm.weight, cl[i].layer_norm.bias, 1e-5, gelu_after=True,
                                            save_stats=save, out=out[:Mi])
                if save:
                    sv.pre.append(u)
                    sv.stats.append((m, r))
            else:
                u = _rows_with_zero_slack(Mi + 8, C, dev) if save else None
                ops.gemm(buf, ws[i - 1], Mi, C, k * C, lda=s * C, out=out, ldc=C, bias=bias, gelu=True, out_pre=u)
                if save:
                    sv.pre.append(u)
                    sv.stats.append(None)
            buf = out
            if save:
                sv.bufs.append(buf)
        return buf[:g.M], sv

    def _conv_backward(self, sv, g, dfeats, want_params=True, want_audio=False):
        """(gradient w.r.t. the waveform | None, gradients of every conv-stack parameter in the order of _conv_params | None).
        dgrad of a strided conv = the weight GEMM on the SAME overlapping-row view: columns [0, s*C) of the virtual-row gradient own
        frames s*t .. s*t+s-1 outright, the remaining (k-s)*C columns are accumulated one virtual row later.  want_params=False
        (frozen conv stack, waveform requires grad): only the data gradients run - no weight GEMMs, column sums or aptai_conv0_bwd."""
        cfg = self.config
        cl = self.feature_extractor.conv_layers
        C = 512
        layer_mode = cfg.feat_extract_norm == "layer"
        ws = self._conv_weights()
        dev = dfeats.device
        grads = {}
        dy = dfeats                                          # gradient w.r.t. the OUTPUT of layer i (post-activation)
        du_ready = False                                     # base mode: dgrad epilogues already applied gelu' of the layer below
        for i in range(len(cl) - 1, 0, -1):
            k, s = cfg.conv_kernel[i], cfg.conv_stride[i]
            Mi = g.B * g.alloc[i]
            x_in = sv.bufs[i - 1]
            if layer_mode:
                m, r = sv.stats[i]
                du, _, dgam, dbet = ops.layernorm_bwd(dy[:Mi], sv.pre[i][:Mi], m, r, cl[i].layer_norm.weight,
                                                      beta_gelu=cl[i].layer_norm.bias)
                grads[(i, "ln_w")], grads[(i, "ln_b")] = dgam, dbet
            else:
                du = dy[:Mi] if du_ready else ops.dgelu(dy[:Mi].contiguous(), sv.pre[i][:Mi])
            if want_params:
                if cfg.conv_bias:
                    grads[(i, "b")] = ops.colsum(du, Mi, C)
                sk = max(1, min(16, Mi // 4096))
                dw = ops.gemm(du, x_in, C, k * C, Mi, a_kmajor=True, b_kmajor=True, out_f32=True, ldb=s * C, split_k=sk)
                grads[(i, "w")] = dw.view(C, k, C).permute(0, 2, 1).contiguous()      # [N][kw][c] -> nn.Conv1d's [N][c][kw]
            # ---- dgrad into the output of layer i-1
            dx = _rows_with_zero_slack(g.B * g.alloc[i - 1] + 8, C, dev)
            fuse = (not layer_mode) and (i - 1 >= 1)         # base: fold gelu'(u_{i-1}) into the epilogue
            aux = sv.pre[i - 1] if fuse else None
            ops.gemm(du, ws[i - 1], Mi, s * C, C, b_kmajor=True, ldb=k * C, out=dx, ldc=s * C, dgelu_aux=aux,
                     **({"ldaux": s * C} if fuse else {}))
            if k > s:
                n2 = (k - s) * C
                ops.gemm(du, ws[i - 1][:, s * C:], Mi, n2, C, b_kmajor=True, ldb=k * C, out=dx[s:], ldc=s * C, residual=dx[s:],
                         ldr=s * C, dgelu_aux=(aux[s:] if fuse else None), **({"ldaux": s * C} if fuse else {}))
            dy = dx
            du_ready = fuse
        l0 = cl[0]
        args0 = (sv.audio, l0.conv.weight, l0.conv.bias if cfg.conv_bias else None, l0.layer_norm.weight, l0.layer_norm.bias,
                 1 if layer_mode else 0, dy, g.Tl[0], g.alloc[0], sv.stats0)
        daudio = ops.conv0_bwd_data(*args0) if want_audio else None
        if not want_params:
            return daudio, None
        dw0, db0, dg0, dbt0 = ops.conv0_bwd(*args0)
        grads[(0, "w")], grads[(0, "b")], grads[(0, "ln_w")], grads[(0, "ln_b")] = dw0, db0, dg0, dbt0
        out = []
        for i in range(len(cl)):
            out.append(grads[(i, "w")])
            if cfg.conv_bias:
                out.append(grads[(i, "b")])
            if layer_mode or i == 0:
                out += [grads[(i, "ln_w")], grads[(i, "ln_b")]]
        return daudio, out

    def _feature_encoder(self, audio: torch.Tensor, g) -> torch.Tensor:
        params = self._conv_params()
        # autograd path when a conv parameter OR the waveform requires grad (input gradients: saliency, attribution)
        trainable = torch.is_grad_enabled() and (audio.requires_grad or any(p.requires_grad for p in params))
        if trainable and getattr(g, "lens0", None) is not None:
            raise NotImplementedError("batch_invariant: the per-utterance GroupNorm has no backward - run the eval-mode forward "
                                      "under torch.no_grad() or freeze the feature encoder")
        if not trainable:
            with torch.no_grad():
                return self._conv_forward(audio, g, save=False)[0]
        return _ConvStackFn.apply(audio, self, g, *params)

    # ------------------------------------------------------------------ exact (fp32-class) inference pass
    def _exact_weights(self, P: int):
        """Split (weight-side) copies of every GEMM weight and the fp32 weight-normed positional-conv weight, built once per
        parameter version (eval mode trusts Tensor._version, see _cached)."""
        cfg = self.config
        cl = self.feature_extractor.conv_layers
        fp = self.feature_projection
        pc = self.encoder.pos_conv_embed.conv
        params = [l.conv.weight for l in cl[1:]] + [fp.projection.weight, pc.parametrizations.weight.original0,
                                                     pc.parametrizations.weight.original1]
        for i in range(len(self.encoder.layers)):
            params += self._layer_params(i)

        def build():
            w = SimpleNamespace(conv=[], layers=[])
            for l in cl[1:]:
                cw = l.conv.weight.detach()                                  # [N][C][kw] -> [N][kw*C] (K index = kw*C + c)
                w.conv.append(ops.split_f32(cw.permute(0, 2, 1).reshape(cw.shape[0], -1).contiguous(), P, weight_side=True))
            w.proj = ops.split_f32(fp.projection.weight.detach().contiguous(), P, weight_side=True)
            # weight_norm(dim=2): w = g * v / ||v||_(0,1) per tap (HF:340-356), fp32, in the kernels' [group][out][kw*Cg + in] layout
            g0, v = pc.parametrizations.weight.original0.detach(), pc.parametrizations.weight.original1.detach()
            G = cfg.num_conv_pos_embedding_groups
            Hh, Cg, Kw = v.shape
            wn = v * (g0 / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
            # split form (round 4): the input channels of a group padded 48 -> 64, so that one FRAME of a group is exactly one K-tile of
            # the split layout and the Toeplitz rows of the implicit GEMM stay contiguous ([tap][64 channels] = tap * 64 + c)
            w64 = torch.zeros((G, Cg, Kw, 64), device=wn.device, dtype=torch.float32)
            w64[..., :Cg] = wn.view(G, Cg, Cg, Kw).permute(0, 1, 3, 2)
            w.posconv = ops.split_f32(w64.view(G * Cg, Kw * 64), P, weight_side=True)                 # [G Cg][P Kw 64]
            for i in range(len(self.encoder.layers)):
                p = [t.detach() for t in self._layer_params(i)]
                w.layers.append(SimpleNamespace(
                    wqkv=ops.split_f32(torch.cat(p[0:3]).contiguous(), P, weight_side=True), bqkv=torch.cat(p[3:6]).contiguous(),
                    wo=ops.split_f32(p[6].contiguous(), P, weight_side=True), bo=p[7],
                    w1=ops.split_f32(p[8].contiguous(), P, weight_side=True), b1=p[9],
                    w2=ops.split_f32(p[10].contiguous(), P, weight_side=True), b2=p[11]))
            return w
        return self._cached(("exact", P), params, build)

    def _exact_attention(self, a_s, w, lens_i32, g, P=3):
        """q|k|v projection + softmax(Q K^T / sqrt(d) + key mask) V per head (HF:438-548) at fp32-class accuracy, from the layer input's
        split pieces `a_s` [M][P H], in TWO launches:
          * the q|k|v projection as one split-operand GEMM whose result leaves already split (APTAI_EPI_SPLIT_OUT): Q in the
            activation-side piece order, K and V (columns >= H, `split_out_bcol`) in the weight-side order.  Per head the 64 feature
            columns are exactly one K-tile of the split layout, so head h is the column block [64 P h, 64 P (h + 1)) of its third;
          * aptai_attention_exact_fwd: scores, masked softmax, the split of the probabilities and P . V in one kernel - every product the
            3 (6) leading bf16 piece products in fp32, nothing but the context (as the out-projection's split A operand) stored.
        (Round 3: 24 launches per layer on the fp32 matrix instruction, 10 of the mode's 27 ms; round 4 first ran the scores, the softmax and
        P . V as three launches with the fp32 scores and the split probabilities in memory: 0.29 ms of the layer's 1.0.)"""
        cfg = self.config
        H, heads, B, Tp, M = cfg.hidden_size, cfg.num_attention_heads, g.B, g.Tp, g.M
        d = H // heads
        if d != 64:
            raise NotImplementedError("the exact attention is built for head_dim 64 (one K-tile of the split layout per head)")
        qkvs = ops.gemm_split(a_s, w.wqkv, M, 3 * H, H, P, bias=w.bqkv, split_out=True, split_bcol=H)          # [M][P 3H]: Q | K | V
        return ops.attention_exact_fwd(qkvs, lens_i32, B, Tp, H, heads, P, d ** -0.5)

    def _forward_exact(self, audio, g, lens_i32, P, output_hidden_states):
        """The whole encoder in eval mode at fp32-class accuracy (set_encoder_precision("f32x3" | "f32x6")).  Returns
        (last hidden state fp32 [M][H], list of hidden states fp32)."""
        cfg = self.config
        cl = self.feature_extractor.conv_layers
        dev = audio.device
        C, H, I, M = 512, cfg.hidden_size, cfg.intermediate_size, g.M
        eps = cfg.layer_norm_eps
        W = self._exact_weights(P)
        layer_mode = cfg.feat_extract_norm == "layer"
        # ---- feature encoder (HF:382-419)
        l0 = cl[0]
        stats = None
        if not layer_mode:                                   # GroupNorm statistics (double-precision window moments, csrc/conv.hip)
            scratch = self._scratch(("conv", 0, g.B * g.alloc[0] + 8), (g.B * g.alloc[0] + 8) * C, dev).view(-1, C)
            stats = ops.conv0_fwd(audio, l0.conv.weight, l0.conv.bias if cfg.conv_bias else None, l0.layer_norm.weight,
                                  l0.layer_norm.bias, 0, scratch, g.Tl[0], g.alloc[0], want_stats=True,
                                  frame_lens0=getattr(g, "lens0", None))
        if layer_mode:
            # wav2vec2-large: a LayerNorm sits between the conv layers, so every layer's fp32 output is stored, normalised and split
            buf = torch.empty((g.B * g.alloc[0] + 8, C), device=dev, dtype=torch.float32)
            buf[g.B * g.alloc[0]:].zero_()
            ops.conv0_fwd_f32(audio, l0.conv.weight, l0.conv.bias if cfg.conv_bias else None, l0.layer_norm.weight, l0.layer_norm.bias,
                              1, buf, g.Tl[0], g.alloc[0], stats)
            pending_gelu = False
            for i in range(1, len(cl)):
                k, s = cfg.conv_kernel[i], cfg.conv_stride[i]
                Mi = g.B * g.alloc[i]
                xs = ops.split_f32(buf, P, gelu=pending_gelu)
                out = torch.empty((Mi + 8, C), device=dev, dtype=torch.float32)
                out[Mi:].zero_()
                ops.gemm_split(xs, W.conv[i - 1], Mi, C, k * C, P, lda=s * C, bias=cl[i].conv.bias if cfg.conv_bias else None, out=out, ldc=C)
                _, y32 = ops.layernorm_fwd_f32in(out[:Mi], cl[i].layer_norm.weight, cl[i].layer_norm.bias, 1e-5, want_bf16=False)
                out[:Mi].copy_(y32)
                buf, pending_gelu = out, True
        else:
            # wav2vec2-base (round 4): no fp32 intermediate between the conv layers at all - the first layer writes its activated output as
            # split pieces (aptai_conv0_fwd_split), layers 1..5 leave their GEMMs GELU'd and split (APTAI_EPI_SPLIT_OUT | APTAI_EPI_GELU),
            # only the last layer's output is fp32 (it feeds the feature projection's LayerNorm).  The 8 slack rows the overlapping-row
            # view of the next layer can read are zeroed; frames beyond an utterance are padded frames like everywhere else.
            M0 = g.B * g.alloc[0]
            xs = torch.empty((M0 + 8, P * C), device=dev, dtype=torch.bfloat16)
            xs[M0:].zero_()
            ops.conv0_fwd_split(audio, l0.conv.weight, l0.conv.bias if cfg.conv_bias else None, l0.layer_norm.weight, l0.layer_norm.bias,
                                0, xs, P, g.Tl[0], g.alloc[0], stats)
            for i in range(1, len(cl)):
                k, s = cfg.conv_kernel[i], cfg.conv_stride[i]
                Mi = g.B * g.alloc[i]
                last = i == len(cl) - 1
                bias_i = cl[i].conv.bias if cfg.conv_bias else None
                if last:
                    buf = torch.empty((Mi + 8, C), device=dev, dtype=torch.float32)
                    buf[Mi:].zero_()
                    ops.gemm_split(xs, W.conv[i - 1], Mi, C, k * C, P, lda=s * C, bias=bias_i, out=buf, ldc=C)
                else:
                    nxt = torch.empty((Mi + 8, P * C), device=dev, dtype=torch.bfloat16)
                    nxt[Mi:].zero_()
                    ops.gemm_split(xs, W.conv[i - 1], Mi, C, k * C, P, lda=s * C, bias=bias_i, out=nxt, ldc=P * C, split_out=True, gelu=True)
                    xs = nxt
        feats = ops.bias_act_res_f32(buf[:M], gelu=True)                                               # [M][512] fp32
        # ---- feature projection, padded-frame zeroing, positional conv (HF:422-434, 678-681, 326-379)
        fp = self.feature_projection
        _, n0 = ops.layernorm_fwd_f32in(feats, fp.layer_norm.weight, fp.layer_norm.bias, eps, want_bf16=False)
        h0 = ops.gemm_split(ops.split_f32(n0, P), W.proj, M, H, C, P, bias=fp.projection.bias)
        ops.bias_act_res_f32(h0, lens_i32=lens_i32, rows_per_b=g.Tp, out=h0)
        G, Kw = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
        Cg, pad = H // G, Kw // 2
        if Cg > 64 or Cg % 8:
            raise NotImplementedError("the exact positional conv is built for at most 64 channels per group (a multiple of 8)")
        rows_p = g.Tp + 2 * pad
        # grouped Conv1d(k = 128, 'same') as ONE batched split-operand NT launch over (group, utterance): row t of group grp is the Kw
        # frames t .. t + Kw - 1 of the zero-padded sequence, 64 (48 real) channels each - lda = one frame.  (Round 3 ran it as 16
        # batched calls on the fp32 matrix instruction: 2.4 ms of the exact-mode step.)
        xg = torch.zeros((G, g.B, rows_p, 64), device=dev, dtype=torch.float32)
        xg[:, :, pad:pad + g.Tp, :Cg].copy_(h0.view(g.B, g.Tp, G, Cg).permute(2, 0, 1, 3))
        xs = ops.split_f32(xg.view(G * g.B * rows_p, 64), P)                                           # [G B rows_p][P 64]
        pc = self.encoder.pos_conv_embed.conv
        conv = torch.empty((M, H), device=dev, dtype=torch.float32)
        KP = P * Kw * 64
        ops.gemm(xs, W.posconv, g.Tp, Cg, KP, lda=P * 64, ldb=KP, out=conv, ldc=H, out_f32=True, bias=pc.bias, tile=128,
                 batch=dict(outer=G, inner=g.B, a=(g.B * rows_p * P * 64, rows_p * P * 64), b=(Cg * KP, 0), c=(Cg, g.Tp * H), bias=(Cg, 0)))
        h = ops.bias_act_res_f32(conv, gelu=True, res=h0)
        h_s = None                                           # split pieces of h where a LayerNorm has just produced them
        if not cfg.do_stable_layer_norm:
            h, h_s = ops.layernorm_fwd_f32in_split(h, self.encoder.layer_norm.weight, self.encoder.layer_norm.bias, eps, P)
        # ---- transformer layers (HF:575-654).  Every LayerNorm whose result feeds a product also writes it split (round 4).
        hidden = []
        for i, layer in enumerate(self.encoder.layers):
            hidden.append(h)
            w = W.layers[i]
            ln1, ln2 = layer.layer_norm, layer.final_layer_norm
            if cfg.do_stable_layer_norm:
                _, a_s = ops.layernorm_fwd_f32in_split(h, ln1.weight, ln1.bias, eps, P, want_f32=False)
            else:
                a_s = h_s if h_s is not None else ops.split_f32(h, P)
            ctx = self._exact_attention(a_s, w, lens_i32, g, P)
            s1 = ops.gemm_split(ctx, w.wo, M, H, H, P, bias=w.bo, residual_f32=h)          # ctx: already split
            if cfg.do_stable_layer_norm:
                _, f_s = ops.layernorm_fwd_f32in_split(s1, ln2.weight, ln2.bias, eps, P, want_f32=False)
                res2 = s1
            else:
                res2, f_s = ops.layernorm_fwd_f32in_split(s1, ln1.weight, ln1.bias, eps, P)
            # FFN1's result leaves its GEMM already GELU'd and split (EPI_SPLIT_OUT): 100 MB of fp32 and a split pass less per layer
            us = ops.gemm_split(f_s, w.w1, M, I, H, P, bias=w.b1, split_out=True, gelu=True)
            s2 = ops.gemm_split(us, w.w2, M, H, I, P, bias=w.b2, residual_f32=res2)
            if cfg.do_stable_layer_norm:
                h, h_s = s2, None
            else:
                h, h_s = ops.layernorm_fwd_f32in_split(s2, ln2.weight, ln2.bias, eps, P)
        if cfg.do_stable_layer_norm:
            _, h = ops.layernorm_fwd_f32in(h, self.encoder.layer_norm.weight, self.encoder.layer_norm.bias, eps, want_bf16=False)
        hidden.append(h)
        return h, hidden

    # ------------------------------------------------------------------ forward, step by step
    def _samples_feature_mask(self, mask_feature_indices) -> bool:
        return mask_feature_indices is None and self.training and self.config.apply_spec_augment and self.config.mask_feature_prob > 0

    def _check_request(self, input_values, want_attn: bool, batch_invariant: bool, mask_feature_indices) -> None:
        """Every refusal of forward(), before anything is launched and before `_step` moves."""
        cfg, prec = self.config, self._encoder_precision
        if not input_values.is_cuda:
            raise ops._lib.AptaiHipError("Wav2Vec2Model runs on the MI355X only (no CPU fallback)")
        if want_attn and prec not in ("bf16", "bf16_f32res"):
            raise NotImplementedError(f"output_attentions is not available with encoder precision {prec!r}: "
                                      "the attention maps come from the bf16 attention kernels ('bf16', 'bf16_f32res')")
        if batch_invariant:                                  # opt-in, eval mode only
            if prec not in _BATCH_INVARIANT_PRECISIONS:
                raise NotImplementedError(f"batch_invariant is not available with encoder precision {prec!r}: its first conv layer "
                                          "does not take the per-utterance statistics")
            if torch.is_grad_enabled() and input_values.requires_grad:
                raise NotImplementedError("batch_invariant: no gradient w.r.t. the waveform (the per-utterance GroupNorm backward is "
                                          "not built); switch it off for input gradients")
        if mask_feature_indices is not None:
            shape, want = tuple(torch.as_tensor(mask_feature_indices).shape), (input_values.shape[0], cfg.hidden_size)
            if shape != want:
                raise ValueError(f"mask_feature_indices has shape {shape}, expected (batch, hidden_size) = {want}")
        elif self._samples_feature_mask(mask_feature_indices):
            if cfg.mask_feature_length < 1 or cfg.mask_feature_length > cfg.hidden_size:
                raise ValueError(f"mask_feature_length={cfg.mask_feature_length} must lie in [1, hidden_size={cfg.hidden_size}]")
            if _SPEC_ON_DEVICE:
                ops.feature_mask_span_check(cfg.hidden_size, cfg.mask_feature_prob, cfg.mask_feature_length, cfg.mask_feature_min_masks)

    def _lengths(self, attention_mask, g, dev, batch_invariant: bool):
        """(frame_lens int64 [B], lens_i32, sample_lens | None).  Batch-invariant inference, each row as if it ran alone: the first conv
        layer's statistics over the row's own frames (g.lens0), the heads' FIR zero padding at the row's own length (g.fir_lens)."""
        cfg = self.config
        sample_lens = None if attention_mask is None else attention_mask.to(dev).long().sum(-1)
        if sample_lens is not None:
            frame_lens = hostlogic.feat_extract_output_lengths(sample_lens, cfg.conv_kernel, cfg.conv_stride).clamp(min=1, max=g.T)
        else:
            frame_lens = torch.full((g.B,), g.T, device=dev, dtype=torch.long)
        lens_i32 = frame_lens.to(torch.int32).contiguous()
        g.lens0 = None
        if batch_invariant and sample_lens is not None:
            g.lens0 = hostlogic.conv0_frame_lengths(sample_lens, cfg.conv_kernel[0], cfg.conv_stride[0]).clamp(min=1, max=g.Tl[0])
        elif batch_invariant:
            g.lens0 = torch.full((g.B,), g.Tl[0], device=dev, dtype=torch.int32)
        # (B,) whatever the mask's rank: APTAI.get_aptai_output hands in its (1, 1) length as a (1, 1, 1) mask
        g.fir_lens = lens_i32.reshape(-1) if batch_invariant else None
        return frame_lens, lens_i32, sample_lens

    def _spec_masks(self, g, lens_i32, ragged_lens, seed, mask_time_indices, mask_feature_indices):
        """(spec [B][T] | None, feat [B][H] | None), device uint8: the SpecAugment masks along time (HF:1272-1316) and along the hidden
        axis (HF `_mask_hidden_states`, second half: spans over the H channels, every row of length H).  Each is the explicit mask, or
        sampled in train mode: by a kernel from the device-resident lengths (no device->host copy, a 2.3 ms stall of the eager loop per
        step; HF's `_compute_mask_indices` rule, counter-hash draws, a seed stream per mask) or, with _SPEC_ON_DEVICE off, by numpy in
        HF's RNG order (`ragged_lens`: frame counts an attention mask gave).  ``apply_spec_augment = False``: none, explicit ones included."""
        cfg = self.config
        if not cfg.apply_spec_augment:
            return None, None
        dev, B, H = lens_i32.device, g.B, cfg.hidden_size
        sample_time = mask_time_indices is None and cfg.mask_time_prob > 0 and self.training
        sample_feat = self._samples_feature_mask(mask_feature_indices)
        spec = feat = None
        if mask_time_indices is not None:
            spec = torch.as_tensor(mask_time_indices).to(dev).to(torch.uint8).contiguous()
        elif sample_time and _SPEC_ON_DEVICE:
            spec = ops.spec_augment_mask(lens_i32, B, g.T, cfg.mask_time_prob, cfg.mask_time_length, cfg.mask_time_min_masks,
                                         _seed(seed, _TIME_MASK_STREAM))
        if mask_feature_indices is not None:
            feat = torch.as_tensor(mask_feature_indices).to(dev).to(torch.uint8).contiguous()
            if feat.data_ptr() % 4:                          # the kernels load four mask bytes as one word
                feat = feat.clone()
        elif sample_feat and _SPEC_ON_DEVICE:
            feat = ops.spec_augment_mask(self._feature_axis_lens(B, dev), B, H, cfg.mask_feature_prob, cfg.mask_feature_length,
                                         cfg.mask_feature_min_masks, _seed(seed, _FEATURE_MASK_STREAM))
        if (sample_time or sample_feat) and not _SPEC_ON_DEVICE:
            m_time, m_feat = _host_spec_masks(cfg, B, g.T, None if ragged_lens is None else ragged_lens.cpu(), sample_time, sample_feat)
            if sample_time:
                spec = torch.from_numpy(m_time.astype(np.uint8)).to(dev)
            if sample_feat:
                feat = torch.from_numpy(m_feat.astype(np.uint8)).to(dev)
        return spec, feat

    # The three passes return (last hidden state bf16 [M][H], the same in fp32 | None, hidden states: the input of every layer and the
    # last one, attention maps: one [B, heads, T, T] fp32 per layer (None where LayerDrop skipped it) | None).
    def _encode_exact(self, audio, g, lens_i32, P, output_hidden_states, mask_time_indices, mask_feature_indices):
        """Inference at fp32-class accuracy (set_encoder_precision("f32x3" | "f32x6")): the whole encoder, conv stack included."""
        if mask_time_indices is not None or mask_feature_indices is not None:
            raise NotImplementedError("the exact inference pass takes no SpecAugment mask (eval mode never samples one)")
        h32, hidden32 = self._forward_exact(audio, g, lens_i32, P, output_hidden_states)
        return h32.to(torch.bfloat16), h32, hidden32, None

    def _encode_f32res(self, h, g, lens_i32, want_attn: bool):
        """Inference with the residual stream in fp32 (set_encoder_precision("bf16_f32res")): the transformer layers."""
        cfg = self.config
        hidden, attn = [], []
        h32 = h.float()
        for i in range(len(self.encoder.layers)):
            hidden.append(h if h is not None else h32)
            impl = _LayerImpl(cfg, g, lens_i32, self._layer_plan().entries[i], False, 0, want_attn=want_attn)
            h, h32, probs = impl.fwd_f32res(h, h32, self._layer_ln_params(i))
            if want_attn:
                attn.append(probs[:, :, :g.T, :g.T])
        if cfg.do_stable_layer_norm:
            h, h32 = ops.layernorm_fwd_f32in(h32, self.encoder.layer_norm.weight, self.encoder.layer_norm.bias, cfg.layer_norm_eps)
        hidden.append(h)
        return h, h32, hidden, attn if want_attn else None

    def _encode_default(self, h, g, lens_i32, seed, want_attn: bool):
        """The transformer layers under autograd with LayerDrop (HF:694-707 / 767-780); eval-mode MXFP8 operands with "mxfp8"."""
        cfg, training = self.config, self.training
        hidden, attn = [], []
        attn_state = SimpleNamespace(seen=False) if want_attn else None
        mx = self._encoder_precision == "mxfp8" and not training
        for i in range(len(self.encoder.layers)):
            hidden.append(h)
            if training and cfg.layerdrop > 0 and float(torch.rand([], generator=self._layerdrop_gen)) < cfg.layerdrop:
                attn.append(None)
                continue
            w, lin_params = self._layer_weights(i)
            impl = _LayerImpl(cfg, g, lens_i32, w, training, _seed(seed, _LAYER_STREAM_BASE + i),
                              mx=self._mx_layer_weights(i) if mx else None, want_attn=want_attn, attn_state=attn_state)
            out = _run(impl, h, *self._layer_ln_params(i), *lin_params)
            h, probs = out if want_attn else (out, None)
            if want_attn:
                attn.append(probs[:, :, :g.T, :g.T])
        if cfg.do_stable_layer_norm:
            h = _run(_FinalLNImpl(cfg, g), h, self.encoder.layer_norm.weight, self.encoder.layer_norm.bias)
        hidden.append(h)
        return h, None, hidden, attn if want_attn else None

    def _output(self, g, frame_lens, last, last_f32, hidden, attn, feats, feat, output_hidden_states):
        def view(t):
            return t.view(g.B, g.Tp, -1)[:, :g.T]
        out = Wav2Vec2BaseModelOutput(
            last_hidden_state=view(hidden[-1]), extract_features=None,       # fp32 from the exact pass, bf16 otherwise
            hidden_states=tuple(view(t) for t in hidden) if output_hidden_states else None,
            attentions=tuple(attn) if attn is not None else None)
        out._geom, out._frame_lens, out._flat_last, out._flat_last_f32 = g, frame_lens, last, last_f32      # flat [M][H]: bf16; fp32 | None
        out._features, out._feature_mask = feats, feat       # conv features [M][512] bf16 | None; the feature-axis mask applied | None
        return out

    def forward(self, input_values, attention_mask=None, mask_time_indices=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, mask_feature_indices=None, **kw):
        """HF:1319-1375.  ``attention_mask`` follows the reference's convention: the (B,1) tensor of sample
        counts (models/aptai.py:77), or a regular (B,S) 0/1 mask; both reduce to lengths via a row sum (HF:1023).

        ``mask_feature_indices`` (bool / uint8 ``[B, hidden_size]``) is an explicit SpecAugment mask along the hidden axis, the
        counterpart of ``mask_time_indices``: those channels are zeroed on every frame of the row, in train and eval mode alike
        (and, like ``mask_time_indices``, not at all under ``apply_spec_augment = False``).  HF has no
        such argument (it only samples the mask, in train mode, when ``mask_feature_prob > 0``, which this forward does as well);
        it exists so that a run can be reproduced and tested.  The mask that was applied, sampled or given, is
        ``out._feature_mask`` (a device uint8 ``[B, hidden_size]``, or None)."""
        want_attn = bool(output_attentions)
        batch_invariant = bool(self.batch_invariant) and not self.training
        self._check_request(input_values, want_attn, batch_invariant, mask_feature_indices)
        audio = input_values.float().contiguous()
        g = self._geometry(*audio.shape)
        frame_lens, lens_i32, _ = self._lengths(attention_mask, g, audio.device, batch_invariant)
        self._step += 1
        seed = _seed(self.base_seed, self._step)
        inference = not self.training and not torch.is_grad_enabled()
        if self.training and torch.is_grad_enabled():
            self._train_marker += 1
        prec = self._encoder_precision
        feats = feat = None
        if prec in ("f32x3", "f32x6") and inference:
            enc = self._encode_exact(audio, g, lens_i32, 3 if prec == "f32x3" else 6, output_hidden_states, mask_time_indices,
                                     mask_feature_indices)
        else:
            feats = self._feature_encoder(audio, g)                                     # [M][512] bf16
            spec, feat = self._spec_masks(g, lens_i32, frame_lens if attention_mask is not None else None, seed, mask_time_indices,
                                          mask_feature_indices)
            # feature projection + SpecAugment + padded-frame zeroing + positional conv (HF:429-434, 678-681, 689-692).  The eager front
            # draws from the step seed itself, the graph runners from _seed(their seed, 1): existing behaviour, part of recorded runs
            front = _FrontImpl(self.config, g, lens_i32, spec, self.training, seed, self, feat=feat)
            h = _run(front, feats, *self._front_params(with_embed=spec is not None))
            self._refresh_layer_copies()
            if prec == "bf16_f32res" and inference:
                enc = self._encode_f32res(h, g, lens_i32, want_attn)
            else:
                enc = self._encode_default(h, g, lens_i32, seed, want_attn)
        return self._output(g, frame_lens, *enc, feats, feat, output_hidden_states)
