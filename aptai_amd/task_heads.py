"""Task heads: what runs after the encoder's last hidden state, written once per model for the eager autograd path (``HeadFn``) and
the hipGraph runners (aptai_amd.graphed).  A head is a plain object (no nn.Module, no state-dict key), reachable as ``model.task_head``:

    params(model)                           the trainable parameters, in gradient order
    state(model, g, seed, training, ...)    the namespace fwd / bwd read (targets, dropout rates; seed = the parts before the stream id)
    fwd(h, params, st)                      -> (outs, saved)
    bwd(saved, st, params, h, gloss)        -> (dh | None, one gradient per parameter); gloss = None means dLoss = 1
    result(outs, g, params)                 the dict the model returns
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import hostlogic, ops
from .modules import fwd_sum_ctc, lstm_whh_grads, xatt_core_bwd, xatt_core_fwd
from .wav2vec2 import _APTAI_HEADS_STREAM, _FORCE_HEADS_STREAM, _PR_HEAD_STREAM, _round_up, _seed

_PADN = 64      # head Linears run on the MFMA GEMM with N padded to a multiple of 64


def padded_head_weight(w, b, Np):
    """(bf16 [Np][H], fp32 [Np]) of a head Linear(H, n): rows n..Np zero."""
    wp = torch.zeros((Np, w.shape[1]), device=w.device, dtype=torch.bfloat16)
    ops.cast_bf16(w.detach(), wp[:w.shape[0]])
    bp = torch.zeros(Np, device=w.device, dtype=torch.float32)
    bp[:b.shape[0]] = b.detach()
    return wp, bp


def padded_linear_bwd(M, H, *heads):
    """Backward of padded head Linears: (dy bf16 [M][Np], wp [Np][H], x [M][H]) each -> [(dx, dW fp32 [Np][H], db [Np])].  Issued
    stage by stage (every dX, then every split-K dW, then every bias sum): the order the tail graph holds."""
    sk = max(1, min(16, M // 1024))
    dx = [ops.gemm(dy, wp, M, H, wp.shape[0], b_kmajor=True) for dy, wp, _ in heads]
    dw = [ops.gemm(dy, x, wp.shape[0], H, M, a_kmajor=True, b_kmajor=True, out_f32=True, split_k=sk) for dy, wp, x in heads]
    db = [ops.colsum(dy, M, wp.shape[0]) for dy, wp, _ in heads]
    return list(zip(dx, dw, db))


class HeadFn(torch.autograd.Function):
    """head.fwd / head.bwd behind autograd (the eager drop-in path): only the loss is differentiable."""

    @staticmethod
    def forward(ctx, head, h, st, *params):
        outs, ctx.saved = head.fwd(h, params, st)
        ctx.head, ctx.st, ctx.params, ctx.h = head, st, params, h
        outs = tuple(t.clone() for t in outs[:head.clones]) + outs[head.clones:]
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    def backward(ctx, gloss, *_):
        grads = ctx.head.bwd(ctx.saved, ctx.st, ctx.params, ctx.h, gloss)
        ctx.saved = ctx.h = None
        return (None, grads[0], None) + tuple(grads[1:])


def _pad_to(v, n, value):
    """v (B, L) with `value` appended up to n columns; rows of n or more stay."""
    return torch.nn.functional.pad(v, (0, n - v.shape[1]), value=value) if v.shape[1] < n else v


class _EncoderHead:
    """A head over an encoder that trains also answers what the graph runners ask about a batch: the batch padded to a bucket of
    Sb samples / Tb frames with the collate's own padding values, what a runner's shape depends on beyond (batch size, bucket length),
    a runner's result cut back to the batch's own T frames; below, the static target buffers of a shape (the target arguments of
    `state`) and the copy of a batch into the runner's static inputs `b` (cfg, g, audio, lens, targets, ring)."""
    clones = 0                              # leading outs that HeadFn hands out as copies
    forward_args = ()                       # what the model's forward takes before the batch (the eager warm-up call)
    global_loss_norm = False                # the loss is a masked mean that data parallelism normalises globally (dp.GlobalLossNorm)

    def pad_batch(self, batch, Sb, Tb, label_bucket):
        return dict(batch, **{self.audio_key: _pad_to(batch[self.audio_key], Sb, 0)})

    def cache_key(self, padded):
        return ()

    def cut(self, out, T):
        return {k: v[:T] if k == "log_probs" else v[:, :T] if v.dim() > 1 else v for k, v in out.items()}     # (B, T, ...) but log_probs (T, B, V)


# ------------------------------------------------------------------------------------------------- APTAI
class AptaiHead(_EncoderHead):
    """tanh/leaky-relu -> Linear(H, n) x2 -> FIR -> masked MSE + masked CE (+ argmax), models/aptai.py:83-106.
    outs = (loss, mse, ce, tvs, pred, logits)."""
    audio_key, forward_args, global_loss_norm = "audio_inputs", (0,), True         # forward(epoch, **batch)
    clones = 3                              # loss, mse, ce leave the scalar block the backward reads

    def params(self, model):
        return [model.tv_head[2].weight, model.tv_head[2].bias, model.phn_head[2].weight, model.phn_head[2].bias]

    def state(self, model, g, seed, training, tv_targets, phn_targets):
        if tv_targets is None:
            tv_targets = torch.full((g.B, g.T, model.n_tv), -100.0, device=model.tv_head[2].weight.device)
            phn_targets = torch.zeros((g.B, g.T), device=tv_targets.device, dtype=torch.long)
        return SimpleNamespace(g=g, p_tv=model.tv_head[0].p if training else 0.0, p_ph=model.phn_head[0].p if training else 0.0,
                               seed=_seed(*seed, _APTAI_HEADS_STREAM), taps=model.tv_lowpass.taps(), tv_tgt=tv_targets.contiguous(),
                               phn_tgt=phn_targets.contiguous(), w_mse=0.5, w_ce=0.5)

    def fwd(self, h, params, st):
        tv_w, tv_b, ph_w, ph_b = params
        g, M, H = st.g, st.g.M, h.shape[1]
        n_tv, n_phn = tv_w.shape[0], ph_w.shape[0]
        a_tv, a_ph = ops.head_act_fwd(h, st.p_tv, st.p_ph, st.seed)
        wtv, btv = padded_head_weight(tv_w, tv_b, _PADN)
        wph, bph = padded_head_weight(ph_w, ph_b, _PADN)
        tv_raw = ops.gemm(a_tv, wtv, M, _PADN, H, bias=btv, out_f32=True)
        logits = ops.gemm(a_ph, wph, M, _PADN, H, bias=bph, out_f32=True)
        tvs = torch.empty((g.B, g.T, n_tv), device=h.device, dtype=torch.float32)
        # batch-invariant inference (Wav2Vec2Model.batch_invariant): the filter's zero padding starts at each row's own length
        ops.lowpass_fir(tv_raw, _PADN, g.Tp, st.taps, tvs, n_tv, g.T, g.B, g.T, g.T, n_tv, n_tv, frame_lens=getattr(g, "fir_lens", None))
        scalars, pred = ops.aptai_loss_fwd(tvs, st.tv_tgt, logits, _PADN, g.Tp, st.phn_tgt, g.B, g.T, n_tv, n_phn, st.w_mse, st.w_ce)
        saved = SimpleNamespace(a_tv=a_tv, a_ph=a_ph, wtv=wtv, wph=wph, tvs=tvs, logits=logits, scalars=scalars, n_tv=n_tv, n_phn=n_phn)
        return (scalars[0], scalars[1], scalars[2], tvs, pred, logits), saved

    def bwd(self, s, st, params, h, gloss):
        g, M, H = st.g, st.g.M, h.shape[1]
        gl = None if gloss is None else gloss.float().reshape(1).contiguous()        # None: the loss kernel gets a null pointer (= 1)
        # data parallel: normalise by the GLOBAL valid counts / world (dp.GlobalLossNorm) instead of this shard's own counts
        norm = getattr(st, "norm_scalars", None)
        d_tvs, d_logits = ops.aptai_loss_bwd(s.tvs, st.tv_tgt, s.logits, _PADN, g.Tp, st.phn_tgt, g.B, g.T, s.n_tv, s.n_phn, st.w_mse,
                                             st.w_ce, norm() if callable(norm) else (norm if norm is not None else s.scalars), gl,
                                             ldd=_PADN)
        d_tvraw = torch.empty((M, _PADN), device=h.device, dtype=torch.bfloat16)
        ops.lowpass_fir(d_tvs, s.n_tv, g.T, st.taps, d_tvraw, _PADN, g.Tp, g.B, g.T, g.Tp, s.n_tv, _PADN)
        (da_tv, dwtv, dbtv), (da_ph, dwph, dbph) = padded_linear_bwd(M, H, (d_tvraw, s.wtv, s.a_tv), (d_logits, s.wph, s.a_ph))
        dh = ops.head_act_bwd(h, da_tv, da_ph, st.p_tv, st.p_ph, st.seed)
        return dh, dwtv[:s.n_tv], dbtv[:s.n_tv], dwph[:s.n_phn], dbph[:s.n_phn]

    def result(self, outs, g, params):
        return dict(zip(("loss", "mse_loss", "ce_loss", "tvs_pred", "phn_fc_pred"), outs))

    # ---- graph runners
    def static_targets(self, model, g, batch, dev):
        return {"tv_targets": torch.zeros((g.B, g.T, model.n_tv), device=dev, dtype=torch.float32),
                "phn_targets": torch.zeros((g.B, g.T), device=dev, dtype=torch.int64)}

    def set_batch(self, b, batch):
        """Host tensors go through a two-slot ring of pinned staging buffers and asynchronous copies on the step's stream:
        10.7 ms/step against 10.3 with the batch resident (pageable copies, which block the host until the GPU has drained:
        34 ms/step)."""
        tv_tgt, phn_tgt = b.targets["tv_targets"], b.targets["phn_targets"]
        lens_cpu = batch["audio_lengths"].detach().cpu().long()
        fl = hostlogic.feat_extract_output_lengths(lens_cpu, b.cfg.conv_kernel, b.cfg.conv_stride).clamp(min=1, max=b.g.T)
        tracks = [batch[k] for k in batch if k not in ("audio_inputs", "audio_lengths", "phn_frames_49hz", "phoneme_labels")]
        if batch["audio_inputs"].device.type == "cpu":
            # staging copies through numpy: single-threaded memcpy / cast.  torch's copy_ goes parallel above 32 K elements
            # and the OpenMP workers then spin on the cores the launching thread needs (host time per step 8 -> 19 ms).
            if b.ring is None:
                b.ring = ops.PinnedRing((b.audio, b.lens, tv_tgt, phn_tgt), 2)
            audio, lens, tv, phn = b.ring.next()
            np.copyto(audio, batch["audio_inputs"].detach().numpy(), casting="same_kind")
            np.copyto(lens, fl.numpy(), casting="same_kind")
            for j, t in enumerate(tracks):                       # f64 (B, T) tracks -> one (B, T, n_tv) f32 block
                tv[:, :, j] = t.detach().numpy()
            np.copyto(phn, batch["phn_frames_49hz"].numpy(), casting="same_kind")
            b.ring.send()
            return
        b.audio.copy_(batch["audio_inputs"].float())
        b.lens.copy_(fl.to(torch.int32))
        tv_tgt.copy_(torch.stack(tracks, dim=-1).float())
        phn_tgt.copy_(batch["phn_frames_49hz"])

    def pad_batch(self, batch, Sb, Tb, label_bucket):
        out = super().pad_batch(batch, Sb, Tb, label_bucket)
        for k, v in batch.items():                               # frame-rate targets (B, T): padded, or cut to the bucket
            if k not in ("audio_inputs", "audio_lengths", "phoneme_labels") and v.dim() == 2:
                out[k] = _pad_to(v, Tb, 0 if k == "phn_frames_49hz" else -100.0) if v.shape[1] <= Tb else v[:, :Tb]
        return out


# ------------------------------------------------------------------------------------------------- CTC
class CtcHead(_EncoderHead):
    """dropout -> Linear(H, V) -> log_softmax -> CTC (models/w2v2_pr.py:54-81).  outs = (loss, logits, log_probs, hd)."""
    audio_key = "input_values"

    def params(self, model):
        return [model.pr_head.weight, model.pr_head.bias]

    def state(self, model, g, seed, training, targets, state_lens, target_lens):
        cfg, dev = model.wav2vec2.config, model.pr_head.weight.device
        i32 = lambda t: t.to(dev).to(torch.int32).contiguous()                                   # noqa: E731
        return SimpleNamespace(g=g, p_final=model.dropout.p if training else 0.0, seed=_seed(*seed, _PR_HEAD_STREAM), targets=i32(targets),
                               state_lens=i32(state_lens), target_lens=i32(target_lens), blank=getattr(cfg, "blank", 0),
                               reduction=cfg.ctc_loss_reduction, zero_infinity=cfg.ctc_zero_infinity)

    def fwd(self, h, params, st):
        w, b = params
        g, M, H = st.g, st.g.M, h.shape[1]
        V = w.shape[0]
        Np = _round_up(V, _PADN)
        hd = ops.dropout(h, st.p_final, st.seed) if st.p_final > 0 else h
        wp, bp = padded_head_weight(w, b, Np)
        logits = ops.gemm(hd, wp, M, Np, H, bias=bp, out_f32=True)
        loss, nll, lp, alpha = ops.ctc_fwd(logits, Np, g.Tp, st.targets, st.state_lens, st.target_lens, g.B, g.T, V,
                                           blank=st.blank, reduction=st.reduction, zero_infinity=st.zero_infinity)
        return (loss.reshape(()), logits, lp, hd), SimpleNamespace(hd=hd, wp=wp, logits=logits, alpha=alpha, nll=nll, V=V, Np=Np)

    def bwd(self, s, st, params, h, gloss):
        g, M, H = st.g, st.g.M, s.hd.shape[1]
        gl = torch.ones(1, device=s.hd.device, dtype=torch.float32) if gloss is None else gloss.float().reshape(1).contiguous()
        dlog = ops.ctc_bwd(s.logits, s.Np, g.Tp, st.targets, st.state_lens, st.target_lens, g.B, g.T, s.V, s.alpha, s.nll, gl,
                           blank=st.blank, reduction=st.reduction, zero_infinity=st.zero_infinity, ldd=s.Np)
        (dh, dw, db), = padded_linear_bwd(M, H, (dlog, s.wp, s.hd))
        if st.p_final > 0:
            dh = ops.dropout(dh, st.p_final, st.seed)
        return dh, dw[:s.V], db[:s.V]

    def result(self, outs, g, params):
        loss, logits, log_probs, hd = outs
        return {"loss": loss, "phoneme_logits": logits.view(g.B, g.Tp, -1)[:, :g.T, :params[0].shape[0]], "log_probs": log_probs,
                "hidden_states": hd.view(g.B, g.Tp, -1)[:, :g.T]}

    # ---- graph runners
    def static_targets(self, model, g, batch, dev):
        return {"targets": torch.full(tuple(batch["phoneme_labels"].shape), -100, device=dev, dtype=torch.int32),
                "state_lens": torch.zeros(g.B, device=dev, dtype=torch.int32),
                "target_lens": torch.zeros(g.B, device=dev, dtype=torch.int32)}

    def set_batch(self, b, batch):
        """Wav2Vec2_PR batch (input_values, input_lengths, phoneme_labels with -100 padding, models/w2v2_pr.py:40-70).  The label
        block may be narrower than the one the graphs were captured with (padded with -100), never wider."""
        labels = b.targets["targets"]
        lens_cpu = batch["input_lengths"].detach().cpu().long().reshape(-1)
        sl = hostlogic.feat_extract_output_lengths(lens_cpu, b.cfg.conv_kernel, b.cfg.conv_stride)
        lab = batch["phoneme_labels"]
        if lab.shape[0] != labels.shape[0] or lab.shape[1] > labels.shape[1]:
            raise ValueError(f"label block {tuple(lab.shape)} does not fit the captured {tuple(labels.shape)}")
        b.audio.copy_(batch["input_values"].float(), non_blocking=True)
        b.lens.copy_(sl.clamp(min=1, max=b.g.T).to(torch.int32), non_blocking=True)
        b.targets["state_lens"].copy_(sl.to(torch.int32), non_blocking=True)
        b.targets["target_lens"].copy_(hostlogic.ctc_target_lengths(lab).to(torch.int32), non_blocking=True)
        if lab.shape[1] < labels.shape[1]:
            labels.fill_(-100)
        labels[:, :lab.shape[1]].copy_(lab.to(torch.int32), non_blocking=True)

    def pad_batch(self, batch, Sb, Tb, label_bucket):
        lab = batch["phoneme_labels"]
        wl = -(-lab.shape[1] // label_bucket) * label_bucket     # the next multiple of label_bucket
        return dict(super().pad_batch(batch, Sb, Tb, label_bucket), phoneme_labels=_pad_to(lab, wl, -100))

    def cache_key(self, padded):
        return (padded["phoneme_labels"].shape[1],)


# ------------------------------------------------------------------------------------------------- Force_APTAI
# field -> parameter of the model; the field order is the gradient order
_FORCE_PARAMS = dict(fl_w="frame_lin.weight", fl_b="frame_lin.bias", emb_w="phn_emb_layer.weight", q_w="xatt.q.weight", q_b="xatt.q.bias",
                     k_w="xatt.k.weight", k_b="xatt.k.bias", ln_w="xatt.layer_norm.weight", ln_b="xatt.layer_norm.bias",
                     wih0="rnn.lstm.weight_ih_l0", whh0="rnn.lstm.weight_hh_l0", bih0="rnn.lstm.bias_ih_l0", bhh0="rnn.lstm.bias_hh_l0",
                     wih1="rnn.lstm.weight_ih_l0_reverse", whh1="rnn.lstm.weight_hh_l0_reverse", bih1="rnn.lstm.bias_ih_l0_reverse",
                     bhh1="rnn.lstm.bias_hh_l0_reverse", l0_w="rnn.linear.0.weight", l0_b="rnn.linear.0.bias", l3_w="rnn.linear.3.weight",
                     l3_b="rnn.linear.3.bias")
ForceParams = namedtuple("ForceParams", list(_FORCE_PARAMS))


class ForceHead:
    """Everything of Force_APTAI.forward after the encoder, fp32 on the device (csrc/force.hip, lstm.hip, ctc.hip): the blocks of
    aptai_amd.modules in one chain, `q` inside cat[:, 128:] at pitch 256 and the forward-sum rows written by the softmax kernel.
    outs = (loss, tv_loss, align_loss, tvs, frame_phns, att_log, att_out, hout, align).  The input `ac` gets no gradient."""
    clones = 0                              # fwd itself clones the losses

    def params(self, model):
        return ForceParams(*map(model.get_parameter, _FORCE_PARAMS.values()))

    def state(self, model, g, seed, training, ids, nlen, frame_lens, tv_targets):
        """All device tensors; no synchronisation."""
        dev = ids.device
        if tv_targets is None:
            tv_targets = torch.full((g.B, g.T, model.rnn.linear[3].weight.shape[0]), -100.0, device=dev)
        consts = model._consts(g.B, dev)
        # models/modules.py:209-212: the batch-1 branch runs the LSTM unpacked over ALL frames
        rnn_lens = consts["full_T"](g.T) if g.B == 1 else frame_lens
        N = model.max_phn_seq_len
        return SimpleNamespace(g=g, ids=ids, nphn=N, pe=model.pe_phn.pe.reshape(N, -1).contiguous(), taps=model.tv_lowpass.taps(),
                               p_hid=model.hidden_drop if training else 0.0, p_rnn=model.rnn_drop if training else 0.0,
                               seed=_seed(*seed, _FORCE_HEADS_STREAM), tv_tgt=tv_targets.contiguous(), fs_targets=consts["fs_targets"],
                               frame_lens=frame_lens, rnn_lens=rnn_lens, text_lens=nlen, vocab_sizes=nlen + 1, readout=model._readout(),
                               mono_targets=consts["mono_targets"])

    def fwd(self, ac, params, st):
        P = ForceParams._make(params)
        g = st.g
        B, Tp, T, M = g.B, g.Tp, g.T, g.M
        dev = ac.device
        N = st.nphn                                        # phoneme slots per utterance (Force_APTAI.max_phn_seq_len, 60 by default)
        ld = ops.fs_row_pitch(N)                           # floats per forward-sum row: 64 up to 63 slots, 256 at 255
        s = SimpleNamespace()
        s.phn = ops.embed_pe_fwd(st.ids, P.emb_w, st.pe, N, st.p_hid, _seed(st.seed, 1))                      # [B*N][128]
        fh = ops.linear_f32(ac, P.fl_w, P.fl_b, rows=M)                                                       # [M][128]
        s.fhd = ops.dropout_f32(fh, st.p_hid, _seed(st.seed, 2))
        s.cat = torch.empty((M, 256), device=dev, dtype=torch.float32)
        q = s.cat[:, 128:]
        ops.linear_f32(s.fhd, P.q_w, P.q_b, out=q, ldc=256)
        s.k = ops.linear_f32(s.phn, P.k_w, P.k_b)                                                              # [B*N][128]
        # forward-sum (CTC) input rows [blank = -1 | att_log | 0], written by the softmax kernel
        s.pad = torch.empty((M, ld), device=dev, dtype=torch.float32)
        s.energy, s.att, s.att_log, s.align = xatt_core_fwd(q, 256, s.k, st.ids, B, Tp, N, 128, s.cat, fs_rows=s.pad)
        s.att_out, s.lm, s.lr = ops.layernorm_f32_fwd(s.cat, P.ln_w, P.ln_b)
        # rows in the LSTM kernels' gate-interleaved order (csrc/lstm.hip: column dir * 1024 + unit * 4 + gate of xproj / gates / dgates)
        perm = ops.lstm_gate_perm(dev)[0]
        s.wih = torch.cat([P.wih0, P.wih1])[perm].contiguous()                                                # [2048][256]
        bsum = torch.cat([P.bih0 + P.bhh0, P.bih1 + P.bhh1])[perm].contiguous()
        xproj = ops.linear_f32(s.att_out, s.wih, bsum)                                                         # [M][2048]
        s.whh = torch.stack([P.whh0, P.whh1]).contiguous()                                                     # [2][1024][256]
        s.hout, s.gates, s.cst = ops.lstm_fwd(xproj, s.whh, st.rnn_lens, B, Tp, T)
        h1 = ops.linear_f32(s.hout, P.l0_w, P.l0_b)
        s.h1a = ops.tanh_dropout_fwd(h1, st.p_rnn, _seed(st.seed, 3))
        tv_raw = ops.linear_f32(s.h1a, P.l3_w, P.l3_b)                                                         # [M][9]
        n_tv = P.l3_w.shape[0]
        s.tvs = torch.empty((B, T, n_tv), device=dev, dtype=torch.float32)
        ops.lowpass_fir(tv_raw, n_tv, Tp, st.taps, s.tvs, n_tv, T, B, T, T, n_tv, n_tv, frame_lens=getattr(g, "fir_lens", None))
        s.dummy_logits = torch.zeros((M, 1), device=dev, dtype=torch.float32)
        s.dummy_phn = torch.zeros((B, T), device=dev, dtype=torch.int64)
        s.sc, _ = ops.aptai_loss_fwd(s.tvs, st.tv_tgt, s.dummy_logits, 1, Tp, s.dummy_phn, B, T, n_tv, 1, 1.0, 0.0, want_pred=False)
        s.fs = (s.pad, Tp, st.fs_targets, st.frame_lens, st.text_lens, st.vocab_sizes, B, T, N)
        s.fs_loss, s.nll, _, s.alpha = fwd_sum_ctc(*s.fs)
        tv_loss = s.sc[1].clone()
        align_loss = s.fs_loss.reshape(()).clone()
        loss = 0.4 * tv_loss + 0.6 * align_loss
        align = s.align
        if getattr(st, "readout", "argmax") == "monotonic":
            # Viterbi read-out of the trellis the forward-sum loss trains (topology 1: every phoneme owns >= 1 frame, no jumps back):
            # the att_log rows sit at column 1 of the forward-sum rows.  More phonemes than frames -> the argmax indices stay.
            ft, _, score, _ = ops.ctc_viterbi(s.pad[:, 1:], ld, Tp, st.mono_targets, st.frame_lens, st.text_lens, B, T, N,
                                              topology="monotonic", vocab_sizes_i32=st.text_lens, want_token_score=False)
            align = s.align.clone()
            align[:, :T] = torch.where((ft >= 0) & torch.isfinite(score)[:, None], ft.long(), s.align[:, :T])
        frame_phns = ops.gather_alignment(st.ids, align, st.frame_lens, B, Tp, N)
        return (loss, tv_loss, align_loss, s.tvs, frame_phns, s.att_log, s.att_out, s.hout, align), s

    def bwd(self, s, st, params, ac, gloss):
        """(None, the gradients in the order of ForceParams), collected by field name."""
        P = ForceParams._make(params)
        g = st.g
        B, Tp, T, M, H = g.B, g.Tp, g.T, g.M, ac.shape[1]
        n_tv, N = P.l3_w.shape[0], st.nphn
        ld = ops.fs_row_pitch(N)
        if B * N > 8192:
            raise ValueError(f"Force_APTAI backward: batch {B} x max_phn_seq_len {N} = {B * N} phoneme rows, the embedding gradient "
                             "kernel (aptai_embed_bwd) takes 8192 at most")
        gl = torch.ones(1, device=ac.device, dtype=torch.float32) if gloss is None else gloss.float().reshape(1)
        d = {}
        # ---- TV branch
        norm = getattr(st, "norm_scalars", None)             # data parallel: global valid TV count / world (dp.GlobalLossNorm)
        d_tvs, _ = ops.aptai_loss_bwd(s.tvs, st.tv_tgt, s.dummy_logits, 1, Tp, s.dummy_phn, B, T, n_tv, 1, 1.0, 0.0,
                                      norm() if norm is not None else s.sc, (0.4 * gl).contiguous(), ldd=8)
        d_tvraw = torch.empty((M, n_tv), device=ac.device, dtype=torch.float32)
        ops.lowpass_fir(d_tvs, n_tv, T, st.taps, d_tvraw, n_tv, Tp, B, T, Tp, n_tv, n_tv)
        d["l3_w"], d["l3_b"] = ops.linear_f32_dwdb(d_tvraw, s.h1a, M)
        dh1 = ops.tanh_dropout_bwd(s.h1a, ops.linear_f32_dx(d_tvraw, P.l3_w, M), st.p_rnn, _seed(st.seed, 3))
        d["l0_w"], d["l0_b"] = ops.linear_f32_dwdb(dh1, s.hout, M)
        dhout = ops.linear_f32_dx(dh1, P.l0_w, M)
        dgates = ops.lstm_bwd(dhout, s.whh, st.rnn_lens, s.gates, s.cst, B, Tp, T)                              # [M][2048]
        dwih, dbg = ops.linear_f32_dwdb(dgates, s.att_out, M)
        dwhh0, dwhh1 = lstm_whh_grads(dgates, s.hout, M)
        datt_out = ops.linear_f32_dx(dgates, s.wih, M)
        # the four products above have the gate axis in the kernels' interleaved order: back to torch's gate-major rows
        inv = ops.lstm_gate_perm(ac.device)[1]
        dwih, dbg = dwih[inv], dbg[inv]
        d.update(wih0=dwih[:1024], whh0=dwhh0[inv[:1024]], bih0=dbg[:1024], bhh0=dbg[:1024],
                 wih1=dwih[1024:], whh1=dwhh1[inv[:1024]], bih1=dbg[1024:], bhh1=dbg[1024:])
        dcat, d["ln_w"], d["ln_b"] = ops.layernorm_f32_bwd(datt_out, s.cat, s.lm, s.lr, P.ln_w)
        # ---- cross attention
        def d_raw_of(d_att):                   # the forward-sum gradient reaches att_log: columns 1..N of its rows, in place
            dpad = fwd_sum_ctc(*s.fs, grad=(s.alpha, s.nll, (0.6 * gl).contiguous()))
            return ops.xattn_softmax_bwd(s.att, s.att_log, d_att, dpad[:, 1:], ld_dattlog=ld)
        dq, dk = xatt_core_bwd(dcat, s.cat[:, 128:], 256, s.k, s.att, B, Tp, N, 128, d_raw_of)
        d["q_w"], d["q_b"] = ops.linear_f32_dwdb(dq, s.fhd, M)
        dfhd = ops.linear_f32_dx(dq, P.q_w, M)
        d["k_w"], d["k_b"] = ops.linear_f32_dwdb(dk, s.phn, B * N)
        dphn = ops.linear_f32_dx(dk, P.k_w, B * N)
        d["emb_w"] = ops.embed_bwd(st.ids, dphn, P.emb_w.shape[0], st.p_hid, _seed(st.seed, 1))
        dfh = ops.dropout_f32(dfhd, st.p_hid, _seed(st.seed, 2))
        dfl_wT = ops.sgemm(ac, 1, H, dfh, 128, 1, H, 128, M)                 # [H][128]: ac may be bf16, which only the A operand takes
        d["fl_b"] = ops.colsum_f32(dfh, M, 128)
        d["fl_w"] = dfl_wT.t().contiguous()
        return (None,) + tuple(ForceParams(**d))

    def result(self, outs, g, params):
        return dict(zip(("loss", "tv_loss", "align_loss", "tvs_pred", "frame_phns"), outs))
