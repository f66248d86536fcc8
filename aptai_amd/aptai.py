"""``APTAI`` — drop-in for the reference's models/aptai.py:14-182 on MI355X.

Same constructor, ``forward(epoch, **batch)`` signature, returned dict keys, inference helper and state-dict
keys (``wav2vec2.*``, ``tv_head.2.*``, ``phn_head.2.*``, ``tv_lowpass.lowpass.weight``).  Differences, all
parameterised with the reference's value as default: the head width follows ``pretrain_cfg.hidden_size`` (the
reference hard-codes 1024, models/aptai.py:46,54) and the tapped hidden state is the last one (the reference
hard-codes ``hidden_states[24]``, :81 — identical for its 24-layer backbone); ``n_tv`` (9) and ``n_phn`` (46)
are arguments so BASELINE.json's 12-track variant can be benchmarked.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hostlogic, longform, task_heads
from .hostlogic import TV_NAMES
from .modules import LowPassFilterLayer
from .wav2vec2 import Wav2Vec2Model, batch_invariant_scope


class APTAI(nn.Module):
    task_head = task_heads.AptaiHead()       # everything after the encoder, for this class and the graph runners (task_heads.py)
    # opt-in: eval-mode calls return for every row what the utterance gets at batch size 1 (Wav2Vec2Model.batch_invariant for the
    # encoder, the low-pass filter padded at each row's own length); training-mode calls are what they were
    batch_invariant = False

    def __init__(self, device, vocab, huggingface_model_id, pretrain_cfg, cache_dir, phn_drop=0.1, tv_drop=0.1,
                 freeze_feature_encoder=True, n_tv=9, n_phn=46):
        super().__init__()
        self.device = device
        self.vocab = vocab
        self.huggingface_model_id = huggingface_model_id
        self.pretrain_cfg = pretrain_cfg
        self.n_tv, self.n_phn = n_tv, n_phn
        if n_tv > task_heads._PADN or n_phn > task_heads._PADN:
            raise ValueError("head widths above 64 are not built")

        self.wav2vec2 = Wav2Vec2Model.from_pretrained(huggingface_model_id, config=pretrain_cfg, cache_dir=cache_dir).to(device)
        self.wav2vec2.gradient_checkpointing_enable()
        if freeze_feature_encoder:
            self.wav2vec2.freeze_feature_encoder()
        H = self.wav2vec2.config.hidden_size

        self.dp_loss_norm = None       # aptai_amd.dp.GlobalLossNorm under data parallelism: masked means over the global batch
        self.tv_head = nn.Sequential(nn.Dropout(tv_drop), nn.Tanh(), nn.Linear(H, n_tv))
        self.tv_lowpass = LowPassFilterLayer(self.device, 10, 49, n_tv)
        self.phn_head = nn.Sequential(nn.Dropout(phn_drop), nn.LeakyReLU(), nn.Linear(H, n_phn))

    def _heads(self, w2v2_out, tv_targets, phn_targets):
        g = w2v2_out._geom
        h = w2v2_out._flat_last                       # hidden_states[-1] == hidden_states[24] for the large backbone
        st = self.task_head.state(self, g, (self.wav2vec2.base_seed, self.wav2vec2._step), self.training, tv_targets, phn_targets)
        if self.dp_loss_norm is not None and self.training:
            self.dp_loss_norm.begin(st.tv_tgt, st.phn_tgt)       # 2-scalar all-reduce under the head GEMMs
            st.norm_scalars = self.dp_loss_norm.scalars           # resolved (waited for) in the backward
        return task_heads.HeadFn.apply(self.task_head, h, st, *self.task_head.params(self))

    def forward(self, epoch, audio_inputs, audio_lengths, phn_frames_49hz, LA=None, LP=None, JA=None, TTCL=None,
                TTCD=None, TMCL=None, TMCD=None, TBCL=None, TBCD=None, **extra_tvs):
        tracks = [LA, LP, JA, TTCL, TTCD, TMCL, TMCD, TBCL, TBCD]
        tracks = [t for t in tracks if t is not None] + [extra_tvs[k] for k in sorted(extra_tvs)]
        if len(tracks) != self.n_tv:
            raise ValueError(f"expected {self.n_tv} TV tracks, got {len(tracks)}")
        tv_targets = torch.stack(tracks, dim=-1).float()                       # models/aptai.py:67-70
        with batch_invariant_scope(self.wav2vec2, self.batch_invariant and not self.training):
            w2v2_out = self.wav2vec2(audio_inputs, attention_mask=audio_lengths[:, None], return_dict=True,
                                     output_hidden_states=True)
        return self.task_head.result(self._heads(w2v2_out, tv_targets, phn_frames_49hz), w2v2_out._geom, None)

    def get_config(self):
        return {'device': self.device, 'vocab': self.vocab, 'huggingface_model_id': self.huggingface_model_id,
                'pretrain_cfg': self.pretrain_cfg}

    def get_aptai_output(self, wav):
        """models/aptai.py:125-179."""
        self.eval()
        device = next(self.parameters()).device
        with torch.no_grad():
            if type(wav) is torch.Tensor:
                wav = wav[0]
            wav_input = torch.unsqueeze(torch.Tensor(wav), dim=0).to(device)
            wav_len = torch.unsqueeze(torch.LongTensor([len(wav)]), dim=0).to(device)
            with batch_invariant_scope(self.wav2vec2, self.batch_invariant):
                w2v2_out = self.wav2vec2(wav_input, attention_mask=wav_len[:, None], return_dict=True, output_hidden_states=True)
            _, _, _, tvs, pred, logits = self._heads(w2v2_out, None, None)
            g = w2v2_out._geom
            phn_logits = logits.view(g.B, g.Tp, -1)[:, :g.T, :self.n_phn]
            phn_probs = F.softmax(phn_logits, dim=-1)
            tvs_out = tvs.squeeze(dim=0).cpu().numpy()
            names = TV_NAMES if self.n_tv == 9 else tuple(f"TV{i}" for i in range(self.n_tv))
            tvs_pred_dict = {n: [row[i] for row in tvs_out] for i, n in enumerate(names)}
            return {
                'phn_fc_probs': phn_probs.permute(2, 1, 0).squeeze(dim=0).cpu().numpy(),      # the reference's `.T` on (1, T, C): (C, T, 1)
                'phn_fc_logits': phn_logits.squeeze(dim=0).cpu().numpy(),
                'phn_fc_pred': pred.squeeze(dim=0).cpu().numpy(),
                'tvs_pred': tvs_pred_dict,
            }

    def get_aptai_outputs(self, wavs):
        """Batched sibling of `get_aptai_output`: a list of 1-D waveforms -> a list of dicts with the same keys and per-utterance
        shapes, from ONE batch-invariant forward (the waveforms zero-padded to the longest; `batch_invariant` is switched on for
        the call and put back), so every entry is what `get_aptai_output` returns for that waveform up to what the batch size
        does to the GEMM plans ("Batch-invariant inference")."""
        self.eval()
        device = next(self.parameters()).device
        wavs = [torch.as_tensor(np.asarray(w), dtype=torch.float32).reshape(-1) for w in wavs]
        if not wavs:
            return []
        lens = [int(w.numel()) for w in wavs]
        cfg = self.wav2vec2.config
        frames = [hostlogic.conv_layer_lengths(n, cfg.conv_kernel, cfg.conv_stride)[-1] for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a waveform of {min(lens)} samples is shorter than the receptive field of the feature encoder")
        audio = torch.zeros((len(wavs), max(lens)), dtype=torch.float32)
        for b, w in enumerate(wavs):
            audio[b, :lens[b]] = w
        names = TV_NAMES if self.n_tv == 9 else tuple(f"TV{i}" for i in range(self.n_tv))
        with torch.no_grad(), batch_invariant_scope(self.wav2vec2, True):
            wav_len = torch.tensor(lens, dtype=torch.long, device=device)
            w2v2_out = self.wav2vec2(audio.to(device), attention_mask=wav_len[:, None], return_dict=True, output_hidden_states=True)
            _, _, _, tvs, pred, logits = self._heads(w2v2_out, None, None)
            g = w2v2_out._geom
            phn_logits = logits.view(g.B, g.Tp, -1)[:, :g.T, :self.n_phn]
            probs, phn_logits = F.softmax(phn_logits, dim=-1).cpu().numpy(), phn_logits.cpu().numpy()
            tvs, pred = tvs.cpu().numpy(), pred.cpu().numpy()
        out = []
        for b, T in enumerate(frames):
            out.append({
                'phn_fc_probs': probs[b:b + 1, :T].transpose(2, 1, 0),                                  # (C, T, 1) as get_aptai_output
                'phn_fc_logits': phn_logits[b, :T],
                'phn_fc_pred': pred[b, :T],
                'tvs_pred': {n: [row[i] for row in tvs[b, :T]] for i, n in enumerate(names)},
            })
        return out

    def get_aptai_output_long(self, wav, window_frames=499, hop_frames=399, trim_frames=25, ramp="linear", windows_per_forward=16):
        """`get_aptai_output` for a recording longer than the clips the model was trained on: the keys and shapes of that helper,
        from overlapped windows of `window_frames` encoder frames every `hop_frames` (hostlogic.long_form_plan), stitched on the
        device - `get_aptai_outputs_long` of one recording.  The waveform is taken as given: a caller who normalises does so over
        the whole recording, never per window."""
        return self.get_aptai_outputs_long([wav], window_frames, hop_frames, trim_frames, ramp, windows_per_forward)[0]

    def get_aptai_outputs_long(self, wavs, window_frames=499, hop_frames=399, trim_frames=25, ramp="linear", windows_per_forward=16):
        """`get_aptai_outputs` over recordings of any length.  The windows of ALL recordings run through the eval-mode,
        batch-invariant forward in groups of `windows_per_forward` (what bounds the encoder's memory; a window's result does not
        depend on its group), the filtered trajectories and the head logits of the windows are stitched per recording
        (aptai_stitch_windows: `ramp` = "linear" fades over the overlap less `trim_frames` at either end, "cut" switches in its
        middle), `phn_fc_pred` is the argmax of the stitched logits and `phn_fc_probs` their softmax; ONE device->host transfer.  A
        recording of at most `window_frames` frames is one window: `get_aptai_output` with `batch_invariant` on ("Long
        recordings")."""
        self.eval()
        device = next(self.parameters()).device
        if not len(wavs):
            return []
        run = longform.LongFormRun(wavs, self.wav2vec2, device, window_frames, hop_frames, trim_frames, ramp)
        n_tv, n_phn = self.n_tv, self.n_phn
        tv_all = logits_all = None
        with torch.no_grad(), batch_invariant_scope(self.wav2vec2, True):
            for first, rows in run.groups(windows_per_forward):
                audio, lens = run.gather(first, rows)
                w2v2_out = self.wav2vec2(audio, attention_mask=lens[:, None], return_dict=True, output_hidden_states=True)
                _, _, _, tvs, _, logits = self._heads(w2v2_out, None, None)
                g = w2v2_out._geom
                tv_all, logits_all = run.collect(tv_all, tvs, first, rows), run.collect(logits_all, logits, first, rows)
            tv, _ = run.stitch(tv_all, n_tv, g.T, n_tv, want_argmax=False)                   # [W][T][n_tv] as the filter wrote them
            phn_logits, pred = run.stitch(logits_all, logits_all.shape[1], g.Tp, n_phn)      # [W * Tp][64], the first n_phn columns
            host = torch.cat([tv, phn_logits, F.softmax(phn_logits, dim=-1), pred[:, None].float()], dim=1).cpu().numpy()
        names = TV_NAMES if n_tv == 9 else tuple(f"TV{i}" for i in range(n_tv))
        out = []
        for r0, T in zip(run.row_start, run.frames):
            rows = host[r0:r0 + T]
            tvs, lg, probs = rows[:, :n_tv], rows[:, n_tv:n_tv + n_phn], rows[:, n_tv + n_phn:n_tv + 2 * n_phn]
            out.append({
                'phn_fc_probs': np.ascontiguousarray(probs)[None].transpose(2, 1, 0),                      # (C, T, 1) as get_aptai_output
                'phn_fc_logits': np.ascontiguousarray(lg),
                'phn_fc_pred': rows[:, -1].astype(np.int64),                                               # an index below 64: exact in fp32
                'tvs_pred': {n: [row[i] for row in tvs] for i, n in enumerate(names)},
            })
        return out
