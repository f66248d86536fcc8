"""``Wav2Vec2_PR`` — drop-in for the reference's CTC phoneme recogniser (models/w2v2_pr.py:18-291) on MI355X.

Same constructor ``(pretrain_cfg, cache_dir, huggingface_model_id, vocab)``, ``forward(input_values, input_lengths,
phoneme_labels)`` dict, inference helpers and state-dict keys (``wav2vec2.*``, ``pr_head.*``).  The torchaudio package whose
flashlight beam-search decoder the reference calls (models/w2v2_pr.py:143-159) is not in the image, so parity with torchaudio
itself stays *unpinned* (SURVEY.md §8c).  Every decoder answers through one read-out (``_read_out``: tokens, timesteps and full
lengths per row, on the device, each row stopping at its own last frame under ``batch_invariant``); the default
``model.decoder = "best_path"`` is the frame argmax, repeats collapsed, blanks dropped (aptai_ctc_greedy_decode, csrc/ctc.hip).

``model.decoder = "flashlight"`` (opt-in) is the same kernel given the silence token ``'(...)'``: what the published decoder
sources say that call returns for the reference's settings, the best path FRAMED by the decoder's opening / closing silence,
timesteps as positions in the framed token row (oracle: hostlogic.ctc_bracketed_best_path; hostlogic.ctc_beam_search restates the
search itself and the CPU tests check the two against each other).  It is not the default because nothing in this image can pin
it and the reference-generated fixtures under tests/golden were made with a plain best-path stand-in.

``model.decoder = "beam"`` (opt-in) runs the published algorithm of that decoder on the device (aptai_ctc_beam_search,
csrc/decode.hip), pinned against its Python restatement hostlogic.ctc_beam_search: ``beam_options`` default to the reference's
call (beam 10, threshold 50, max-merge, 1-best) and also give what no closed form can: true prefix scores (``log_add``), token
beams, and through ``decode_nbest`` / ``predict_nbest`` n-best lists with per-token timesteps.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import hostlogic, longform, ops, task_heads
from .modules import _LinearFn
from .wav2vec2 import Wav2Vec2Model, _round_up, batch_invariant_scope


class Wav2Vec2_PR(nn.Module):
    """Wav2Vec2 model used as a phoneme recognizer."""

    # opt-in: eval-mode calls (forward in eval mode, force_align, get_embeddings, get_ctc_logits, ...) return for every row what the
    # utterance gets at batch size 1 - Wav2Vec2Model.batch_invariant for the encoder, and every decoder stops at each row's
    # own last frame.  Training-mode forwards are what they were.
    batch_invariant = False
    task_head = task_heads.CtcHead()         # everything after the encoder, for this class and the graph runners (task_heads.py)

    def __init__(self, pretrain_cfg, cache_dir, huggingface_model_id, vocab):
        super().__init__()
        self.cache_dir = cache_dir
        self.huggingface_model_id = huggingface_model_id
        self.pretrain_cfg = pretrain_cfg
        self.wav2vec2 = Wav2Vec2Model.from_pretrained(huggingface_model_id, config=pretrain_cfg, cache_dir=cache_dir)
        self.wav2vec2.gradient_checkpointing_enable()
        cfg = self.wav2vec2.config
        self.dropout = nn.Dropout(cfg.final_dropout)
        self.pr_head = nn.Linear(cfg.hidden_size, cfg.vocab_size)
        self.vocab = vocab

    # ------------------------------------------------------------------ training forward (models/w2v2_pr.py:40-88)
    def forward(self, input_values, input_lengths, phoneme_labels):
        """A row with fewer frames than its labels need (speed perturbation shortens the audio, not the transcript) has an infinite
        CTC loss; with `ctc_zero_infinity` (the training loop sets it) it counts as zero, loss and gradient."""
        with batch_invariant_scope(self.wav2vec2, self.batch_invariant and not self.training):
            outputs = self.wav2vec2(input_values, attention_mask=input_lengths[:, None], return_dict=True, output_hidden_states=True)
        w, head = self.wav2vec2, self.task_head
        st = head.state(self, outputs._geom, (w.base_seed, w._step), self.training, phoneme_labels,              # lengths as models/w2v2_pr.py:62-70
                        w._get_feat_extract_output_lengths(input_lengths), hostlogic.ctc_target_lengths(phoneme_labels))
        params = head.params(self)
        return head.result(task_heads.HeadFn.apply(head, outputs._flat_last, st, *params), outputs._geom, params)

    # ------------------------------------------------------------------ inference helpers
    def _logits_eval(self, audio_inputs, audio_lengths):
        """eval-mode encoder + pr_head (fp32 logits (B,T,V)); shared by every helper below.  Lengths as (B,) or (B, 1)."""
        lengths_2d = audio_lengths[:, None] if audio_lengths.dim() == 1 else audio_lengths
        with batch_invariant_scope(self.wav2vec2, self.batch_invariant and not self.training):
            out = self.wav2vec2(audio_inputs, attention_mask=lengths_2d, return_dict=True, output_hidden_states=True)
        g, h = out._geom, out._flat_last
        V, H = self.pr_head.weight.shape
        Np = _round_up(V, 64)

        # padded bf16 head weight: rebuilt only when the parameters moved (eval mode trusts Tensor._version, see _cached)
        h32 = out._flat_last_f32
        if h32 is not None and self.wav2vec2.encoder_precision in ("f32x3", "f32x6"):
            # exact inference pass: the head is an fp32 product too (fp32 matrix instruction), so the frame argmax of the decode
            # sees fp32 logits
            def build32():
                w32 = torch.zeros((Np, H), device=h.device, dtype=torch.float32)
                w32[:V] = self.pr_head.weight.detach()
                b32 = torch.zeros(Np, device=h.device, dtype=torch.float32)
                b32[:V] = self.pr_head.bias.detach()
                return w32, b32
            w32, b32 = self.wav2vec2._cached(("pr_head_eval32",), [self.pr_head.weight, self.pr_head.bias], build32)
            full = ops.linear_f32(h32, w32, b32)
            out._logits_full = full
            return out, full.view(g.B, g.Tp, Np)[:, :g.T, :V]
        wp, bp = self.wav2vec2._cached(("pr_head_eval",), [self.pr_head.weight, self.pr_head.bias],
                                       lambda: task_heads.padded_head_weight(self.pr_head.weight, self.pr_head.bias, Np))
        full = ops.gemm(h, wp, g.M, Np, H, bias=bp, out_f32=True)
        out._logits_full = full                                   # [B*Tp][Np] fp32: what the device decode reads
        return out, full.view(g.B, g.Tp, Np)[:, :g.T, :V]

    def _blank(self) -> int:
        return int(self.vocab.get('(blank)', 0)) if isinstance(self.vocab, dict) else 0

    decoder = "best_path"           # or "flashlight" (framed like the reference's decoder call) or "beam": module docstring
    # keywords of ops.ctc_beam_search for decoder = "beam"; the defaults are the reference's decoder call (models/w2v2_pr.py:144-153).
    # An instance's own dict may add "lm" (an ngram.NGramLM over the vocabulary) and "lm_weight": the token n-gram the reference
    # leaves at lm=None, fused into the search on the device; every decode of the model then uses it.
    beam_options = {"beam_size": 10, "beam_threshold": 50.0, "log_add": False, "nbest": 1}

    def _sil(self) -> int:
        if not (isinstance(self.vocab, dict) and '(...)' in self.vocab):
            raise ValueError("'flashlight', 'beam' and the n-best lists need the silence token '(...)' in the vocabulary (models/w2v2_pr.py:153)")
        return int(self.vocab['(...)'])

    def _beam_search(self, out, **options):
        """ops.ctc_beam_search over the logits of `out`, `beam_options` overridden by `options`: the five device tensors.  All
        frames of the padded batch are decoded, like the reference's decoder call; with batch_invariant each row stops at its own
        frame count (`input_lens`), which is what the utterance gets alone.  Nothing here synchronises host and device."""
        g, full = out._geom, out._logits_full
        opts = dict(self.beam_options)
        opts.update(options)
        return ops.ctc_beam_search(full, full.shape[1], g.Tp, g.B, g.T, self.pr_head.weight.shape[0], self._blank(), self._sil(),
                                   input_lens_i32=getattr(g, "fir_lens", None), **opts)

    def _read_out(self, out, max_n: int):
        """The decode of `decoder`, on the device: (tokens, timesteps int32 [B][max_n] zero-padded, n int32 [B] = full length, which
        may exceed max_n).  "best_path" / "flashlight": aptai_ctc_greedy_decode without / with the silence token (oracle:
        hostlogic.ctc_bracketed_best_path); "beam": the top hypothesis of `_beam_search`, whose rows and row lengths all three read."""
        if self.decoder == "beam":
            tokens, timesteps, n_tok, _, _ = self._beam_search(out, max_n=max_n)
            return tokens[:, 0].contiguous(), timesteps[:, 0].contiguous(), n_tok[:, 0].contiguous()
        if self.decoder not in ("best_path", "flashlight"):
            raise ValueError(f"Wav2Vec2_PR.decoder must be 'best_path', 'flashlight' or 'beam', not {self.decoder!r}")
        g, full = out._geom, out._logits_full
        return ops.ctc_greedy_decode(full, full.shape[1], g.Tp, g.B, g.T, self.pr_head.weight.shape[0], self._blank(), max_n,
                                     input_lens_i32=getattr(g, "fir_lens", None), want_timesteps=True,
                                     sil=self._sil() if self.decoder == "flashlight" else None)

    def _decode_device(self, out, max_n: int):
        """(tokens, n) of `_read_out`: the seam of Force_APTAI and the training script."""
        tokens, _, n = self._read_out(out, max_n)
        return tokens, n

    @staticmethod
    def _rows(tokens, timesteps, n, score=None):
        """Host view of decoded rows [R][max_n] with lengths [R] (and scores [R]): [(ids int64, timesteps int32, score | None)] in
        ONE device->host transfer (int32 values are exact in fp64)."""
        max_n = tokens.shape[1]
        packed = torch.cat([tokens.double(), timesteps.double(), n[:, None].double()] + ([] if score is None else [score[:, None]]),
                           dim=1).cpu().numpy()
        keep = np.minimum(packed[:, 2 * max_n].astype(np.int64), max_n)
        return [(r[:k].astype(np.int64), r[max_n:max_n + k].astype(np.int32), None if score is None else float(r[-1]))
                for r, k in zip(packed, keep)]

    @staticmethod
    def _ipa(vocab, idx):
        inv = {v: k for k, v in vocab.items()}
        return [inv.get(int(i), '?') for i in idx]

    def _decode(self, out):
        """Decoded id lists of the batch: the device decode + ONE host transfer."""
        return [idx for idx, _, _ in self._rows(*self._read_out(out, out._geom.T + 2))]

    def _nbest(self, audio_inputs, audio_lengths, options):
        self.eval()
        with torch.no_grad():
            out, _ = self._logits_eval(audio_inputs, audio_lengths)
            tokens, timesteps, n_tok, score, n_hyp = self._beam_search(out, **options)
            frame_lens = self.wav2vec2._get_feat_extract_output_lengths(audio_lengths.reshape(-1).to(tokens.device)).to(torch.int32)
            return {'tokens': tokens, 'timesteps': timesteps, 'n_tok': n_tok, 'score': score, 'n_hyp': n_hyp,
                    'frame_seq_lens': frame_lens}, out._geom.T

    def decode_nbest(self, audio_inputs, audio_lengths, **options):
        """n-best lists of the batch from the device beam search, whatever `decoder` is set to: `beam_options` overridden by
        `options` (beam_size, beam_size_token, beam_threshold, log_add, sil_score, nbest, max_n, lm, lm_weight:
        ops.ctc_beam_search).  Runs in eval mode without gradients.  Returns DEVICE tensors and never synchronises:
          tokens, timesteps int32 [B][nbest][max_n]  zero-padded; a timestep is the position in the framed token row (frame t -> t + 1)
          n_tok             int32 [B][nbest]         length of each hypothesis (0: the row has fewer hypotheses)
          score             fp64  [B][nbest]         best first; -inf where the row has fewer hypotheses
          n_hyp             int32 [B]
          frame_seq_lens    int32 [B]"""
        return self._nbest(audio_inputs, audio_lengths, options)[0]

    def predict_nbest(self, wav, vocab, **options):
        """`predict_phonemes_durations` for every hypothesis of the n-best list of ONE utterance, best first: a list of
        {'phn_seq_idx', 'phn_seq_ipa', 'phn_seq_dur', 'score'}.  One device->host transfer; a rank without hypothesis has no tokens."""
        wav, wav_input, wav_len = self._wav(wav)
        res, n_frames = self._nbest(wav_input, wav_len, options)
        frame_sec_ratio = len(wav) / n_frames / 16000
        return [{'phn_seq_idx': idx, 'phn_seq_ipa': self._ipa(vocab, idx), 'phn_seq_dur': [int(t) * frame_sec_ratio for t in ts],
                 'score': score}
                for idx, ts, score in self._rows(res['tokens'][0], res['timesteps'][0], res['n_tok'][0], res['score'][0]) if len(idx)]

    def get_embeddings_grad(self, audio_inputs, audio_lengths, vocab, intermediate_hidden, latter_hidden):
        """models/w2v2_pr.py:91-122: the encoder in whatever mode the module is in, WITH gradients (probing / saliency use):
        the last, an intermediate and a latter hidden state as (batch, feat, time), and `pr_head` applied to each of the three.
        `features_hidden` (the reference's separate `feature_extractor` pass, :93) is the conv stack's output (batch, 512, time).
        Gradients flow from every returned tensor into the encoder's trainable parameters and, when `audio_inputs.requires_grad`,
        into the waveform (`audio_inputs.grad`: saliency / attribution), `features_hidden` included."""
        out = self.wav2vec2(audio_inputs, attention_mask=audio_lengths[:, None], return_dict=True, output_hidden_states=True)
        g = out._geom
        W, bvec = self.pr_head.weight, self.pr_head.bias

        def head(h):                                       # nn.Linear on (B, T, H): differentiable, fp32 matrix instruction
            return _LinearFn.apply(h, W, bvec)
        last = out.last_hidden_state
        inter = out.hidden_states[intermediate_hidden]
        latter = out.hidden_states[latter_hidden]
        feats = out._features
        return {'features_hidden': None if feats is None else feats.view(g.B, g.Tp, -1)[:, :g.T].permute(0, 2, 1),
                'last_transf_hidden': last.permute(0, 2, 1),
                'phoneme_logits_last': head(last), 'phoneme_logits_inter': head(inter), 'phoneme_logits_latter': head(latter),
                'intermediate_hidden': inter.permute(0, 2, 1), 'latter_hidden': latter.permute(0, 2, 1)}

    def get_embeddings(self, audio_inputs, audio_lengths):
        """models/w2v2_pr.py:124-167 (the encoder runs ONCE: the reference's extra feature_extractor pass :129 only
        produced 'features_hidden', which no caller reads; it is returned as None)."""
        self.eval()
        with torch.no_grad():
            out, logits = self._logits_eval(audio_inputs, audio_lengths)
            frame_seq_lens = self.wav2vec2._get_feat_extract_output_lengths(audio_lengths)
            return {'features_hidden': None, 'last_transf_hidden': out.last_hidden_state.permute(0, 2, 1),
                    'phoneme_logits': logits.cpu().numpy().transpose(0, 2, 1), 'phn_pred_seq_idx': self._decode(out),
                    'frame_seq_lens': frame_seq_lens.cpu().numpy(), '_out': out}

    def _wav(self, wav):
        device = next(self.parameters()).device
        if type(wav) is torch.Tensor:
            wav = wav[0]
        wav_input = torch.unsqueeze(torch.Tensor(wav), dim=0).to(device)
        wav_len = torch.unsqueeze(torch.LongTensor([len(wav)]), dim=0).to(device)
        return wav, wav_input, wav_len

    def get_ctc_logits(self, wav):
        self.eval()
        with torch.no_grad():
            _, wav_input, wav_len = self._wav(wav)
            _, logits = self._logits_eval(wav_input, wav_len)
            return logits.squeeze(dim=0).cpu().numpy()

    def pred_phn_seq(self, wav, vocab):
        self.eval()
        with torch.no_grad():
            _, wav_input, wav_len = self._wav(wav)
            out, logits = self._logits_eval(wav_input, wav_len)
            idx = self._decode(out)[0]
            return {'phn_seq_idx': idx, 'phn_seq_ipa': self._ipa(vocab, idx)}

    def predict_phonemes_durations(self, wav, vocab):
        """models/w2v2_pr.py:191-235; timesteps = first frame of each emitted (non-blank, de-duplicated) label."""
        self.eval()
        with torch.no_grad():
            wav, wav_input, wav_len = self._wav(wav)
            out, logits = self._logits_eval(wav_input, wav_len)
            frame_sec_ratio = len(wav) / logits.size(1) / 16000
            (idx, ts, _), = self._rows(*self._read_out(out, logits.size(1) + 2))       # tokens AND timesteps in one transfer
            return {'phn_seq_idx': idx, 'phn_seq_ipa': self._ipa(vocab, idx), 'phn_seq_dur': [t * frame_sec_ratio for t in ts]}

    # ------------------------------------------------------------------ long recordings ("Long recordings")
    def _long(self, wavs, window_frames, hop_frames, trim_frames, ramp, windows_per_forward):
        """The stitched CTC logits of recordings of any length as `_read_out` takes them: (run, out) where `out._logits_full` is
        fp32 [n_rec * max_frames][Np] (one block of rows per recording, zeros beyond its frames and beyond the vocabulary) and
        `out._geom` says so (B = n_rec, T = Tp = max_frames, fir_lens = the frame counts).  The windows of all recordings run through
        `_logits_eval` with `batch_invariant` on, `windows_per_forward` at a time (longform.LongFormRun)."""
        self.eval()
        run = longform.LongFormRun(wavs, self.wav2vec2, next(self.parameters()).device, window_frames, hop_frames, trim_frames, ramp)
        prev, self.batch_invariant = self.batch_invariant, True
        try:
            with torch.no_grad():
                full_all = None
                for first, rows in run.groups(windows_per_forward):
                    audio, lens = run.gather(first, rows)
                    out, _ = self._logits_eval(audio, lens)
                    full_all = run.collect(full_all, out._logits_full, first, rows)
                Np = full_all.shape[1]
                stitched, _ = run.stitch(full_all, Np, out._geom.Tp, self.pr_head.weight.shape[0], per_recording_rows=True, ldo=Np,
                                         want_argmax=False)
        finally:
            self.batch_invariant = prev
        geom = SimpleNamespace(B=run.n_rec, T=run.max_frames, Tp=run.max_frames, fir_lens=run.frames_i32())
        return run, SimpleNamespace(_geom=geom, _logits_full=stitched)

    def get_ctc_logits_long(self, wav, window_frames=499, hop_frames=399, trim_frames=25, ramp="linear", windows_per_forward=16):
        """`get_ctc_logits` of a recording of any length: overlapped windows of `window_frames` encoder frames every `hop_frames`
        (hostlogic.long_form_plan), their logits stitched on the device (aptai_stitch_windows).  The waveform is taken as given."""
        run, out = self._long([wav], window_frames, hop_frames, trim_frames, ramp, windows_per_forward)
        return out._logits_full[:run.frames[0], :self.pr_head.weight.shape[0]].cpu().numpy()

    def pred_phn_seq_long(self, wav, vocab, window_frames=499, hop_frames=399, trim_frames=25, ramp="linear", windows_per_forward=16):
        """`pred_phn_seq` over the stitched logits: the decode of `decoder`, the recording as ONE row of its own frame count."""
        _, out = self._long([wav], window_frames, hop_frames, trim_frames, ramp, windows_per_forward)
        with torch.no_grad():
            idx = self._decode(out)[0]
        return {'phn_seq_idx': idx, 'phn_seq_ipa': self._ipa(vocab, idx)}

    def predict_phonemes_durations_long(self, wav, vocab, window_frames=499, hop_frames=399, trim_frames=25, ramp="linear",
                                        windows_per_forward=16):
        """`predict_phonemes_durations` over the stitched logits (same `frame_sec_ratio`: samples / frames / 16000)."""
        run, out = self._long([wav], window_frames, hop_frames, trim_frames, ramp, windows_per_forward)
        n_frames = run.frames[0]
        frame_sec_ratio = run.plans[0].n_samples / n_frames / 16000
        with torch.no_grad():
            (idx, ts, _), = self._rows(*self._read_out(out, n_frames + 2))
        return {'phn_seq_idx': idx, 'phn_seq_ipa': self._ipa(vocab, idx), 'phn_seq_dur': [t * frame_sec_ratio for t in ts]}

    # ------------------------------------------------------------------ forced alignment of a known transcript
    def force_align(self, audio_inputs, audio_lengths, phoneme_labels):
        """Hard alignment of KNOWN phoneme sequences to the frames, on the device (aptai_ctc_viterbi, CTC topology): what
        torchaudio.functional.forced_align does for a CTC recogniser (torchaudio is not in the image: *parity unpinned*).
        The batch has the layout of `forward`: waveforms, their lengths, labels padded with -100 (at most 255 per row).  Runs in
        eval mode without gradients, in the encoder precision that is set.  Returns DEVICE tensors and never synchronises:
          frame_token    int32 [B][T]     transcript position of each frame, -1 blank, -2 padding / no path
          frame_phns     int32 [B][T]     vocabulary ids: the label of the position, the blank id on blank frames, 0 beyond the length
          spans          int32 [B][L][2]  first and one-past-last frame of each position (-1, -1: none)
          score          fp32  [B]        log-probability of the path (-inf: the transcript does not fit the utterance)
          token_score    fp32  [B][L]     mean log-probability of each label over its span
          frame_seq_lens int32 [B]
        Tie rule and limits: include/aptai_hip.h; hostlogic.ctc_forced_align is the same contract in numpy."""
        self.eval()
        with torch.no_grad():
            out, _ = self._logits_eval(audio_inputs, audio_lengths)
            g, full = out._geom, out._logits_full                     # [B*Tp][Np] fp32 with its padded pitches
            dev = full.device
            V = self.pr_head.weight.shape[0]
            labels = phoneme_labels.to(dev).to(torch.int32)
            if labels.shape[1] == 0:
                labels = torch.full((g.B, 1), -100, device=dev, dtype=torch.int32)
            if labels.shape[1] > 255:
                raise ValueError(f"force_align: at most 255 labels per utterance (got rows of {labels.shape[1]})")
            labels = labels.contiguous()
            target_lens = (labels >= 0).sum(dim=-1).to(torch.int32)    # hostlogic.ctc_target_lengths, on the device
            frame_lens = self.wav2vec2._get_feat_extract_output_lengths(audio_lengths.reshape(-1).to(dev)).to(torch.int32).contiguous()
            blank = self._blank()
            ft, spans, score, token_score = ops.ctc_viterbi(full, full.shape[1], g.Tp, labels, frame_lens, target_lens, g.B, g.T, V,
                                                            blank=blank, topology="ctc")
            return {'frame_token': ft, 'frame_phns': self._frame_phns(labels, ft, blank), 'spans': spans, 'score': score,
                    'token_score': token_score, 'frame_seq_lens': frame_lens}

    @staticmethod
    def _frame_phns(labels, ft, blank):
        """Vocabulary id of every frame of an alignment: the label of its position, the blank id on blank frames, 0 beyond the length."""
        lab = torch.gather(labels, 1, ft.clamp(min=0).long())
        return torch.where(ft >= 0, lab, torch.where(ft == -1, blank, 0)).to(torch.int32)

    def align_phonemes_durations(self, wav, phn_seq_idx, vocab):
        """`predict_phonemes_durations` for a KNOWN phoneme sequence: start and end of every phoneme in seconds (same
        `frame_sec_ratio`), its mean log-probability, and a phoneme id for every frame (`phn_frames`: blank frames assigned by
        hostlogic.fill_blank_frames).  Raises ValueError when the sequence does not fit the utterance."""
        self.eval()
        with torch.no_grad():
            wav, wav_input, wav_len = self._wav(wav)
            idx = np.asarray(phn_seq_idx, dtype=np.int64).reshape(-1)
            res = self.force_align(wav_input, wav_len.reshape(-1), torch.as_tensor(idx[None].astype(np.int32)))
            n_frames = res['frame_token'].shape[1]
            frame_sec_ratio = len(wav) / n_frames / 16000
            score = float(res['score'][0].cpu())
            if not np.isfinite(score):
                raise ValueError(f"align_phonemes_durations: {len(idx)} phonemes do not fit the utterance's "
                                 f"{int(res['frame_seq_lens'][0].cpu())} frames (or a phoneme id is outside the vocabulary)")
            spans = res['spans'][0, :len(idx)].cpu().numpy()
            ft = res['frame_token'][0, :int(res['frame_seq_lens'][0].cpu())].cpu().numpy()
            filled = hostlogic.fill_blank_frames(ft)
            return {'phn_seq_idx': idx, 'phn_seq_ipa': self._ipa(vocab, idx),
                    'phn_start': [int(a) * frame_sec_ratio for a in spans[:, 0]],
                    'phn_end': [int(b) * frame_sec_ratio for b in spans[:, 1]],
                    'phn_score': res['token_score'][0, :len(idx)].cpu().numpy().tolist(), 'score': score,
                    'phn_frames': [int(idx[k]) if k >= 0 else self._blank() for k in filled]}

    # ------------------------------------------------------------------ forced alignment of long recordings
    def _force_align_long(self, wavs, phoneme_seqs, window_frames, hop_frames, trim_frames, ramp, windows_per_forward):
        """(run, result dictionary) of `force_align_long`: one `_long` pass for all recordings, one wide Viterbi over its rows."""
        seqs = [np.asarray(q, dtype=np.int64).reshape(-1) for q in phoneme_seqs]
        if len(seqs) != len(wavs):
            raise ValueError(f"force_align_long: {len(wavs)} recordings but {len(seqs)} phoneme sequences")
        cap = ops.CTC_VITERBI_WIDE_MAX_LABELS
        if max((len(q) for q in seqs), default=0) > cap:
            raise ValueError(f"force_align_long: at most {cap} labels per recording (got {max(len(q) for q in seqs)})")
        run, out = self._long(wavs, window_frames, hop_frames, trim_frames, ramp, windows_per_forward)
        with torch.no_grad():
            full = out._logits_full                                   # [n_rec * max_frames][Np] fp32
            n, ldt = run.n_rec, max([len(q) for q in seqs] + [1])
            host = np.full(n * ldt + n, -100, dtype=np.int32)         # label rows, then their lengths: one upload
            for r, q in enumerate(seqs):
                host[r * ldt:r * ldt + len(q)] = q
                host[n * ldt + r] = len(q)
            both = torch.from_numpy(host).to(full.device)
            labels, target_lens = both[:n * ldt].view(n, ldt), both[n * ldt:]
            frame_lens = run.frames_i32()
            blank = self._blank()
            ft, spans, score, token_score = ops.ctc_viterbi_wide(full, full.shape[1], run.max_frames, labels, frame_lens, target_lens, n,
                                                                 run.max_frames, self.pr_head.weight.shape[0], blank=blank)
            return run, {'frame_token': ft, 'frame_phns': self._frame_phns(labels, ft, blank), 'spans': spans, 'score': score,
                         'token_score': token_score, 'frame_seq_lens': frame_lens}

    def force_align_long(self, wavs, phoneme_seqs, window_frames=499, hop_frames=399, trim_frames=25, ramp="linear",
                         windows_per_forward=16):
        """`force_align` for recordings of any length against their whole transcripts: `wavs` is a list of 1-D waveforms,
        `phoneme_seqs` one id sequence per recording (at most ops.CTC_VITERBI_WIDE_MAX_LABELS = 8191 labels, ValueError beyond).
        The windows run as in the other `*_long` helpers (same plan arguments, precisions and refusals), their logits are stitched
        on the device and aptai_ctc_viterbi_wide aligns each recording's row block to its transcript: same contract and tie rule as
        `force_align`, no T^2 attention over the recording and no limit of 255 labels.  Eval mode, no gradients.  Returns the
        dictionary of `force_align` as DEVICE tensors, never synchronising: frame_token / frame_phns int32 [n][max frames], spans
        int32 [n][L][2], score fp32 [n], token_score fp32 [n][L], frame_seq_lens int32 [n] = the recordings' frame counts.
        hostlogic.long_form_force_align is the same in numpy.  Accuracy at the seams and parity with torchaudio's forced_align
        are unmeasured (no trained checkpoint and no torchaudio here)."""
        return self._force_align_long(wavs, phoneme_seqs, window_frames, hop_frames, trim_frames, ramp, windows_per_forward)[1]

    def align_phonemes_durations_long(self, wav, phn_seq_idx, vocab, **plan):
        """`align_phonemes_durations` of a recording of any length (`plan`: the keywords of `force_align_long`; same
        `frame_sec_ratio` as `predict_phonemes_durations_long`: samples / frames / 16000).  One device->host transfer.  Raises
        ValueError when the sequence does not fit the recording."""
        idx = np.asarray(phn_seq_idx, dtype=np.int64).reshape(-1)
        keys = ("window_frames", "hop_frames", "trim_frames", "ramp", "windows_per_forward")
        unknown = sorted(set(plan) - set(keys))
        if unknown:
            raise TypeError(f"align_phonemes_durations_long: unknown keyword(s) {unknown}")
        args = dict(window_frames=499, hop_frames=399, trim_frames=25, ramp="linear", windows_per_forward=16)
        args.update(plan)
        run, res = self._force_align_long([wav], [idx], *(args[k] for k in keys))
        n_frames, n = run.frames[0], len(idx)
        frame_sec_ratio = run.plans[0].n_samples / n_frames / 16000
        with torch.no_grad():                                         # int32 and fp32 values are exact in fp64
            packed = torch.cat([res['frame_token'][0, :n_frames].double(), res['spans'][0, :n].reshape(-1).double(),
                                res['token_score'][0, :n].double(), res['score'][:1].double()]).cpu().numpy()
        score = float(packed[-1])
        if not np.isfinite(score):
            raise ValueError(f"align_phonemes_durations_long: {n} phonemes do not fit the recording's {n_frames} frames "
                             f"(or a phoneme id is outside the vocabulary)")
        ft = packed[:n_frames].astype(np.int32)
        spans = packed[n_frames:n_frames + 2 * n].astype(np.int64).reshape(n, 2)
        filled = hostlogic.fill_blank_frames(ft)
        return {'phn_seq_idx': idx, 'phn_seq_ipa': self._ipa(vocab, idx),
                'phn_start': [int(a) * frame_sec_ratio for a in spans[:, 0]],
                'phn_end': [int(b) * frame_sec_ratio for b in spans[:, 1]],
                'phn_score': packed[n_frames + 2 * n:n_frames + 3 * n].astype(np.float32).tolist(), 'score': score,
                'phn_frames': [int(idx[k]) if k >= 0 else self._blank() for k in filled]}

    def get_config(self):
        return {'huggingface_model_id': self.huggingface_model_id, 'cache_dir': self.cache_dir, 'pretrain_cfg': self.pretrain_cfg}

    def freeze_feature_encoder(self):
        self.wav2vec2.freeze_feature_encoder()
