"""``Force_APTAI`` — drop-in for models/force_aptai.py:19-323 on MI355X: frozen ``Wav2Vec2_PR`` encoder (inference
only, models/w2v2_pr.py:124-127) -> cross-attention forced aligner + BiLSTM regression.  Same constructor
``(pr_model_path, device, vocab)``, ``forward(epoch, **batch)`` dict keys, helpers and state-dict keys.  ``max_phn_seq_len``
(keyword, default 60 as in the reference, up to 255) is the number of phoneme slots per utterance.

Differences from the shipped reference, all forced by defects recorded in SURVEY.md §0:
 * batch > 1 works (the reference's ``RNN.forward`` raises NameError at models/modules.py:207; intent followed);
 * the CTC decode inside the step is the recogniser's: the best path by default, its `decoder = "flashlight"` / `"beam"` (the
   device beam search, aptai_ctc_beam_search) when set there; parity with torchaudio's decoder itself is unpinned, the package is
   not available.  It costs ONE device->host transfer per batch; the alignment read-out (:148-161, B*T host syncs in the reference) is one gather
   kernel + one transfer;
 * the encoder runs once per step (the reference ran the conv stack twice, models/w2v2_pr.py:129,132).
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops, task_heads
from .config import load_model_cfg
from .hostlogic import TV_NAMES
from .modules import CrossAttention, ForwardSumLoss, LowPassFilterLayer, PositionalEncoding, RNN, fwd_sum_targets
from .w2v2_pr import Wav2Vec2_PR
from .wav2vec2 import batch_invariant_scope

_NPHN = 60                              # the reference's max_phn_seq_len (models/force_aptai.py:36): the default slot count
MAX_PHN_SLOTS = ops.XATTN_MAX_SLOTS     # 255: what the wide softmax pair and the CTC kernels (256 classes, 511 states) hold


def labels_to_slots(labels, cap):
    """The phoneme slots of `Force_APTAI.transcript = "labels"`: `labels` int [B][L], padded with negative values (-100) ->
    (ids int32 [B][cap], zero where the label is padding, padded or cut to `cap` slots; lens int32 [B], the count of labels >= 0
    BEFORE the cut, so that a transcript that does not fit still shows).  Pure tensor arithmetic on the labels' device."""
    valid = labels >= 0
    ids = torch.where(valid, labels, torch.zeros_like(labels)).to(torch.int32)
    L = ids.shape[1]
    ids = torch.nn.functional.pad(ids, (0, cap - L)) if L < cap else ids[:, :cap]
    return ids.contiguous(), valid.sum(dim=1).to(torch.int32)


class EncoderAhead:
    """The frozen recogniser's pass (`Force_APTAI._encode`) one batch ahead on a side stream: the ONE owner of that stream, of the captured
    passes and of the hand-over, for the eager loop (`Force_APTAI.prefetch`) and for `GraphedForceStep`.  The recogniser is frozen and runs
    in eval mode, so WHEN it runs changes no result; beside the heads of batch n, the pass of batch n+1 fills the CUs the cooperating LSTM
    kernels (32 workgroups for 3.5 ms) leave idle.  Each step still does one encoder pass and one heads pass.  From the second launch of a
    batch shape on the pass is ONE hipGraph launch (no trainable state, no host-dependent control flow): the step was otherwise bound by the
    host's ~350 launches.  The hand-over rule: take() copies graph-owned outputs out on the CONSUMER stream, and every launch() begins with
    "the side stream waits for the current stream" - so a caller that takes and launches from one stream never has an output overwritten
    under a copy."""
    tensors = ("ac", "ids", "nlen", "frame_lens", "nlen_full")         # what `_encode` hands the heads, in the order of take(into=)

    def __init__(self, model):
        self.model = model
        self.stream = None             # the side stream, made at the first launch or capture
        self.entries = {}              # (shapes, dtypes, encoder precision) -> captured pass; None: its capture failed, stay eager
        self.captures = 0
        self._seen = set()             # keys that have run eagerly once: captured at the next sight
        self._launches = self._valid_from = 0

    def _key(self, audio, lengths):
        return (tuple(audio.shape), tuple(lengths.shape), audio.dtype, lengths.dtype, self.model.w2v2_pr.wav2vec2.encoder_precision)

    def capture(self, audio, lengths):
        """The captured pass for this batch shape, captured NOW if there is none (an eager pass with this shape has already run:
        weight copies and scratch buffers exist).  Raises if the capture fails."""
        key, w = self._key(audio, lengths), self.model.w2v2_pr.wav2vec2
        e = self.entries.get(key)
        if e is not None:
            return e
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=audio.device)
        e = SimpleNamespace(audio=audio.clone(), lengths=lengths.clone(), graph=torch.cuda.CUDAGraph(), out=None, last=0)
        step0 = w._step
        torch.cuda.synchronize(audio.device)
        # APTAI_FORCE_ENC_TILE forces one GEMM tile in the side-stream pass.  128-row tiles were the default while whole-CU workgroups kept the
        # heads' BiLSTM clusters waiting (12 % of the step).  Since the cluster kernels hold their compute units alone (csrc/lstm.hip, APTAI_LSTM_LDS_KB)
        # the dispatcher's own rule is the faster one again: 6.36 ms with 128, 6.09 ms with 0, 6.63 ms with 192 (interleaved, one box).
        with torch.cuda.graph(e.graph, stream=self.stream, capture_error_mode=ops.CAPTURE_MODE), \
                ops.auto_tile(int(os.environ.get("APTAI_FORCE_ENC_TILE", "0"))):
            e.out = self.model._encode(e.audio, e.lengths)
        w._step = step0                                                # capturing issued nothing
        self.entries[key] = e
        self.captures += 1
        return e

    def launch(self, audio, lengths):
        """Starts the pass for (audio, lengths) on the side stream; returns the handle take() turns into `_encode`'s result.  A
        replay of the shape's captured pass, or eager launches: at the first sight of a shape, with APTAI_FORCE_ENC_GRAPH=0, in
        batch-invariant evaluation (the captured pass is a training device) and after a capture that failed."""
        m, w, dev = self.model, self.model.w2v2_pr.wav2vec2, self.model.frame_lin.weight.device       # (a replay takes a host batch too)
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))        # the inputs, the previous step's frees, the copies of take()
        key = self._key(audio, lengths)
        graphs = os.environ.get("APTAI_FORCE_ENC_GRAPH", "1") != "0" and not (m.batch_invariant and not m.training)
        self._launches += 1
        with torch.cuda.stream(self.stream):
            e = self.entries.get(key) if graphs else None
            if e is None and graphs and key in self._seen and key not in self.entries:
                try:
                    e = self.capture(audio, lengths)
                except Exception as exc:                               # noqa: BLE001 - keep training, eagerly
                    import warnings
                    warnings.warn(f"Force_APTAI: encoder hipGraph capture failed ({exc!r}); the pass ahead stays eager")
                    torch.cuda.synchronize(dev)
                    self.entries[key] = None
            if e is not None:
                e.audio.copy_(audio, non_blocking=True)
                e.lengths.copy_(lengths, non_blocking=True)
                e.graph.replay()
                w._step += 1                                           # what the eager pass does on the host
                e.last, out = self._launches, e.out
            else:
                out = m._encode(audio, lengths)
                self._seen.add(key)
            event = self.stream.record_event()
        return SimpleNamespace(out=out, entry=e, n=self._launches, step=w._step, event=event)

    def take(self, handle, into=None):
        """`_encode`'s result for a launch, ready on the CURRENT stream: its tensors copied into `into` (static tensors in the order
        of `tensors`), into fresh tensors when a graph owns them, or handed over as they are.  None when the handle no longer
        holds its result: invalidated since, or its captured pass replayed again."""
        e, o = handle.entry, handle.out
        if handle.n <= self._valid_from or (e is not None and e.last != handle.n):
            return None
        cur = torch.cuda.current_stream(o.ac.device)
        cur.wait_event(handle.event)
        ts = [getattr(o, k) for k in self.tensors]
        if e is None:
            for t in ts:                                               # allocated on the side stream, consumed on this one
                t.record_stream(cur)
        if e is not None or into is not None:
            into = into if into is not None else [torch.empty_like(t) for t in ts]
            for d, t in zip(into, ts):
                d.copy_(t, non_blocking=True)
            ts = into
        return SimpleNamespace(g=o.g, step=handle.step, **dict(zip(self.tensors, ts)))

    def invalidate(self):
        """Drops every captured pass and every pending hand-over: the captured passes hold the addresses of the recogniser's
        compute copies (bf16 weights, layer copies, the eval head), which are rebuilt as new tensors when the parameters change."""
        self.entries, self._seen, self._valid_from = {}, set(), self._launches


class Force_APTAI(nn.Module):
    task_head = task_heads.ForceHead()      # everything after the frozen encoder, for this class and GraphedForceStep (task_heads.py)

    def __init__(self, pr_model_path, device, vocab, max_phn_seq_len=_NPHN):
        super().__init__()
        assert os.path.exists(pr_model_path)
        # phoneme slots per utterance; a transcript must stay BELOW it (models/force_aptai.py:111), so 255 slots take 254 phonemes
        if isinstance(max_phn_seq_len, bool) or not isinstance(max_phn_seq_len, (int, np.integer)) \
                or not 2 <= int(max_phn_seq_len) <= MAX_PHN_SLOTS:
            raise ValueError(f"Force_APTAI: max_phn_seq_len must be an integer in 2..{MAX_PHN_SLOTS}, not {max_phn_seq_len!r}")
        self.vocab = vocab
        self.device = device
        self.i = 0
        self.dp_loss_norm = None       # aptai_amd.dp.GlobalLossNorm under data parallelism
        self.hidden_drop = 0.2
        self.rnn_drop = 0.1
        self.max_phn_seq_len = int(max_phn_seq_len)
        self.frame_hidden_dim = 128
        self.phn_hidden_dim = 128
        self.att_hidden_dim = 128
        self.rnn_in_dim = 2 * self.att_hidden_dim
        self.xatt = CrossAttention(self.frame_hidden_dim, self.phn_hidden_dim, self.att_hidden_dim)
        self.align_loss = ForwardSumLoss()
        # wav2vec2 phoneme recognizer (models/force_aptai.py:60-78): config pickle + state dict written by the PR training script
        self.pr_model_path = pr_model_path
        pr_ckpt_path = os.path.join(pr_model_path, 'best-model-ckpt')
        # restricted unpickler: plain containers / values and configuration objects as attribute bags, nothing callable
        self.w2v2_pr_cfg = load_model_cfg(os.path.join(pr_ckpt_path, 'model_cfg.pkl'))
        self.w2v2_pr = Wav2Vec2_PR(self.w2v2_pr_cfg['pretrain_cfg'], self.w2v2_pr_cfg['cache_dir'],
                                   self.w2v2_pr_cfg['huggingface_model_id'], vocab).to(self.device)
        self.w2v2_pr.load_state_dict(torch.load(os.path.join(pr_ckpt_path, 'pytorch_model.bin'),
                                                map_location=torch.device(self.device), weights_only=True))
        H = self.w2v2_pr.wav2vec2.config.hidden_size          # reference hard-codes 1024 (:43)
        self.frame_lin = nn.Linear(H, self.frame_hidden_dim)
        self.frame_drop = nn.Dropout(self.hidden_drop)
        self.phn_emb_layer = nn.Embedding(len(self.vocab), self.phn_hidden_dim, padding_idx=0)
        self.pe_phn = PositionalEncoding(self.phn_hidden_dim, max_len=self.max_phn_seq_len, dropout=self.hidden_drop)
        self.rnn = RNN(self.rnn_in_dim, 9, self.rnn_drop)
        self.tv_lowpass = LowPassFilterLayer(self.device, 10, 49, 9)
        for param in self.w2v2_pr.parameters():
            param.requires_grad = False
        # the frozen recogniser only ever runs forward here: keep its residual stream in fp32 and hand the heads an fp32 last hidden
        # state (+1.6 % step time, smaller bf16 noise band on the alignment indices; "bf16" restores the plain bf16 stream)
        self.w2v2_pr.wav2vec2.set_encoder_precision("bf16_f32res")
        self.encoder_ahead = EncoderAhead(self)      # the recogniser's pass one batch ahead: prefetch() here, GraphedForceStep
        self._prefetched = None

    # how `pred_frame_phns` is read out of the attention: "argmax" (the reference, models/force_aptai.py:148: per-frame argmax, may
    # jump backwards and skip phonemes) or "monotonic" (opt-in: the best monotonic path through the same att_log rows, the Viterbi
    # read-out that belongs to the forward-sum loss; aptai_ctc_viterbi topology 1).  Losses, tvs_pred and gradients do not depend on it.
    alignment_readout = "argmax"

    # opt-in: in eval mode every row of a batch gets what the utterance gets at batch size 1 (the frozen recogniser runs with
    # Wav2Vec2_PR.batch_invariant, the low-pass filter pads at each row's own length).  Training steps - the recogniser's pass
    # inside them and the prefetch graph included - are what they were.
    batch_invariant = False

    # where the phoneme sequence comes from: "decoded" (the reference: the frozen recogniser's best path) or "labels" (opt-in: the
    # batch's `phoneme_labels`, the known transcript - labels_to_slots; no decode error can reach the aligner).  get_alignment and
    # get_faptai_output take a waveform alone and always decode.
    transcript = "decoded"

    def _transcript(self) -> str:
        if self.transcript not in ("decoded", "labels"):
            raise ValueError(f"Force_APTAI.transcript must be 'decoded' or 'labels', not {self.transcript!r}")
        return self.transcript

    def _too_long(self, n) -> str:
        return ('Need longer max phoneme sequence length.'
                f' ({n} phonemes do not fit max_phn_seq_len={self.max_phn_seq_len}: a transcript must be shorter than it;'
                f' Force_APTAI(..., max_phn_seq_len=) takes up to {MAX_PHN_SLOTS})')

    def _readout(self) -> str:
        if self.alignment_readout not in ("argmax", "monotonic"):
            raise ValueError(f"Force_APTAI.alignment_readout must be 'argmax' or 'monotonic', not {self.alignment_readout!r}")
        return self.alignment_readout

    # ------------------------------------------------------------------ shared body
    def _encode(self, audio_inputs, audio_lengths, phn_pred_list=None, labels=None):
        """Frozen recogniser (inference) + device best-path decode on the CURRENT stream: everything the heads read from it.
        `labels` (transcript = "labels"): the phoneme slots come from them and nothing is decoded."""
        pr = self.w2v2_pr
        pr.eval()                                                      # models/w2v2_pr.py:125: the recogniser always runs in eval mode
        # the recogniser is in eval mode while the heads train too: batch invariance reaches it only when this module evaluates
        with torch.no_grad(), batch_invariant_scope(pr, self.batch_invariant and not self.training):
            lens1d = audio_lengths.reshape(-1)
            out, _ = pr._logits_eval(audio_inputs, lens1d[:, None])
            dev = out._flat_last.device
            frame_lens = pr.wav2vec2._get_feat_extract_output_lengths(lens1d.to(dev)).to(torch.int32).contiguous()
            nlen_full = None
            if phn_pred_list is None and labels is not None:
                ids, nlen, nlen_full = self._label_slots(labels, dev)
            elif phn_pred_list is None:
                ids, nlen_full = pr._decode_device(out, self.max_phn_seq_len)  # int32 [B][slots] zero-padded, int32 [B] full length
                nlen = nlen_full.clamp(max=self.max_phn_seq_len - 1)           # as _label_slots: the kernels never leave a row
            else:
                padded = []
                for lst in phn_pred_list:
                    assert len(lst) < self.max_phn_seq_len, self._too_long(len(lst))
                    padded.append(np.pad(np.asarray(lst, dtype=np.int64), (0, self.max_phn_seq_len - len(lst)), mode='constant'))
                ids = torch.tensor(np.array(padded), dtype=torch.int32, device=dev)
                nlen = torch.tensor([len(l) for l in phn_pred_list], dtype=torch.int32, device=dev)
        # with the fp32 residual stream the heads read the UNROUNDED last hidden state (the fp32 GEMM takes either dtype)
        ac = out._flat_last_f32
        return SimpleNamespace(g=out._geom, ac=ac if ac is not None else out._flat_last, ids=ids, nlen=nlen, frame_lens=frame_lens,
                               step=pr.wav2vec2._step, nlen_full=nlen_full)

    def _label_slots(self, labels, dev):
        """(ids, lengths the kernels see, label counts the host checks) of transcript = "labels".  The kernels get the count cut to
        slots - 1, so a transcript that is too long cannot send them past a row; the uncut count is what trips the assertion."""
        ids, n = labels_to_slots(labels.to(dev), self.max_phn_seq_len)
        return ids, n.clamp(max=self.max_phn_seq_len - 1), n

    def prefetch(self, audio_inputs, audio_lengths):
        """Run the frozen recogniser for a batch on a side stream NOW (EncoderAhead.launch); the next forward / _run called with
        these same tensors picks the result up instead of encoding inline."""
        self._prefetched = (audio_inputs, audio_lengths, self.encoder_ahead.launch(audio_inputs, audio_lengths))

    def _take_prefetched(self, audio_inputs, audio_lengths):
        pf, self._prefetched = self._prefetched, None
        if pf is None or pf[0] is not audio_inputs or pf[1] is not audio_lengths:
            return None
        return self.encoder_ahead.take(pf[2])

    def _heads_state(self, g, ids, nlen, frame_lens, tv_targets, step):
        """(st, P) of the task head for one encoded batch: its state and the named parameters (task_heads.ForceParams)."""
        head = self.task_head
        st = head.state(self, g, (self.w2v2_pr.wav2vec2.base_seed, step), self.training, ids, nlen, frame_lens, tv_targets)
        if getattr(self, "dp_loss_norm", None) is not None and self.training:
            # the TV loss is a masked mean over the batch (models/force_aptai.py:137-141); the alignment and CTC terms are
            # means over utterances, which equal-sized shards already average exactly
            self.dp_loss_norm.begin(st.tv_tgt, None)
            st.norm_scalars = self.dp_loss_norm.scalars
        return st, head.params(self)

    def _run(self, audio_inputs, audio_lengths, tv_targets=None, phn_pred_list=None, _ac_override=None, _prefetch_next=None,
             labels=None):
        """Encoder (inference) -> decode -> heads.  Nothing in here synchronises host and device: the best-path decode, the
        phoneme slots, every length vector and the alignment read-out stay on the device; `_lists` makes the Python lists the
        reference returns with one round of transfers at the very end."""
        enc = self._take_prefetched(audio_inputs, audio_lengths) if phn_pred_list is None else None
        if enc is None:
            enc = self._encode(audio_inputs, audio_lengths, phn_pred_list, labels)
        elif labels is not None:                                       # a prefetched pass decoded: the known transcript replaces it
            enc.ids, enc.nlen, enc.nlen_full = self._label_slots(labels, enc.ids.device)
        if _prefetch_next is not None:                                 # the NEXT batch's encoder pass goes out before this batch's heads
            self.prefetch(*_prefetch_next)
        g, ids, nlen, frame_lens = enc.g, enc.ids, enc.nlen, enc.frame_lens
        ac = enc.ac if _ac_override is None else _ac_override          # test hook: heads on given embeddings
        st, P = self._heads_state(g, ids, nlen, frame_lens, tv_targets, enc.step)
        res = task_heads.HeadFn.apply(self.task_head, ac, st, *P)
        nlen_full = getattr(enc, "nlen_full", None)
        return res, g, (ids, nlen if nlen_full is None else nlen_full, frame_lens, phn_pred_list)

    def _consts(self, B, dev):
        """Batch-size dependent constants (forward-sum targets 1..slots, the all-frames length of the batch-1 branch)."""
        N = self.max_phn_seq_len
        key = (B, str(dev), N)
        c = getattr(self, "_const_cache", {}).get(key)
        if c is None:
            full = {}

            def full_T(T):
                if T not in full:
                    full[T] = torch.full((B,), T, dtype=torch.int32, device=dev)
                return full[T]
            c = {"fs_targets": fwd_sum_targets(B, N, dev),
                 "mono_targets": torch.arange(N, dtype=torch.int32, device=dev)[None, :].repeat(B, 1).contiguous(),
                 "full_T": full_T}
            self._const_cache = dict(getattr(self, "_const_cache", {}))
            self._const_cache[key] = c
        return c

    def _lists(self, dec):
        """Host views of the decode: (decoded id lists, frame lengths, decoded lengths, phoneme table) - the step's only
        device->host transfers.  The status words of the cooperative BiLSTM kernels (csrc/lstm.hip: every cross-workgroup wait
        is bounded and raises a status word on timeout) ride in the same transfer as the lengths: a timed-out wait means
        incomplete hidden states, so it raises here instead of returning a silently wrong `tvs_pred`."""
        ids, nlen, frame_lens, given = dec
        B = int(frame_lens.numel())
        status = ops.lstm_status_words(ids.device)
        parts = [frame_lens.reshape(-1).to(torch.int32), nlen.reshape(-1).to(torch.int32)] + ([status] if status is not None else [])
        host = torch.cat(parts).cpu().tolist()                        # ONE transfer: frame lengths | decoded lengths | LSTM status
        fl, n = [int(v) for v in host[:B]], [int(v) for v in host[B:2 * B]]
        ops.lstm_check(host[2 * B:], ids.device)
        table = ids.cpu().numpy()
        if given is None:
            # models/force_aptai.py:111 (checked once the lengths are on the host; the device decode filled the slots at most)
            assert all(v < self.max_phn_seq_len for v in n), self._too_long(max(n))
            given = [table[b, :n[b]].astype(np.int64) for b in range(len(n))]
        return given, fl, n, table

    def forward(self, epoch, audio_inputs, audio_lengths, phoneme_labels, phn_frames_49hz, LA, LP, JA, TTCL, TTCD, TMCL, TMCD,
                TBCL, TBCD, _phn_pred_list=None, _ac_override=None, _prefetch_next=None, _device_outputs=False):
        """`_prefetch_next = (audio_inputs, audio_lengths)` of the batch the NEXT call will receive (the same tensor objects)
        starts its frozen-encoder pass on a side stream beside this call's heads (see prefetch).  A row with fewer frames than
        phonemes (a speed-perturbed utterance: the audio shrinks, the transcript does not) has no alignment; the forward-sum loss
        runs with zero_infinity and counts it as zero."""
        tv_targets = torch.stack([LA, LP, JA, TTCL, TTCD, TMCL, TMCD, TBCL, TBCD], dim=-1).float()
        labels = phoneme_labels if (self._transcript() == "labels" and _phn_pred_list is None) else None
        res, g, dec = self._run(audio_inputs, audio_lengths, tv_targets, _phn_pred_list, _ac_override, _prefetch_next, labels)
        out = self.task_head.result(res, g, None)
        if _device_outputs:
            # private route of the device-resident evaluation (train_force_aptai._device_eval): the tensors `_run` already holds,
            # no lists and no transfer; the caller folds the checks of `_lists` into its own single read
            ids, nlen, frame_lens, _ = dec
            return dict(out, ctc_ids=ids, ctc_lens=nlen, frame_lens=frame_lens)
        phn_pred_list, frame_seq_lens, _, _ = self._lists(dec)
        fp = out.pop('frame_phns').cpu().numpy()                       # ONE transfer (reference: B*T .cpu() calls)
        return dict(out, pred_frame_phns=[fp[b, :frame_seq_lens[b]].tolist() for b in range(g.B)], pred_ctc_phn_seq=phn_pred_list)

    def load_state_dict(self, state_dict, *args, **kwargs):
        self.encoder_ahead.invalidate()
        # `pe_phn.pe` is a pure function of (max_phn_seq_len, width) whose rows do not depend on the row count: a checkpoint written
        # at another max_phn_seq_len loads, and this module keeps its own table
        pe, own = state_dict.get("pe_phn.pe"), self.pe_phn.pe
        if pe is not None and pe.shape != own.shape and pe.shape[1:] == own.shape[1:]:
            meta = getattr(state_dict, "_metadata", None)
            state_dict = state_dict.copy()
            state_dict["pe_phn.pe"] = own
            if meta is not None:
                state_dict._metadata = meta
        return super().load_state_dict(state_dict, *args, **kwargs)

    def set_encoder_precision(self, precision: str = "bf16"):
        """"bf16_f32res" (default here): bf16 GEMMs, fp32 residual stream; "bf16": all-bf16 stream; "mxfp8": the frozen recogniser's
        transformer Linear layers run with MX block-scaled FP8 operands (BASELINE configs[4]).  The heads stay fp32.  See
        Wav2Vec2Model.set_encoder_precision."""
        self.w2v2_pr.wav2vec2.set_encoder_precision(precision)
        return self

    def get_config(self):
        cfg = {'pr_model_path': self.pr_model_path, 'w2v2_pr_cfg': self.w2v2_pr_cfg, 'device': self.device, 'vocab': self.vocab}
        if self.max_phn_seq_len != _NPHN:                              # default-cap pickles stay what they were
            cfg['max_phn_seq_len'] = self.max_phn_seq_len
        return cfg

    def _wav(self, wav):
        device = next(self.parameters()).device
        if type(wav) is torch.Tensor:
            wav = wav[0]
        return (torch.unsqueeze(torch.Tensor(wav), dim=0).to(device),
                torch.unsqueeze(torch.LongTensor([len(wav)]), dim=0).to(device))

    def get_alignment(self, wav):
        """models/force_aptai.py:188-236: (N x T) log-attention of the decoded phonemes."""
        self.eval()
        with torch.no_grad():
            wav_input, wav_len = self._wav(wav)
            res, g, dec = self._run(wav_input, wav_len.reshape(-1))
            _, frame_seq_lens, phn_seq_lens, _ = self._lists(dec)
            att = res[5].view(g.B, g.Tp, self.max_phn_seq_len)[0]
            return {'alignment': att[0:frame_seq_lens[0], 0:phn_seq_lens[0]].permute(1, 0).cpu().numpy()}

    def get_faptai_output(self, wav):
        """models/force_aptai.py:238-322."""
        self.eval()
        with torch.no_grad():
            wav_input, wav_len = self._wav(wav)
            res, g, dec = self._run(wav_input, wav_len.reshape(-1))
            phn_pred_list, frame_seq_lens, _, table = self._lists(dec)
            tvs_out = res[3].squeeze(dim=0).cpu().numpy()
            tvs_pred_dict = {n: [row[i] for row in tvs_out] for i, n in enumerate(TV_NAMES)}
            align = res[8].view(g.B, g.Tp)[0, :g.T].cpu().numpy()
            return {'tvs_pred': tvs_pred_dict, 'pred_frame_phns': [int(table[0][a]) for a in align],
                    'pred_ctc_phn_seq': phn_pred_list, 'hidden_alignment': res[6].view(g.B, g.Tp, -1)[:, :g.T],
                    'hidden_tvs': res[7].view(g.B, g.Tp, -1)[:, :g.T]}
