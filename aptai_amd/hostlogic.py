"""Host-side (integer / control) logic of the hot path.  No device work happens here.

Every function cites the reference call site it mirrors.  "HF:" = the un-vendored
``transformers/models/wav2vec2/modeling_wav2vec2.py`` (5.15.0 in the survey container).
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

TV_NAMES = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")   # models/aptai.py:67-70


# ----------------------------------------------------------------------------- frame arithmetic
def conv_out_length(n, kernel: int, stride: int):
    """``floor((n - k) / s) + 1`` — HF:1004-1007 (torch.div(..., rounding_mode='floor') + 1)."""
    if isinstance(n, torch.Tensor):
        return torch.div(n - kernel, stride, rounding_mode="floor") + 1
    if isinstance(n, np.ndarray):
        return np.floor_divide(n - kernel, stride) + 1
    return (int(n) - kernel) // stride + 1


def feat_extract_output_lengths(n, conv_kernel: Sequence[int], conv_stride: Sequence[int]):
    """HF:997-1016 ``_get_feat_extract_output_lengths`` (no adapter). Exact integer arithmetic.

    Device tensors take the composed form: ``floor((floor(a / p) + q) / r) == floor((a + p q) / (p r))`` for integers with
    p, r > 0, so the seven ``floor((n - k) / s) + 1`` steps fold into ONE ``floor((n + c) / d)`` (c, d from the loop below:
    c = -80, d = 320 for wav2vec2) - two tiny launches instead of 21 on the step's dependency chain, bit-identical for every
    integer n (tests/test_cpu_host.py sweeps it against the step-by-step form)."""
    if isinstance(n, torch.Tensor) and n.is_cuda and not n.is_floating_point():
        c, d = 0, 1
        for k, s in zip(conv_kernel, conv_stride):
            c += d * (s - k)
            d *= s
        return torch.div(n + c, d, rounding_mode="floor")
    for k, s in zip(conv_kernel, conv_stride):
        n = conv_out_length(n, k, s)
    return n


def _composed_length_constants(conv_kernel: Sequence[int], conv_stride: Sequence[int]):
    c, d = 0, 1
    for k, s in zip(conv_kernel, conv_stride):
        c += d * (s - k)
        d *= s
    return c, d


def conv_layer_lengths(n_samples: int, conv_kernel: Sequence[int], conv_stride: Sequence[int]) -> List[int]:
    """Frame count after every conv layer (31999, 15999, ... 499 for 160000 samples)."""
    out = []
    n = int(n_samples)
    for k, s in zip(conv_kernel, conv_stride):
        n = (n - k) // s + 1
        out.append(n)
    return out


def conv0_frame_lengths(sample_lengths: torch.Tensor, kernel: int = 10, stride: int = 5) -> torch.Tensor:
    """First-layer frame count of every utterance, ``(len - kernel) // stride + 1`` as int32 (``conv_layer_lengths(len)[0]``),
    for the batch-invariant kernels (aptai_conv0_fwd_lens).  Pure tensor arithmetic on the lengths' device: no read-back.
    Utterances shorter than one window give values < 1; the model refuses those from the padded shape."""
    n = sample_lengths.reshape(-1).long()
    return (torch.div(n - kernel, stride, rounding_mode="floor") + 1).to(torch.int32).contiguous()


def frame_attention_mask(n_frames: int, frame_lengths: torch.Tensor) -> torch.Tensor:
    """(B, T) bool mask of valid frames — same result as HF:1018-1036's flip/cumsum construction."""
    ar = torch.arange(n_frames, device=frame_lengths.device)
    return ar[None, :] < frame_lengths[:, None]


# ----------------------------------------------------------------------------- long recordings: windows on the frame grid
def conv_stride_and_field(conv_kernel: Sequence[int], conv_stride: Sequence[int]):
    """(s, r) of the conv stack: frame j reads samples [s j, s j + r).  320 and 400 for wav2vec2's (10,3,3,3,3,2,2) / (5,2,2,2,2,2,2)."""
    s, r = 1, 1
    for k, st in zip(conv_kernel, conv_stride):
        r += (k - 1) * s
        s *= st
    return s, r


class LongFormPlan(NamedTuple):
    """Windows 0 .. K of one recording (long_form_plan).  Per window: first global frame, frame count, first sample, sample count."""
    n_samples: int
    frames: int                  # F
    K: int
    stride: int                  # s
    field: int                   # r
    window_frames: int
    hop_frames: int
    trim_frames: int
    overlap: int                 # window_frames - hop_frames
    frame_start: tuple           # f0_k = k hop_frames
    window_len: tuple            # frames_k = min(window_frames, F - f0_k)
    sample_start: tuple          # s f0_k
    sample_count: tuple          # s (window_frames - 1) + r, the last window: everything up to n_samples


def long_form_plan(n_samples: int, conv_kernel: Sequence[int], conv_stride: Sequence[int], window_frames: int = 499,
                   hop_frames: int = 399, trim_frames: int = 25) -> LongFormPlan:
    """Overlapped windows of a recording of `n_samples`, laid on the encoder's frame grid (HF pipelines: chunk_length_s /
    stride_length_s, there in samples).  F = conv_layer_lengths(n)[-1]; K = 0 if F <= window_frames else
    ceil((F - window_frames) / hop_frames); window k starts at global frame k hop_frames = sample s k hop_frames and, unless it is
    the last, carries exactly the s (window_frames - 1) + r samples of window_frames frames; the last carries the rest.  A valid
    convolution stack is shift-invariant in steps of s samples, so frame j of window k is global frame f0_k + j computed from the
    same samples; every frame lies in one or two windows and the last window owns more than `overlap` frames.  The defaults are a
    10 s window (the longest training clip), 2 s of overlap and the low-pass filter's half width as trim (long_form_ramp)."""
    W, hop, trim = int(window_frames), int(hop_frames), int(trim_frames)
    if W < 1 or hop < 1 or trim < 0:
        raise ValueError(f"long_form_plan: window_frames={W}, hop_frames={hop} must be positive and trim_frames={trim} not negative")
    if 2 * hop < W:
        raise ValueError(f"long_form_plan: hop_frames={hop} below half of window_frames={W}: a frame would lie in three windows")
    s, r = conv_stride_and_field(conv_kernel, conv_stride)
    n = int(n_samples)
    F = conv_layer_lengths(n, conv_kernel, conv_stride)[-1]
    if F < 1:
        raise ValueError(f"long_form_plan: a recording of {n} samples is shorter than the receptive field of the feature encoder ({r})")
    K = 0 if F <= W else -((W - F) // hop)
    overlap = W - hop
    if K > 0 and overlap <= 2 * trim:
        raise ValueError(f"long_form_plan: an overlap of {overlap} frames leaves nothing between two trims of {trim}")
    f0 = tuple(k * hop for k in range(K + 1))
    return LongFormPlan(n, F, K, s, r, W, hop, trim, overlap, f0, tuple(min(W, F - f) for f in f0), tuple(s * f for f in f0),
                        tuple(s * (W - 1) + r if k < K else n - s * f for k, f in enumerate(f0)))


def long_form_ramp(plan: LongFormPlan, kind: str = "linear") -> np.ndarray:
    """fp32 [overlap]: the weight of the LATER window at position j of an overlap, built in fp64 and rounded once.
    "linear": clip((j - trim + 0.5) / (overlap - 2 trim), 0, 1) - the `trim` frames next to either window's edge are never used
    at an interior seam (0 next to the later window's start, 1 next to the earlier window's end), a linear fade between them.
    "cut": 0 below the middle of the overlap, 1 from it on (no blending: what HF's pipeline does with its strides).
    A plan of one window has no seam: its table is all zeros and never read."""
    if kind not in ("linear", "cut"):
        raise ValueError(f"long_form_ramp: ramp must be 'linear' or 'cut', not {kind!r}")
    n = max(plan.overlap, 0)
    j = np.arange(n, dtype=np.float64)
    if plan.K == 0 and n <= 2 * plan.trim_frames:
        return np.zeros(n, dtype=np.float32)
    if kind == "cut":
        return (j + 0.5 >= n / 2).astype(np.float32)
    return np.clip((j - plan.trim_frames + 0.5) / (n - 2 * plan.trim_frames), 0.0, 1.0).astype(np.float32)


def long_form_stitch(windows, plan: LongFormPlan, ramp: np.ndarray):
    """numpy restatement of aptai_stitch_windows for one recording: `windows[k]` holds the fp32 rows of window k (at least
    window_len[k] of them, C channels).  Returns (stitched fp32 [F][C], frame argmax int64 [F], first maximum).  At position j of the
    overlap between windows k-1 and k: x0 where ramp[j] <= 0, x1 where ramp[j] >= 1, else x0 + ramp[j] (x1 - x0) in three rounded
    fp32 operations."""
    if len(windows) != plan.K + 1:
        raise ValueError(f"long_form_stitch: {len(windows)} windows for a plan of {plan.K + 1}")
    ramp = np.asarray(ramp, dtype=np.float32)
    wins = [np.asarray(w, dtype=np.float32)[:n] for w, n in zip(windows, plan.window_len)]
    if any(w.ndim != 2 or w.shape != (n, wins[0].shape[1]) for w, n in zip(wins, plan.window_len)):
        raise ValueError("long_form_stitch: every window needs its window_len rows of the same width")
    out = np.empty((plan.frames, wins[0].shape[1]), dtype=np.float32)
    for k, (f0, w) in enumerate(zip(plan.frame_start, wins)):
        out[f0:f0 + len(w)] = w                                        # the overlap with window k+1 is rewritten below
        if k > 0:
            m = min(plan.overlap, len(w))                              # == overlap: the last window owns more than that
            x0, x1, r = wins[k - 1][plan.hop_frames:plan.hop_frames + m], w[:m], ramp[:m, None]
            blend = x0 + r * (x1 - x0)                                 # float32 arrays: each operation rounds on its own
            out[f0:f0 + m] = np.where(r <= 0, x0, np.where(r >= 1, x1, blend))
    return out, out.argmax(axis=-1).astype(np.int64)


# ----------------------------------------------------------------------------- SpecAugment
def compute_mask_indices(shape, mask_prob: float, mask_length: int,
                         attention_mask: Optional[torch.Tensor] = None, min_masks: int = 0,
                         rng=np.random) -> np.ndarray:
    """SpecAugment span sampler, a restatement of HF:101-217 ``_compute_mask_indices``.

    Consumes the numpy RNG in the same order as the reference (one ``rand(1)`` for the
    probabilistic-rounding epsilon, then one ``choice`` per batch row) so that with the same
    ``np.random.seed`` both produce the same mask.  Returns a (B, L) bool array.
    """
    batch_size, sequence_length = shape
    if mask_length < 1:
        raise ValueError("`mask_length` has to be bigger than 0.")
    if mask_length > sequence_length:
        raise ValueError(
            f"`mask_length` has to be smaller than `sequence_length`, but got `mask_length`: {mask_length}"
            f" and `sequence_length`: {sequence_length}`")

    epsilon = rng.rand(1).item()

    def num_spans(input_length):
        n = int(mask_prob * input_length / mask_length + epsilon)
        n = max(n, min_masks)
        if n * mask_length > sequence_length:
            n = sequence_length // mask_length
        if input_length - (mask_length - 1) < n:
            n = max(input_length - (mask_length - 1), 0)
        return n

    if attention_mask is not None:
        input_lengths = [int(x) for x in attention_mask.detach().sum(-1).tolist()]
    else:
        input_lengths = [sequence_length] * batch_size

    mask = np.zeros((batch_size, sequence_length), dtype=bool)
    max_spans = num_spans(sequence_length)
    if max_spans == 0:
        return mask

    rows = []
    for input_length in input_lengths:
        n = num_spans(input_length)
        idx = rng.choice(np.arange(input_length - (mask_length - 1)), n, replace=False)
        dummy = sequence_length - 1 if len(idx) == 0 else idx[0]
        idx = np.concatenate([idx, np.ones(max_spans - n, dtype=np.int32) * dummy])
        rows.append(idx)
    starts = np.array(rows)
    starts = np.broadcast_to(starts[:, :, None], (batch_size, max_spans, mask_length))
    starts = starts.reshape(batch_size, max_spans * mask_length)
    offsets = np.arange(mask_length)[None, None, :]
    offsets = np.broadcast_to(offsets, (batch_size, max_spans, mask_length)).reshape(
        batch_size, max_spans * mask_length)
    idxs = starts + offsets
    if idxs.max() > sequence_length - 1:
        idxs[idxs > sequence_length - 1] = sequence_length - 1
    np.put_along_axis(mask, idxs, 1, -1)
    return mask


# ----------------------------------------------------------------------------- optimiser schedule
def get_lr_schedule(warmup_epochs: int, static_epochs: int, lr_decay: float) -> Callable[[int], float]:
    """LambdaLR factor of train/train_aptai.py:372-386 — note the 10x during warm-up/static phases."""
    plateau_end = warmup_epochs + static_epochs

    def lambda_lr(epoch):
        if epoch >= plateau_end:                       # exponential decay from the 10x plateau
            return 10.0 * lr_decay ** (epoch - plateau_end)
        if epoch >= warmup_epochs:                     # plateau
            return 10.0
        return 10.0 * (epoch + 1) / warmup_epochs      # linear warm-up to 10x
    return lambda_lr


# ----------------------------------------------------------------------------- collate (batch dict C0)
def _pad(seqs, value):
    return torch.nn.utils.rnn.pad_sequence(seqs, batch_first=True, padding_value=value)


def collate_aptai(batch: List[dict], with_phoneme_labels: bool = False) -> Dict[str, torch.Tensor]:
    """Batch dict of train/train_aptai.py:268-332 (+ ``phoneme_labels`` of train/train_force_aptai.py:271-275).

    ``audio_inputs`` zero-padded f32, ``audio_lengths`` i64, ``phn_frames_49hz`` i64 padded with 0,
    nine TV tracks f64 padded with -100.0.
    """
    out = {
        "audio_inputs": _pad([torch.as_tensor(x["audio"]) for x in batch], 0.0),
        "audio_lengths": torch.LongTensor([int(x["audio_len"]) for x in batch]),
    }
    if with_phoneme_labels:
        out["phoneme_labels"] = _pad([torch.IntTensor(x["phoneme_label"]) for x in batch], -100)
    out["phn_frames_49hz"] = _pad([torch.LongTensor(x["phn_frames_49hz"]) for x in batch], 0)
    for name in TV_NAMES:
        out[name] = _pad([torch.from_numpy(np.asarray(x["tvs_norm_49hz"][name])) for x in batch], -100.0)
    return out


def collate_pr(batch: List[dict]) -> Dict[str, torch.Tensor]:
    """Batch dict of train/train_phoneme_recognizer.py:224-239 (labels padded with -100)."""
    return {
        "input_values": _pad([torch.as_tensor(x["audio"]) for x in batch], 0.0),
        "input_lengths": torch.LongTensor([int(x["audio_len"]) for x in batch]),
        "phoneme_labels": _pad([torch.IntTensor(x["phoneme_label"]) for x in batch], -100),
    }


def ctc_target_lengths(phoneme_labels: torch.Tensor) -> torch.Tensor:
    """Count of labels >= 0 per row — the double Python loop of models/w2v2_pr.py:62-70, vectorised."""
    return (phoneme_labels >= 0).sum(dim=-1).to(torch.long).cpu()


# ----------------------------------------------------------------------------- low-pass taps (M1)
def lowpass_taps(cutoff: float, sampling_rate: float) -> np.ndarray:
    """51-tap Hann-windowed sinc of models/modules.py:27-44 (float64, unit DC gain)."""
    fc = cutoff / sampling_rate
    if fc > 0.5:
        raise Exception('Cutoff frequency must be at least twice the sampling rate.')
    b = 0.08
    N = int(np.ceil(4 / b))
    if not N % 2:
        N += 1
    n = np.arange(N)
    h = np.sinc(fc * 2 * (n - (N - 1) / 2))
    w = 0.5 * (1 - np.cos(n * 2 * np.pi / (N - 1)))
    h = h * w
    return h / np.sum(h)


# ----------------------------------------------------------------------------- greedy CTC read-out
def ctc_best_path(logits: np.ndarray, length: int, blank: int = 0) -> np.ndarray:
    """Best-path decode: frame argmax -> collapse repeats -> drop blank.

    Stands where the reference calls torchaudio's lexicon-free beam search
    (models/w2v2_pr.py:143-159).  That decoder is not in the container: *parity unpinned*
    (SURVEY.md §8c); with no LM the top beam is the best path up to beam pruning.
    """
    ids = np.asarray(logits)[:length].argmax(axis=-1)
    keep = np.ones(len(ids), dtype=bool)
    keep[1:] = ids[1:] != ids[:-1]
    ids = ids[keep]
    return ids[ids != blank].astype(np.int64)


# ----------------------------------------------------------------------------- the reference's beam decoder, restated
def ctc_bracketed_best_path(logits: np.ndarray, length: int, blank: int = 0, sil: int = None):
    """What the reference's decoder call returns for its settings, in closed form: (tokens int64, timesteps int32).

    models/w2v2_pr.py:144-159 / utility.py:448-471 call torchaudio.models.decoder.ctc_decoder(lexicon=None, lm=None, nbest=1,
    beam_size=10, beam_threshold=50, log_add=False (default), blank_token='(blank)', sil_token='(...)'): flashlight's
    lexicon-free decoder.  With no language model and max-merging of equal hypotheses a hypothesis' score is the sum of the emissions
    along its best alignment, so the prefix of the frame-wise argmax path is the top candidate of every frame, survives every pruning
    (beam_size >= 1, beam_threshold >= 0) and the first returned hypothesis IS the best path - `ctc_beam_search` below restates the
    published algorithm and tests/test_cpu_host.py checks the equality on random emissions.  What differs from a plain best-path read-out
    is the decoder's FRAMING: it starts every hypothesis with the silence token and closes it with another one (decodeBegin /
    decodeEnd), torchaudio then collapses repeats over that T + 2 long token row and drops blanks, and reports as `timesteps` the row
    positions where a token starts - so a frame t appears as t + 1, the first silence at 0, the closing one at T + 1, and a silence
    emitted at the very first / last frame merges with the framing one.  torchaudio is not in the image: *parity unpinned*
    (SURVEY.md section 8c); the sources restated are flashlight-text LexiconFreeDecoder.cpp and torchaudio/models/decoder/_ctc_decoder.py
    as published."""
    ids = np.asarray(logits)[:length].argmax(axis=-1).astype(np.int64)
    row = ids if sil is None else np.concatenate([[sil], ids, [sil]])
    keep = np.ones(len(row), dtype=bool)
    keep[1:] = row[1:] != row[:-1]
    keep &= row != blank
    pos = np.nonzero(keep)[0]
    return row[pos].astype(np.int64), pos.astype(np.int32)


def ctc_beam_search(emissions: np.ndarray, blank: int, sil: int, beam_size: int = 10, beam_size_token: int = None,
                    beam_threshold: float = 50.0, log_add: bool = False, nbest: int = 1, sil_score: float = 0.0, stats: dict = None,
                    lm=None, lm_weight: float = 1.0):
    """flashlight's lexicon-free CTC beam search, without a language model or with a token n-gram (`lm`), restated from the
    published sources (see ctc_bracketed_best_path), plus torchaudio's read-out of each hypothesis.  emissions [T][N] (any scores:
    the reference feeds raw logits).  Returns the `nbest` best hypotheses, best first, as (tokens int64, timesteps int32, score float).

    State of a hypothesis = (token history, last token, last-was-blank); per frame every hypothesis is extended by every token (the
    `beam_size_token` best of the frame when given): a non-blank token that differs from the last one, or follows a blank, EXTENDS
    the history; a blank keeps it and sets the flag; a repeat keeps it.  Candidates below best - beam_threshold are dropped,
    candidates of equal state are merged (max, or log-add with `log_add`), the `beam_size` best survive.  The oracle of the device
    search (aptai_ctc_beam_search, `Wav2Vec2_PR.decoder = "beam"`) and of the closed form above: O(T beam N) Python, not a product
    hot path.

    `stats` (optional dict; the result does not depend on it) receives what a test needs to know about its INPUT before it compares
    another implementation with this one:
      min_decision_gap   the smallest score difference any decision of the search rests on: last kept vs first dropped merged
                         candidate, any candidate vs the floor, adjacent n-best scores (the first one not returned included), the
                         k-th vs (k+1)-th token score where `beam_size_token` cuts, and the best vs second candidate of a merged
                         state (whose back-pointer survives).  inf when no such pair exists.
      revived_histories  survivors that extend into a history which existed before the frame, is held by no hypothesis of the beam
                         it is extended from, and has a descendant in that beam
      max_merge          the largest number of candidates merged into one state

    `lm` (an ngram.NGramLM; only its tables W = lm_weight * score, next, Wf = lm_weight * final and start are used) adds
    W[state(history)][n] to every candidate that EXTENDS its history: sc = ((score + em) + sil bonus) + W, in that order; blanks
    and repeats take no term.  The state of a new history is next[state(parent)][n], the empty history holds `start`; the closing
    silence adds Wf[state(history)].  The frame floor is the maximum over all candidates, LM term included, - beam_threshold; merge
    rule, tie rule and read-out are unchanged (flashlight keeps its LM states in a trie over the whole history: equal token
    sequences still merge).  With an LM `stats` also receives
      best_not_from_slot0  the number of frames whose best candidate does not descend from the first hypothesis of the beam"""
    em = np.asarray(emissions, dtype=np.float64)
    T, N = em.shape
    if lm is not None:
        if lm.n_tokens != N:
            raise ValueError(f"ctc_beam_search: the language model has {lm.n_tokens} tokens, the emissions {N}")
        lm_w, lm_next, lm_wf, lm_start = lm.host_tables(lm_weight)
        state_of = {0: lm_start}                   # history id -> LM state
    k_tok = N if beam_size_token is None else min(int(beam_size_token), N)
    trie = {}                                      # (history id, token) -> history id (the ZeroLM state tree)
    parent_of = {0: None}                          # history id -> parent history id
    if stats is not None:
        stats.update(min_decision_gap=float("inf"), revived_histories=0, max_merge=0)
        if lm is not None:
            stats["best_not_from_slot0"] = 0

    def gap(d):
        if stats is not None and d == d:
            stats["min_decision_gap"] = min(stats["min_decision_gap"], abs(float(d)))

    def child(hist, tok):
        key = (hist, tok)
        if key not in trie:
            trie[key] = len(trie) + 1
            parent_of[trie[key]] = hist
            if lm is not None:
                state_of[trie[key]] = int(lm_next[state_of[hist], tok])
        return trie[key]

    def score_of(h, n):
        sc = h[0] + em[t, n] + (sil_score if n == sil else 0.0)
        if lm is not None and n != blank and (n != h[3] or h[4]):
            sc = sc + lm_w[state_of[h[1]], n]
        return sc

    # a hypothesis: (score, history id, parent hypothesis or None, token, last-was-blank)
    hyps = [(0.0, 0, None, sil, False)]
    for t in range(T):
        order = np.argsort(-em[t], kind="stable")[:k_tok] if k_tok < N else np.arange(N)
        if stats is not None:
            if 0 < k_tok < N:
                by_score = np.sort(em[t])[::-1]
                gap(by_score[k_tok - 1] - by_score[k_tok])
            known = len(trie)                      # history ids up to here existed before the frame
            held = {h[1] for h in hyps}
            ancestors = set()
            for hist in held:
                hist = parent_of[hist]
                while hist is not None and hist not in ancestors:
                    ancestors.add(hist)
                    hist = parent_of[hist]
        cands, best = [], -np.inf
        for h in hyps:
            hs, hist, _, prev, prev_blank = h
            for n in order:
                n = int(n)
                sc = score_of(h, n)
                if n != blank and (n != prev or prev_blank):
                    c = (sc, child(hist, n), h, n, False)
                elif n == blank:
                    c = (sc, hist, h, n, True)
                else:
                    c = (sc, hist, h, n, False)
                best = max(best, sc)
                if sc >= best - beam_threshold:
                    cands.append(c)
        if stats is not None:                  # every candidate against the floor, those the running maximum dropped included;
            for h in hyps:                     # the maximum itself passes by construction (threshold >= 0): not a decision
                for n in order:
                    sc = score_of(h, int(n))
                    if sc != best:
                        gap(sc - (best - beam_threshold))
            if lm is not None and max(score_of(hyps[0], int(n)) for n in order) < best:
                stats["best_not_from_slot0"] += 1
        hyps = _merge_and_prune(cands, best - beam_threshold, beam_size, log_add, stats)
        if stats is not None:
            stats["revived_histories"] += sum(1 for h in hyps if h[1] != h[2][1] and h[1] <= known and h[1] not in held
                                              and h[1] in ancestors)
    cands = [(h[0] if lm is None else h[0] + lm_wf[state_of[h[1]]], h[1], h, sil, False) for h in hyps]
    best = max(c[0] for c in cands)
    floor = best - beam_threshold
    if stats is not None:
        for c in cands:
            if c[0] != best:
                gap(c[0] - floor)
    final = _merge_and_prune(cands, floor, beam_size, log_add, stats)
    if stats is not None:
        for a, b in zip(final[:nbest], final[1:nbest + 1]):
            gap(a[0] - b[0])
    out = []
    for h in final[:nbest]:
        row, node = [], h
        while node is not None:
            row.append(node[3])
            node = node[2]
        row = np.asarray(row[::-1], dtype=np.int64)          # T + 2 tokens: opening silence, one per frame, closing silence
        keep = np.ones(len(row), dtype=bool)
        keep[1:] = row[1:] != row[:-1]
        keep &= row != blank
        pos = np.nonzero(keep)[0]
        out.append((row[pos], pos.astype(np.int32), float(h[0])))
    return out


def _merge_and_prune(cands, floor, beam_size, log_add, stats=None):
    cands = [c for c in cands if c[0] >= floor]
    cands.sort(key=lambda c: (c[1], c[3], c[4], -c[0]))          # equal states adjacent, the best of each first
    merged, size = [], 0
    for c in cands:
        if merged and merged[-1][1] == c[1] and merged[-1][3] == c[3] and merged[-1][4] == c[4]:
            size += 1
            if stats is not None:
                stats["max_merge"] = max(stats["max_merge"], size)
                if size == 2:                                    # best vs second of the state: which back-pointer survives
                    stats["min_decision_gap"] = min(stats["min_decision_gap"], abs(best_of_state - c[0]))
            if log_add:
                m = merged[-1]
                merged[-1] = (float(np.logaddexp(m[0], c[0])),) + m[1:]
            continue
        merged.append(c)
        size, best_of_state = 1, c[0]
        if stats is not None:
            stats["max_merge"] = max(stats["max_merge"], 1)
    merged.sort(key=lambda c: -c[0])
    if stats is not None and len(merged) > beam_size:
        stats["min_decision_gap"] = min(stats["min_decision_gap"], abs(merged[beam_size - 1][0] - merged[beam_size][0]))
    return merged[:beam_size]


# ----------------------------------------------------------------------------- forced alignment of a known transcript
def ctc_forced_align(logits: np.ndarray, length: int, targets, blank: int = 0, topology: str = "ctc"):
    """Best (Viterbi) path of the label sequence `targets` through the first `length` frames of `logits` [T][V]:
    (frame_token int32 [T], score).  The contract of aptai_ctc_viterbi (include/aptai_hip.h), restated with the same order of
    operations so that the device kernel can be checked against it bit for bit; also the CPU route for host-side tools.

    topology "ctc": states blank, l1, blank, ..., lL, blank; transitions stay, +1, and +2 where the two labels differ.
    topology "monotonic": states l1 .. lL, transitions stay and +1, start in l1, end in lL (`blank` is ignored).
    frame_token[t] = transcript position 0..L-1, -1 on a blank frame, -2 at t >= length and everywhere when no path exists.

    The path does not depend on the per-frame normaliser (one constant for every state of a frame), so the recursion runs on
    the RAW logits in their own dtype: new[s] = best + x_t[ext_s], one addition per state and frame; max is exact.
    Tie rule: stay is the incumbent; the s-1 predecessor replaces it only if strictly greater; then the s-2 predecessor
    replaces that only if strictly greater; the path ends in the last state unless the one before it is strictly greater.
    score = log-probability of the path under the per-frame log-softmax (float64 sum; -inf when no path exists, 0.0 for
    length == 0 and no labels).  A label outside [0, V) has no path."""
    if topology not in ("ctc", "monotonic"):
        raise ValueError(f"topology must be 'ctc' or 'monotonic', not {topology!r}")
    x = np.asarray(logits)
    if not np.issubdtype(x.dtype, np.floating):
        x = x.astype(np.float32)
    T, V = x.shape
    Tb = max(0, min(int(length), T))
    tg = np.asarray(targets, dtype=np.int64).reshape(-1)
    L = len(tg)
    ctc = topology == "ctc"
    ext = np.full(2 * L + 1, blank, dtype=np.int64) if ctc else tg.copy()
    if ctc:
        ext[1::2] = tg
    S = len(ext)
    frame_token = np.full(T, -2, dtype=np.int32)
    if Tb == 0 or S == 0:
        return frame_token, (0.0 if (Tb == 0 and L == 0) else -np.inf)
    ninf = x.dtype.type(-np.inf)
    ok = (ext >= 0) & (ext < V)
    xe = np.where(ok[None, :], x[:Tb][:, np.where(ok, ext, 0)], ninf)             # [Tb][S] raw logit per extended state
    skip = np.zeros(S, dtype=bool)                                                # s-2 -> s allowed
    if ctc and S >= 4:
        skip[3::2] = tg[1:] != tg[:-1]
    bp = np.zeros((Tb, S), dtype=np.int8)
    cur = np.full(S, ninf)
    n_init = min(2, S) if ctc else 1
    cur[:n_init] = xe[0, :n_init]
    for t in range(1, Tb):
        best, c = cur.copy(), bp[t]
        a1 = np.concatenate([[ninf], cur[:-1]])
        m = a1 > best
        best[m], c[m] = a1[m], 1
        if ctc:
            a2 = np.concatenate([[ninf, ninf], cur[:-2]])[:S]
            m = skip & (a2 > best)
            best[m], c[m] = a2[m], 2
        with np.errstate(invalid="ignore"):
            cur = best + xe[t]
    s = S - 1
    if ctc and S >= 2 and cur[S - 2] > cur[S - 1]:
        s = S - 2
    if not cur[s] > ninf:
        return frame_token, -np.inf
    states = np.empty(Tb, dtype=np.int64)
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    frame_token[:Tb] = (np.where(states & 1, states >> 1, -1) if ctc else states).astype(np.int32)
    x64 = x[:Tb].astype(np.float64)
    mx = x64.max(axis=1)
    lz = mx + np.log(np.exp(x64 - mx[:, None]).sum(axis=1))
    score = float((x64[np.arange(Tb), ext[states]] - lz).sum())
    return frame_token, score


def alignment_spans(frame_token, n_tokens: int) -> np.ndarray:
    """int32 [n_tokens][2]: first and one-past-last frame of every transcript position of a `frame_token` row (-1, -1 = the
    position owns no frame) - the `spans` output of aptai_ctc_viterbi."""
    ft = np.asarray(frame_token).reshape(-1)
    spans = np.full((int(n_tokens), 2), -1, dtype=np.int32)
    for k in range(int(n_tokens)):
        hit = np.nonzero(ft == k)[0]
        if hit.size:
            spans[k] = (hit[0], hit[-1] + 1)
    return spans


def long_form_force_align(window_logits, plan: LongFormPlan, ramp, targets, blank: int = 0):
    """Forced alignment of a long recording in numpy: the per-window logits stitched (long_form_stitch; `ramp` is the table of
    long_form_ramp or its kind, "linear" / "cut"), then ctc_forced_align of the whole transcript over the `plan.frames` stitched
    frames, then alignment_spans.  Returns (frame_token int32 [F], spans int32 [len(targets)][2], score, stitched fp32 [F][V]):
    what Wav2Vec2_PR.force_align_long computes on the device, for host-side tools and as its oracle."""
    table = long_form_ramp(plan, ramp) if isinstance(ramp, str) else ramp
    stitched, _ = long_form_stitch(window_logits, plan, table)
    tg = np.asarray(targets, dtype=np.int64).reshape(-1)
    frame_token, score = ctc_forced_align(stitched, plan.frames, tg, blank=blank)
    return frame_token, alignment_spans(frame_token, len(tg)), score, stitched


def fill_blank_frames(frame_token) -> np.ndarray:
    """A transcript position for EVERY valid frame of a CTC alignment (what per-frame labels such as `phn_frames_49hz` need).
    This is OUR rule - the reference takes its frame labels from MAUS boundaries, which are not reproducible here: a run of
    blank frames between two tokens is split at its midpoint, the earlier token taking the extra frame of an odd run; leading
    blanks go to the first token and trailing blanks to the last.  Frames marked -2 (padding / no path) stay -2; a row without
    any token is returned unchanged."""
    out = np.array(frame_token, dtype=np.int32).reshape(-1).copy()
    tok = np.nonzero(out >= 0)[0]
    if tok.size == 0:
        return out
    valid = np.nonzero(out != -2)[0]
    out[valid[valid < tok[0]]] = out[tok[0]]
    out[valid[valid > tok[-1]]] = out[tok[-1]]
    for a, b in zip(tok[:-1], tok[1:]):
        n = b - a - 1                                  # blank run a+1 .. b-1
        if n > 0:
            h = (n + 1) // 2
            out[a + 1:a + 1 + h] = out[a]
            out[a + 1 + h:b] = out[b]
    return out


# ----------------------------------------------------------------------------- target preparation
def interpolate_signal(org_sig, tar_len: int) -> np.ndarray:
    """Linear resampling of a [frames] or [frames][channels] track to ``tar_len`` points that span the same time range
    (data/dataset_hprc.py:2307-2313: 100 Hz trajectories -> the encoder's 49 Hz frames).  scipy's interp1d(kind='linear') on the
    integer grid, written out: out[i] = (1-w) x[floor(p)] + w x[floor(p)+1] at p = i (n-1)/(tar_len-1)."""
    x = np.asarray(org_sig, dtype=np.float64)
    n = x.shape[0]
    pos = np.linspace(0, n - 1, tar_len)
    lo = np.clip(np.floor(pos).astype(np.int64), 0, max(n - 2, 0))
    w = pos - lo
    hi = np.minimum(lo + 1, n - 1)
    if x.ndim > 1:
        w = w.reshape((-1,) + (1,) * (x.ndim - 1))
    return x[lo] + (x[hi] - x[lo]) * w


def speed_rate(rate: int, factor: float) -> int:
    """The rate a source sampled at `rate` counts as when it is played `factor` times as fast: int(round(rate * factor)), the rule
    of torchaudio.transforms.Speed (and sox `speed`).  Resampling from it back to the target rate is the speed perturbation of
    Ko et al. 2015: 16 kHz at 0.9 is 14400 -> 16000 = 9:10, ten samples out for nine in."""
    return int(round(rate * factor))


def _warp_positions(n_in: int, n_out: int) -> np.ndarray:
    return np.linspace(0, n_in - 1, n_out)


def warp_track(x, n_in: int, n_out: int, ignore: float = -100.0) -> np.ndarray:
    """The first `n_in` frames of a fp64 track stretched to `n_out` frames over the same time range, as `interpolate_signal` does
    it (the oracle of aptai_warp_targets, bit for bit).  A frame whose left neighbour is `ignore`, or whose right neighbour is and
    has a weight above 0, is `ignore`.  n_in == n_out returns the frames as they are; n_in == 0 returns n_out frames of `ignore`."""
    x = np.asarray(x, dtype=np.float64)[:n_in]
    n_in, n_out = int(n_in), int(n_out)
    if n_in == 0:
        return np.full(n_out, ignore, dtype=np.float64)
    if n_in == n_out:
        return x.copy()
    out = interpolate_signal(x, n_out)
    pos = _warp_positions(n_in, n_out)
    lo = np.clip(np.floor(pos).astype(np.int64), 0, max(n_in - 2, 0))
    hi = np.minimum(lo + 1, n_in - 1)
    out[(x[lo] == ignore) | ((pos - lo > 0) & (x[hi] == ignore))] = ignore
    return out


def warp_frame_labels(lab, n_in: int, n_out: int) -> np.ndarray:
    """The first `n_in` frame labels stretched to `n_out` frames: frame i takes the label nearest to its position on the old grid,
    lab[min(floor(p_i + 0.5), n_in - 1)] with warp_track's positions.  n_in == 0 returns n_out zeros (the collate's padding)."""
    lab = np.asarray(lab)[:n_in]
    n_in, n_out = int(n_in), int(n_out)
    if n_in == 0:
        return np.zeros(n_out, dtype=lab.dtype)
    k = np.minimum(np.floor(_warp_positions(n_in, n_out) + 0.5).astype(np.int64), n_in - 1)
    return lab[k]


def match_phonemes_to_frames(phoneme_boundaries, phoneme_list, frame_duration: float = 0.02) -> list:
    """Frame labels from phoneme END boundaries (utility.py:317-342): frame k covers [k*step, (k+1)*step) centiseconds with
    step = int(frame_duration*100); it takes the first phoneme whose boundary falls inside, otherwise keeps the previous frame's
    label (None before the first hit).  The reference's O(frames x phonemes) scan as one searchsorted."""
    b = np.asarray(phoneme_boundaries, dtype=np.float64)
    step = int(frame_duration * 100)
    stop = int(b[-1] * 100) + 1
    out, current = [], None
    starts = np.arange(0, stop, step)
    for fs in starts:
        lo, hi = fs / 100.0, (fs + int(frame_duration * 100)) / 100.0
        hit = np.nonzero((b >= lo) & (b < hi))[0]
        if hit.size:
            current = phoneme_list[int(hit[0])]
        out.append(current)
    return out



# ----------------------------------------------------------------------------- input pipeline: 16 kHz resample + crop (f-4)
def resample(waveform, orig_freq: int, new_freq: int = 16000, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """`torchaudio.functional.resample(waveform, orig_freq, new_freq)` as data/dataset_commonphone.py:31-33 calls it (wav2vec2
    was pre-trained on 16 kHz audio): band-limited sinc interpolation with a Hann window (torchaudio's default
    `sinc_interp_hann`, lowpass_filter_width 6, rolloff 0.99), restated from the published algorithm - torchaudio is not in this
    image, so parity with it is unpinned; the test pins the properties (length, DC gain, a tone keeps its frequency, identity).
    waveform: 1-D or (channels, time) array / tensor; returns a float32 tensor of the same rank."""
    import math
    w = torch.as_tensor(np.asarray(waveform), dtype=torch.float32) if not torch.is_tensor(waveform) else waveform.float()
    squeeze = w.dim() == 1
    w = w.reshape(1, -1) if squeeze else w.reshape(-1, w.shape[-1])
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq == new_freq:
        return w[0] if squeeze else w
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    length = w.shape[-1]
    x = torch.nn.functional.pad(w, (width, width + orig))
    y = torch.nn.functional.conv1d(x[:, None], kernels.float(), stride=orig)          # (channels, new, frames)
    y = y.transpose(1, 2).reshape(w.shape[0], -1)
    y = y[..., :math.ceil(new * length / orig)]
    return y[0] if squeeze else y


def resample_out_length(n: int, orig: int, new: int) -> int:
    """``ceil(new * n / orig)`` in integer arithmetic: the number of samples `resample` returns for `n` input samples."""
    return (int(new) * int(n) + int(orig) - 1) // int(orig)


def resample_taps(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> dict:
    """The windowed-sinc filter bank `resample` builds, in fp64, without its clamped entries: what aptai_resample_batch reads.

    The full bank is [new][2 width + orig] (orig, new = the rates over their gcd); row p is the filter of the output samples
    n = q new + p.  Wherever |t base| >= lowpass_filter_width the clamp puts the Hann window at cos^2(pi/2): such an entry is below
    2e-49 and at most 2 width + 1 entries per row are not of that kind.  Returns dict(taps fp64 [new][Kc], first int64 [new],
    orig, new, width) with full[p][first[p] + j] == taps[p][j] and only clamped entries outside, so that

        y[q new + p] = sum_j taps[p][j] x[q orig + first[p] + j - width],   x = 0 outside [0, len).

    Kc is the largest unclamped count made odd (rows of an odd pitch start on different LDS banks); a row is shifted left where
    it would otherwise run past the bank's end.  Equal rates give the identity table (one tap of 1.0, width 0)."""
    import math
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"sampling rates must be positive, got {orig_freq} -> {new_freq}")
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    if orig == new:
        return {"taps": np.ones((1, 1)), "first": np.zeros(1, dtype=np.int64), "orig": 1, "new": 1, "width": 0}
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    full_w = 2 * width + orig
    # per row the unclamped entries form one run around k = width + p orig / new; rows are built one at a time so that a ratio
    # such as 16001 -> 16000 (a full bank of 16000 x 16015 entries) never exists in memory
    half = lowpass_filter_width * orig / base                      # |k - centre| < half  <=>  unclamped (up to rounding: checked below)
    span = 2 * int(math.ceil(half)) + 3
    p = np.arange(new, dtype=np.int64)
    k0 = np.clip(np.floor(width + p * orig / new - half).astype(np.int64) - 1, 0, max(full_w - span, 0))
    k = k0[:, None] + np.arange(min(span, full_w), dtype=np.int64)[None, :]          # candidate columns, [new][span]

    def t_of(cols):                                                # `resample`'s own expression, operation for operation
        return (-(p.reshape((-1,) + (1,) * (cols.ndim - 1)).astype(np.float64)) / new + (cols - width).astype(np.float64) / orig) * base

    t_raw = t_of(k)
    t = np.clip(t_raw, -lowpass_filter_width, lowpass_filter_width)
    live = np.abs(t_raw) < lowpass_filter_width
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    tp = t * math.pi
    vals = np.where(tp == 0, 1.0, np.sin(tp) / np.where(tp == 0, 1.0, tp)) * window * (base / orig)
    # t grows with k, so the unclamped entries of a row are one run: the window holds all of them if its two neighbours are clamped
    left, right = k[:, 0] - 1, k[:, -1] + 1
    assert (((left < 0) | (np.abs(t_of(left)) >= lowpass_filter_width))
            & ((right >= full_w) | (np.abs(t_of(right)) >= lowpass_filter_width))).all(), "unclamped entry outside the candidate window"
    count = live.sum(axis=1)
    Kc = int(count.max())
    Kc += 1 - Kc % 2
    assert Kc <= 2 * width + 1 <= full_w
    first_live = np.argmax(live, axis=1)
    j0 = np.minimum(first_live, k.shape[1] - Kc)                   # row start inside the candidate window
    j0 = np.minimum(j0, (full_w - Kc) - k0)                        # ... and inside the bank
    assert (j0 >= 0).all() and (j0 <= first_live).all()
    cols = j0[:, None] + np.arange(Kc)[None, :]
    taps = np.take_along_axis(vals, cols, axis=1)
    assert (np.take_along_axis(live, cols, axis=1).sum(axis=1) == count).all()
    return {"taps": np.ascontiguousarray(taps), "first": (k0 + j0).astype(np.int64), "orig": orig, "new": new, "width": int(width)}


def _pack_audio(batch: List[dict]):
    """The items' audio back to back in one 1-D tensor (their own dtype: float32, or int16 PCM) and int64 offsets [B + 1]."""
    waves = [torch.as_tensor(x["audio"]).reshape(-1) for x in batch]
    lens = [int(x["audio_len"]) for x in batch]
    offsets = torch.zeros(len(batch) + 1, dtype=torch.long)
    offsets[1:] = torch.cumsum(torch.LongTensor(lens), 0)
    return (torch.cat(waves) if waves else torch.zeros(0)), offsets


def collate_pr_raw(batch: List[dict]) -> Dict[str, torch.Tensor]:
    """`collate_pr` for audio at its native rate: no padding on the host - `audio_packed` holds the utterances back to back,
    `audio_offsets` int64 [B + 1] their running lengths; aptai_amd.frontend turns the pair into `input_values` / `input_lengths`
    on the device.  The labels are `collate_pr`'s."""
    packed, offsets = _pack_audio(batch)
    return {"audio_packed": packed, "audio_offsets": offsets,
            "phoneme_labels": _pad([torch.IntTensor(x["phoneme_label"]) for x in batch], -100)}


def collate_aptai_raw(batch: List[dict], with_phoneme_labels: bool = False) -> Dict[str, torch.Tensor]:
    """`collate_aptai` for audio at its native rate (see collate_pr_raw): `audio_packed` + `audio_offsets` instead of
    `audio_inputs` + `audio_lengths`; frame labels, phoneme labels and TV targets exactly as `collate_aptai` pads them."""
    packed, offsets = _pack_audio(batch)
    out = {"audio_packed": packed, "audio_offsets": offsets}
    if with_phoneme_labels:
        out["phoneme_labels"] = _pad([torch.IntTensor(x["phoneme_label"]) for x in batch], -100)
    out["phn_frames_49hz"] = _pad([torch.LongTensor(x["phn_frames_49hz"]) for x in batch], 0)
    for name in TV_NAMES:
        out[name] = _pad([torch.from_numpy(np.asarray(x["tvs_norm_49hz"][name])) for x in batch], -100.0)
    return out


def convert_ts_float(input_string: str):
    """'[(0.0, 0.1), (0.1, 0.25)]' -> [(0.0, 0.1), (0.1, 0.25)] (utility.py:298-309)."""
    s = input_string.replace('[', '').replace(']', '').replace(' ', '')
    out = []
    for piece in s.split('),('):
        a, b = map(float, piece.strip('()').split(','))
        out.append((a, b))
    return out


def phonemes_idx(vocab: dict, phonemes: str) -> List[int]:
    """Space-separated phoneme string -> vocabulary ids (utility.py:236-244)."""
    return [vocab[p] for p in phonemes.split(' ')]


def crop_one_second(audio, phoneme_timestamps: str, phonemes: str, vocab: dict, rng=None, duration_samples: int = 16000):
    """The optional 1-second training crop of data/dataset_commonphone.py:35-70: a random window of `duration_samples` and the
    ids of the phonemes that overlap it (first = the phoneme that contains the window start, last = the one that contains its
    end).  `rng` needs `randint(a, b)` with both ends included (default: the `random` module, as the reference)."""
    import random as _random
    rng = rng or _random
    audio = torch.as_tensor(audio)
    start = rng.randint(0, len(audio) - duration_samples)
    end = start + duration_samples
    crop = audio[start:end]
    t0, t1 = start / 16000, end / 16000
    ts = convert_ts_float(phoneme_timestamps)
    hit = []
    for i, (a, b) in enumerate(ts):
        if a <= t0 < b:
            hit.append(i)
        if a < t1 <= b:
            hit.append(i)
    assert len(hit) == 2
    names = phonemes.split(' ')
    label = phonemes_idx(vocab, ' '.join(names[i] for i in range(hit[0], hit[1] + 1)))
    return {"audio": crop, "audio_len": len(crop), "phoneme_label": label}
