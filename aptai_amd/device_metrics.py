"""Evaluation metrics of validate() / test() on the device (csrc/eval.hip), opt-in through `device_metrics=True` of the three
training loops.  The functions take and return DEVICE tensors and never synchronise; CPU tensors raise `AptaiHipError` (no
fallback - `aptai_amd.metrics` is the host implementation, and the yardstick of these kernels).

    tv_scores        per-track RMSE and Pearson r         metrics.tvs_metric_rmse / tvs_metric_ppc (r only, no p-value)
    frame_scores     {frames, frames equal}               torch.eq(...).sum() of the loops, metrics.evaluate_overlap
    boundary_counts  {precision_counter, recall_counter}  the counting half of metrics.get_stats
    collapse_runs    runs of equal labels collapsed       metrics.phn_frame_id2phn
    edit_distance    Levenshtein distance                 metrics.edit_distance (parity with `editdistance` unpinned, as there)

`EvalAccumulator` collects these per batch as device tensors and brings everything to the host in ONE transfer at the end of
the loop, where the existing host formulas (`metrics.get_metrics`, the numpy means / sums / stds of the loops) finish the job.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import metrics, ops
from ._lib import AptaiHipError

TV_NAMES = metrics.TV_NAMES


def _need_device(*ts):
    for t in ts:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise AptaiHipError("aptai_amd.device_metrics needs tensors on the MI355X (no CPU fallback; aptai_amd.metrics is the host path)")


def _lens_i32(lens, B, full, device):
    """int32 [B] device length vector; None = every row in full."""
    if lens is None:
        return torch.full((B,), int(full), dtype=torch.int32, device=device)
    _need_device(lens)
    return lens.reshape(-1).to(torch.int32).contiguous()


def _rows(x, dtype):
    """[B][n] view with unit inner stride of a 1-D or 2-D tensor -> (tensor, pitch)."""
    if x.dim() == 1:
        x = x[None, :]
    if x.dim() != 2:
        raise AptaiHipError(f"expected [B][n] or [n] values, got {tuple(x.shape)}")
    if x.dtype != dtype:
        x = x.to(dtype)
    if x.shape[1] == 0:
        x = torch.zeros((x.shape[0], 1), dtype=dtype, device=x.device)     # one unread slot per row
    elif x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else max(x.shape[1], 1))


def _tracks(x):
    """fp32 [B][T][C] trajectories with unit track stride -> (tensor, row pitch, rows per utterance)."""
    if x.dtype != torch.float32:
        x = x.float()
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3:
        raise AptaiHipError(f"expected [B][T][C] or [T][C] trajectories, got {tuple(x.shape)}")
    B, T, C = x.shape
    ok = x.stride(2) == 1 and x.stride(1) >= C and (B == 1 or (x.stride(0) % x.stride(1) == 0 and x.stride(0) >= T * x.stride(1)))
    if not ok or T == 0:
        x = x.contiguous()
    ld = x.stride(1) if T > 0 else C
    rows = (x.stride(0) // ld) if B > 1 else T
    return x, ld, rows


def tv_scores(tvs_gt, tvs_pred, frame_lens=None):
    """(rmse, pcc) fp64 [B][C] (or [C] for [T][C] inputs): per-track RMSE and Pearson r over the first frame_lens[b] frames, fp64
    arithmetic on the fp32 values.  NaN r for a constant track, NaN rows for an empty utterance."""
    _need_device(tvs_gt, tvs_pred)
    squeeze = tvs_gt.dim() == 2
    g, ldg, rows_g = _tracks(tvs_gt)
    p, ldp, rows_p = _tracks(tvs_pred)
    if g.shape != p.shape:
        raise AptaiHipError(f"tv_scores: shapes differ: {tuple(g.shape)} and {tuple(p.shape)}")
    B, T, C = g.shape
    lens = _lens_i32(frame_lens, B, T, g.device)
    rmse, pcc = ops.eval_tv_scores(g, ldg, rows_g, p, ldp, rows_p, lens, B, T, C)
    return (rmse[0], pcc[0]) if squeeze else (rmse, pcc)


def frame_scores(gt, pred, frame_lens=None):
    """int32 [B][2] = {frames, frames where gt == pred} over the first frame_lens[b] labels of each row."""
    _need_device(gt, pred)
    g, ldg = _rows(gt, torch.int64)
    p, ldp = _rows(pred, torch.int64)
    B, T = g.shape[0], min(g.shape[1], p.shape[1])
    if frame_lens is None and g.shape != p.shape:
        raise AptaiHipError("frame_scores: frame label sequences differ in length")
    lens = _lens_i32(frame_lens, B, T, g.device)
    return ops.eval_frame_scores(g, ldg, p, ldp, lens, B, T)


def boundary_counts(y, ny, yhat, nh, tolerance: float = 0.02):
    """int32 [B][2] = {precision_counter, recall_counter} of metrics.get_stats for y[b, :ny[b]] against yhat[b, :nh[b]] (values of
    any dtype, compared in fp64 like numpy; ny / nh None = whole rows)."""
    _need_device(y, yhat)
    yy, ldy = _rows(y, torch.float64)
    hh, ldh = _rows(yhat, torch.float64)
    B = yy.shape[0]
    n_y = _lens_i32(ny, B, y.shape[-1], yy.device)
    n_h = _lens_i32(nh, B, yhat.shape[-1], hh.device)
    return ops.eval_boundary_counts(yy, ldy, n_y, hh, ldh, n_h, B, tolerance)


def collapse_runs(x, lens=None):
    """(out int32 [B][n] zero-padded, n_out int32 [B]): metrics.phn_frame_id2phn of x[b, :lens[b]]."""
    _need_device(x)
    xx, ld = _rows(x, torch.int64)
    B = xx.shape[0]
    return ops.eval_collapse_runs(xx, ld, _lens_i32(lens, B, x.shape[-1], xx.device), B, ldo=xx.shape[1])


def edit_distance(a, a_lens, b, b_lens):
    """int32 [B]: Levenshtein distance of a[p, :a_lens[p]] and b[p, :b_lens[p]] (int32 symbols).  One side must be at most 2048
    symbols wide; it is the one the kernel keeps in registers."""
    _need_device(a, b)
    aa, lda = _rows(a, torch.int32)
    bb, ldb = _rows(b, torch.int32)
    B = aa.shape[0]
    if bb.shape[0] != B:
        raise AptaiHipError("edit_distance: the two sides hold different numbers of sequences")
    return ops.eval_edit_distance(aa, lda, _lens_i32(a_lens, B, a.shape[-1], aa.device), bb, ldb,
                                  _lens_i32(b_lens, B, b.shape[-1], bb.device), B)


class EvalAccumulator:
    """Per-batch device results of an evaluation loop, finished on the host once.

    `add_*` launch kernels and append device tensors; nothing in them waits for the device.  `result()` concatenates everything
    into one fp64 vector (int32 counts and fp32 losses are exact in fp64), copies it to the host once, and forms the loops'
    dictionaries with the host formulas (metrics.eval_summary, where the host loops end as well):

        kind       "val" (val_mean_* keys), "test" (test_{rate}_* keys), "pr_val" (mean_val_per, mean_val_loss), "pr_test"
        per        which distance feeds the PER of the TV loops: "frames_rounded" = collapsed frame labels through compute_PER's
                   two-decimal rounding (train_aptai.validate), "frames" = collapsed frame labels (train_aptai.test),
                   "edit" = the pairs given to add_edit (train_force_aptai: CTC decode against the phoneme labels)
        with_std   the std entries of train_force_aptai.test
    """

    def __init__(self, kind: str = "val", rate: Optional[str] = None, per: str = "frames", with_std: bool = False,
                 tolerance: float = 0.02, names=TV_NAMES, max_phonemes: Optional[int] = None):
        if kind not in ("val", "test", "pr_val", "pr_test"):
            raise ValueError(f"EvalAccumulator: unknown kind {kind!r}")
        if kind == "test" and rate not in ("F", "N"):
            raise ValueError("EvalAccumulator: kind='test' needs rate 'F' or 'N'")
        if per not in ("frames", "frames_rounded", "edit"):
            raise ValueError(f"EvalAccumulator: unknown per {per!r}")
        self.kind, self.rate, self.per, self.with_std, self.tolerance = kind, rate, per, with_std, tolerance
        self.names = tuple(names)
        self.max_phonemes = max_phonemes
        self._parts: Dict[str, List[torch.Tensor]] = {}
        self._lstm_device = None

    # ------------------------------------------------------------------ collecting (device, no synchronisation)
    def push(self, name: str, values: torch.Tensor) -> None:
        """Append already computed per-utterance values under `name` (what the add_* methods do with their kernels' outputs)."""
        self._parts.setdefault(name, []).append(values.detach().reshape(-1).to(torch.float64))

    def add_loss(self, loss) -> None:
        self.push("loss", loss)

    def add_tv(self, tvs_gt, tvs_pred, frame_lens=None) -> None:
        rmse, pcc = tv_scores(tvs_gt, tvs_pred, frame_lens)
        if rmse.shape[-1] != len(self.names):
            raise AptaiHipError(f"EvalAccumulator.add_tv: {rmse.shape[-1]} tracks, {len(self.names)} names")
        self.push("rmse", rmse)
        self.push("pcc", pcc)

    def add_frames(self, gt_frames, pred_frames, frame_lens=None) -> None:
        """Frame counts, boundary counts (the loops hand get_stats the frame LABEL sequences, as the reference does) and the
        Levenshtein distance of the two run-collapsed label sequences."""
        _need_device(gt_frames, pred_frames)
        B = gt_frames.shape[0] if gt_frames.dim() == 2 else 1
        lens = _lens_i32(frame_lens, B, min(gt_frames.shape[-1], pred_frames.shape[-1]), gt_frames.device)
        fs = frame_scores(gt_frames, pred_frames, lens)
        bc = boundary_counts(gt_frames, lens, pred_frames, lens, self.tolerance)
        y_grp, n_y = collapse_runs(gt_frames, lens)
        h_grp, n_h = collapse_runs(pred_frames, lens)
        self.push("frames", fs[:, 0]); self.push("correct", fs[:, 1])
        self.push("prec", bc[:, 0]); self.push("rec", bc[:, 1])
        self.push("grp_n", n_y); self.push("grp_dist", edit_distance(y_grp, n_y, h_grp, n_h))

    def add_edit(self, gt, gt_lens, pred, pred_lens) -> None:
        self.push("edit_dist", edit_distance(gt, gt_lens, pred, pred_lens))
        self.push("edit_n", _lens_i32(gt_lens, gt.shape[0] if gt.dim() == 2 else 1, gt.shape[-1], gt.device))

    def add_decoded_lengths(self, nlen) -> None:
        """Decoded phoneme counts of Force_APTAI's recogniser: checked against `max_phonemes` in result()."""
        self.push("decoded_n", nlen)

    def add_lstm_status(self, device) -> None:
        """Status words of the cooperative BiLSTM kernels after this batch (what Force_APTAI._lists reads every step)."""
        w = ops.lstm_status_words(device)
        if w is not None:
            self._lstm_device = device
            self.push("lstm_status", w)

    # ------------------------------------------------------------------ finishing (host)
    def fetch(self) -> Dict[str, np.ndarray]:
        """ONE device->host transfer: name -> fp64 numpy vector in the order the values were added."""
        names = sorted(self._parts)
        if not names:
            return {}
        cat = [torch.cat(self._parts[n]) for n in names]
        if len({str(c.device) for c in cat}) != 1:
            raise AptaiHipError("EvalAccumulator: values from more than one device")
        host = torch.cat(cat).cpu().numpy()
        out, o = {}, 0
        for n, c in zip(names, cat):
            out[n] = host[o:o + c.numel()]
            o += c.numel()
        return out

    def result(self) -> Dict[str, float]:
        h = self.fetch()
        if "lstm_status" in h:
            ops.lstm_check(h["lstm_status"].astype(np.int64).tolist(), self._lstm_device)
        if "decoded_n" in h and self.max_phonemes is not None:
            assert all(int(v) < self.max_phonemes for v in h["decoded_n"]), 'Need longer max phoneme sequence length.'
        if self.kind in ("pr_val", "pr_test"):
            d, n = self._dist(h, "edit")
            return metrics.eval_summary(self.kind, d, n, losses=h["loss"].tolist() if self.kind == "pr_val" else ())
        C = len(self.names)
        frames, correct = [int(v) for v in h["frames"]], [int(v) for v in h["correct"]]
        # get_stats: len(yhat) == len(y) == frames
        stats = [metrics.get_metrics(int(pc), int(rc), f, f) for pc, rc, f in zip(h["prec"], h["rec"], frames)]
        d, n = self._dist(h, self.per)
        return metrics.eval_summary(self.kind, d, n, losses=h["loss"].tolist() if self.kind == "val" else (),
                                    rmse=h["rmse"].reshape(-1, C).tolist(), pcc=h["pcc"].reshape(-1, C).tolist(), frames=frames,
                                    correct=correct, overlaps=[c / f for c, f in zip(correct, frames)], stats=stats, rate=self.rate,
                                    with_std=self.with_std, names=self.names)

    @staticmethod
    def _dist(h, per):
        if per == "edit":
            return [int(v) for v in h["edit_dist"]], [int(v) for v in h["edit_n"]]
        d, n = [int(v) for v in h["grp_dist"]], [int(v) for v in h["grp_n"]]
        if per == "frames_rounded":                                      # metrics.compute_PER(...) / 100.0 * len(y_grp), as the loop writes it
            d = [round(a / b * 100, 2) / 100.0 * b for a, b in zip(d, n)]
        return d, n


def frame_lengths(w2v2, audio_lengths, max_frames: int):
    """int32 [B] device frame counts of the utterances of a batch: the encoder's own length formula on `audio_lengths`, bounded
    by the frames the batch actually holds."""
    lens = w2v2._get_feat_extract_output_lengths(audio_lengths.reshape(-1))
    return lens.clamp(max=int(max_frames)).to(torch.int32).contiguous()


def label_lengths(labels):
    """int32 [B]: number of labels before the -100 padding of the collate functions."""
    return (labels >= 0).sum(dim=-1).to(torch.int32).contiguous()
