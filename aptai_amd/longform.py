"""Long recordings: overlapped-window inference, stitched on the device ("Long recordings").

The models are trained on clips of at most 10 s (499 frames); a recording of a minute pushed through one forward runs self-attention
over a context the weights have never seen, at a cost that grows with T^2.  `LongFormRun` is what `APTAI.get_aptai_output[s]_long` and
`Wav2Vec2_PR.*_long` share: the window plans of a list of recordings (hostlogic.long_form_plan), their samples packed on the device,
the windows cut out of them in groups (aptai_window_gather) for the models' existing eval-mode, batch-invariant forward, and the
per-window results stitched into one row of frames per recording (aptai_stitch_windows).  Every window of every recording is padded
to the same sample count, so every group has the geometry of the first and a window's result does not depend on its group.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hostlogic, ops

_EXACT = ("f32x3", "f32x6")


def as_wave(wav) -> torch.Tensor:
    """One waveform as the short helpers take it (a (1, n) tensor counts as its first row) -> 1-D float32 on the host."""
    if isinstance(wav, torch.Tensor):
        return (wav[0] if wav.dim() > 1 else wav).detach().to("cpu", torch.float32).reshape(-1)
    return torch.as_tensor(np.asarray(wav), dtype=torch.float32).reshape(-1)


class LongFormRun:
    def __init__(self, wavs, encoder, device, window_frames=499, hop_frames=399, trim_frames=25, ramp="linear"):
        if encoder.encoder_precision in _EXACT:
            raise NotImplementedError(f"long-form inference is not available with encoder precision {encoder.encoder_precision!r}: "
                                      f"the windows run through the bf16-class forwards (not {', '.join(map(repr, _EXACT))})")
        cfg = encoder.config
        wavs = [as_wave(w) for w in wavs]
        self.plans = [hostlogic.long_form_plan(w.numel(), cfg.conv_kernel, cfg.conv_stride, window_frames, hop_frames, trim_frames)
                      for w in wavs]
        seams = [p for p in self.plans if p.K > 0]
        table = hostlogic.long_form_ramp(seams[0] if seams else self.plans[0], ramp)       # validates `ramp` for every plan
        self.window_frames, self.hop_frames = int(window_frames), int(hop_frames)
        self.frames = [p.frames for p in self.plans]
        self.max_frames = max(self.frames)
        self.S = max(max(p.sample_count) for p in self.plans)
        self.n_rec = len(self.plans)

        # one int64 upload: the window table, then the recording table for packed rows and the one for n_rec rows of max_frames
        win, rec_packed, rec_rows, off, w0, f0 = [], [], [], 0, 0, 0
        for r, p in enumerate(self.plans):
            win += [(off, a, n) for a, n in zip(p.sample_start, p.sample_count)]
            rec_packed.append((w0, p.frames, f0))
            rec_rows.append((w0, p.frames, r * self.max_frames))
            off, w0, f0 = off + p.n_samples, w0 + p.K + 1, f0 + p.frames
        self.n_windows, self.total_frames = w0, f0
        self.row_start = [e[2] for e in rec_packed]
        tables = torch.tensor(win + rec_packed + rec_rows, dtype=torch.int64).to(device)
        self.table = tables[:w0]
        self._rec_packed, self._rec_rows = tables[w0:w0 + self.n_rec], tables[w0 + self.n_rec:]
        self.packed = torch.cat(wavs).to(device)
        self.ramp = torch.from_numpy(table).to(device) if seams and table.size else None

    def groups(self, windows_per_forward: int):
        """(first, rows) of every forward: at most `windows_per_forward` windows each, the windows of all recordings in one row."""
        n = int(windows_per_forward)
        if n < 1:
            raise ValueError(f"windows_per_forward must be at least 1, not {windows_per_forward}")
        return [(a, min(n, self.n_windows - a)) for a in range(0, self.n_windows, n)]

    def gather(self, first: int, rows: int):
        """(audio fp32 [rows][S] zero-padded, lens int64 [rows]) of a group, on the device."""
        return ops.window_gather(self.packed, self.table, first, rows, self.S)

    def collect(self, store, part, first: int, rows: int):
        """The results `part` of a group (leading dimension: rows x whatever a window has) kept until every window has run: the
        only group's own tensor, or a buffer for all windows that the groups are copied into (a seam between two groups needs both)."""
        if rows == self.n_windows:
            return part
        m = part.shape[0] // rows
        if store is None:
            store = torch.empty((self.n_windows * m,) + tuple(part.shape[1:]), device=part.device, dtype=part.dtype)
        store[first * m:(first + rows) * m] = part
        return store

    def stitch(self, x, ldx: int, rows_per_window: int, C: int, *, per_recording_rows=False, ldo=None, want_argmax=True):
        """ops.stitch_windows over the results of all windows.  Rows of the output: the recordings back to back ([sum F][ldo]), or
        with `per_recording_rows` one block of max_frames rows per recording ([n_rec * max_frames][ldo], zeros where a recording ends):
        the layout the CTC read-outs take."""
        rec = self._rec_rows if per_recording_rows else self._rec_packed
        out_rows = self.n_rec * self.max_frames if per_recording_rows else self.total_frames
        return ops.stitch_windows(x, ldx, rows_per_window, self.n_windows, rec, self.max_frames, self.window_frames, self.hop_frames,
                                  self.ramp, C, out_rows=out_rows, ldo=ldo, want_argmax=want_argmax)

    def frames_i32(self) -> torch.Tensor:
        """Frame count of every recording, int32 on the device (a view of the uploaded table, cast there)."""
        return self._rec_packed[:, 1].to(torch.int32).contiguous()
