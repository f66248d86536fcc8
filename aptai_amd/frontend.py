"""The audio front end on the device: what the reference does on the host inside `__getitem__`, once per item per epoch
(data/dataset_commonphone.py:28-33, data/dataset_hprc.py:68-70: `torchaudio.functional.resample` to 16 kHz), as one launch per
batch on the utterances' own samples (csrc/frontend.hip), plus the HF feature extractor's zero-mean / unit-variance
normalisation.  The upload is the files' PCM, packed back to back; the result is the zero-padded fp32 batch and the int64
lengths the models take.  Lengths and offsets are integer arithmetic on the host: nothing is read back from the device.

    fe = DeviceFrontend(48000)
    audio, lengths = fe([wave0, wave1, ...])             # 1-D float32 or int16 arrays / CPU tensors
    out = model(input_values=audio, input_lengths=lengths, phoneme_labels=labels)

There is no CPU route: `hostlogic.resample` is the host function, the `ops` wrappers refuse CPU tensors.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hostlogic, ops


def _host_offsets(offsets, numel: Optional[int] = None) -> np.ndarray:
    """int64 offsets [B + 1] on the host, checked: non-decreasing, from >= 0, and (with `numel`) inside the packed buffer - the
    kernel reads wherever they point."""
    off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
    if off.size < 2 or (np.diff(off) < 0).any() or off[0] < 0:
        raise ValueError("offsets must be B + 1 non-decreasing sample positions starting at or above 0")
    if numel is not None and off[-1] > numel:
        raise ValueError(f"offsets end at sample {int(off[-1])}, the packed buffer holds {numel}")
    return off


class _PinnedRing:
    """Two pinned staging buffers per dtype, grown on demand and reused: pinning a fresh buffer per batch costs more than the copy
    it speeds up.  A slot is handed out again only after the copy that last read it has finished (an event per slot)."""

    def __init__(self):
        self._slots = {}                                   # dtype -> [[buffer, event], [buffer, event]]
        self._turn = {}

    def stage(self, numel: int, dtype) -> torch.Tensor:
        slots = self._slots.setdefault(dtype, [[None, None], [None, None]])
        i = self._turn.get(dtype, 0)
        self._turn[dtype] = i ^ 1
        slot = slots[i]
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < numel:
            slot[0] = torch.empty(max(numel, 1024) * 5 // 4, dtype=dtype).pin_memory()
        self._last = slot
        return slot[0][:numel]

    def sent(self) -> None:
        """Call after the asynchronous copy out of the buffer `stage` returned last has been enqueued."""
        ev = torch.cuda.Event()
        ev.record()
        self._last[1] = ev


class DeviceFrontend:
    """`orig_freq` -> `new_freq` resampling (torchaudio's sinc_interp_hann defaults, the filter bank of hostlogic.resample) and,
    with `normalize`, zero_mean_unit_var_norm, for whole batches on the device.  The taps table is built once per instance and
    kept on the device it is first used on."""

    def __init__(self, orig_freq: int, new_freq: int = 16000, normalize: bool = False, lowpass_filter_width: int = 6,
                 rolloff: float = 0.99):
        bank = hostlogic.resample_taps(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.orig_freq, self.new_freq, self.normalize = int(orig_freq), int(new_freq), bool(normalize)
        self.orig, self.new, self.width = int(bank["orig"]), int(bank["new"]), int(bank["width"])
        self.Kc = int(bank["taps"].shape[1])
        if self.new * self.Kc > ops.RESAMPLE_MAX_TABLE:
            raise ValueError(f"{orig_freq} -> {new_freq} reduces to {self.orig} -> {self.new}: a table of {self.new} x {self.Kc} taps "
                             f"exceeds the {ops.RESAMPLE_MAX_TABLE} entries the device resampler takes")
        self._taps_host = torch.from_numpy(bank["taps"]).float().contiguous()           # rounded as hostlogic.resample rounds its bank
        self._first_host = torch.from_numpy(bank["first"]).to(torch.int32).contiguous()
        self._tables = {}                                                               # device -> (taps, first)
        self._ring = _PinnedRing()

    def out_lengths(self, lengths) -> np.ndarray:
        """ceil(new * len / orig) per utterance, int64, on the host."""
        n = np.asarray(lengths, dtype=np.int64)
        return (self.new * n + self.orig - 1) // self.orig

    def _device_tables(self, device):
        key = str(device)
        if key not in self._tables:
            self._tables[key] = (self._taps_host.to(device), self._first_host.to(device))
        return self._tables[key]

    @staticmethod
    def _arrays(waves: Sequence):
        """1-D float32 / int16 arrays or CPU tensors -> (numpy views, int64 offsets [B + 1])."""
        arrs = [w.detach().numpy() if torch.is_tensor(w) else np.asarray(w) for w in waves]
        if not arrs:
            raise ValueError("an empty batch")
        if any(a.ndim != 1 for a in arrs) or len({a.dtype for a in arrs}) != 1 or arrs[0].dtype not in (np.float32, np.int16):
            raise ValueError("waves must be 1-D and all float32 or all int16")
        off = np.zeros(len(arrs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([a.shape[0] for a in arrs])
        return arrs, off

    def _upload(self, arrs, off, device) -> torch.Tensor:
        """The utterances back to back through a reused pinned buffer, one asynchronous copy (8 spare elements at the end: an
        all-empty batch still has a pointer; the offsets say where the audio ends)."""
        n = int(off[-1])
        host = self._ring.stage(n + 8, torch.from_numpy(arrs[0][:0]).dtype)
        view = host.numpy()
        for a, o in zip(arrs, off[:-1]):
            view[o:o + a.shape[0]] = a
        view[n:] = 0
        dev = host.to(device, non_blocking=True)
        self._ring.sent()
        return dev

    def upload_packed(self, packed: torch.Tensor, device) -> torch.Tensor:
        """A packed 1-D CPU tensor (a `collate_*_raw` batch) through the same pinned buffer."""
        n = packed.numel()
        host = self._ring.stage(n + 8, packed.dtype)
        host[:n].copy_(packed.reshape(-1))
        host[n:].zero_()
        dev = host.to(device, non_blocking=True)
        self._ring.sent()
        return dev

    def __call__(self, waves, pad_to: Optional[int] = None, window=None, device="cuda"):
        """(audio fp32 [B][S], lengths int64 [B]), both on the device.  `waves`: a list of 1-D CPU tensors / arrays (packed into one
        pinned buffer and uploaded in one copy), or a (packed device tensor, host offsets [B + 1]) pair.  S = the longest output,
        or `pad_to`.  `window=(starts, n)`: n columns from output sample starts[b] of each utterance (a crop), lengths
        min(n, full length - start) clamped at 0."""
        arrs = packed = None
        if isinstance(waves, tuple) and len(waves) == 2 and torch.is_tensor(waves[0]) and waves[0].is_cuda:
            packed, off = waves[0], _host_offsets(waves[1], waves[0].numel())
        else:
            arrs, off = self._arrays(list(waves))
        B = off.size - 1
        full = self.out_lengths(np.diff(off))
        starts = None
        if window is not None:
            st, n = window
            st = np.asarray(st.cpu() if torch.is_tensor(st) else st, dtype=np.int64).reshape(-1)
            if st.size != B or (st < 0).any() or int(n) < 0:
                raise ValueError(f"window=(starts, n) needs {B} non-negative starts and n >= 0")
            lens, S, starts = np.clip(np.minimum(int(n), full - st), 0, None), int(n), st
        else:
            lens, S = full, int(full.max())
        crop = S if window is not None else None                # a crop is n columns wide whatever the padding: the rest is zeros
        if pad_to is not None:
            if int(pad_to) < S:
                raise ValueError(f"pad_to={pad_to} is shorter than the longest output ({S} samples)")
            S = int(pad_to)
        if packed is None:
            packed = self._upload(arrs, off, device)
        dev = packed.device
        # one small upload: offsets | lengths | starts
        meta = np.concatenate([off, lens] + ([starts] if starts is not None else [])).astype(np.int64)
        meta_h = self._ring.stage(meta.size, torch.int64)
        meta_h.numpy()[:] = meta
        meta_d = meta_h.to(dev, non_blocking=True)
        self._ring.sent()
        off_d, len_d = meta_d[:B + 1], meta_d[B + 1:2 * B + 1]
        st_d = meta_d[2 * B + 1:] if starts is not None else None
        out = torch.empty((B, max(S, 1)), device=dev, dtype=torch.float32)[:, :S]
        ncols = S if crop is None else crop
        if S > ncols:
            out[:, ncols:].zero_()
        if ncols > 0:
            taps, first = self._device_tables(dev) if self.orig != self.new else (None, None)
            ops.resample_batch(packed, off_d, B, taps, first, self.orig, self.new, self.Kc, self.width, out, ncols, st_d)
            if self.normalize:
                ops.wave_normalize(out, len_d, S)
        return out, len_d


def raw_batch_to_device(batch: Dict[str, torch.Tensor], frontend: DeviceFrontend, device, audio_key: str, length_key: str,
                        host_lengths: bool = False) -> Dict[str, torch.Tensor]:
    """A `collate_*_raw` batch (audio_packed + audio_offsets) -> the batch the model takes: every other entry moved to `device`,
    the packed audio uploaded as it is and resampled there into `audio_key`, the 16 kHz lengths under `length_key` (a host tensor
    with `host_lengths`, for the graphed runners, which size their buckets on the host)."""
    out = {k: v.to(device) for k, v in batch.items() if k not in ("audio_packed", "audio_offsets")}
    packed = batch["audio_packed"]
    if not packed.is_cuda:
        _host_offsets(batch["audio_offsets"], packed.numel())
        packed = frontend.upload_packed(packed, device)
    audio, lens = frontend((packed, batch["audio_offsets"]))
    out[audio_key] = audio
    out[length_key] = torch.from_numpy(frontend.out_lengths(np.diff(_host_offsets(batch["audio_offsets"])))) if host_lengths else lens
    return out


def make_frontend(cfg) -> Optional[DeviceFrontend]:
    """The training loops' opt-in: with `cfg.source_rate` (the corpus' rate) or `cfg.normalize_audio` set the batches are
    `collate_*_raw` ones and pass through this front end; None with both unset."""
    rate, norm = getattr(cfg, "source_rate", None), bool(getattr(cfg, "normalize_audio", False))
    if not rate and not norm:
        return None
    return DeviceFrontend(int(rate or 16000), 16000, normalize=bool(getattr(cfg, "normalize_audio", False)))
