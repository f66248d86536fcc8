"""The audio front end on the device: what the reference does on the host inside `__getitem__`, once per item per epoch
(data/dataset_commonphone.py:28-33, data/dataset_hprc.py:68-70: `torchaudio.functional.resample` to 16 kHz), as one launch per
batch on the utterances' own samples (csrc/frontend.hip), plus the HF feature extractor's zero-mean / unit-variance
normalisation.  The upload is the files' PCM, packed back to back; the result is the zero-padded fp32 batch and the int64
lengths the models take.  Lengths and offsets are integer arithmetic on the host: nothing is read back from the device.

    fe = DeviceFrontend(48000)
    audio, lengths = fe([wave0, wave1, ...])             # 1-D float32 or int16 arrays / CPU tensors
    out = model(input_values=audio, input_lengths=lengths, phoneme_labels=labels)

With `speeds=` the same launch resamples every row at a factor of its own (speed perturbation, `speed_index=`), and
`raw_batch_to_device(..., augment=True)` stretches a batch's frame-level targets to match (aptai_warp_targets).

There is no CPU route: `hostlogic.resample` is the host function, the `ops` wrappers refuse CPU tensors.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hostlogic, ops

# wav2vec2's feature encoder: 320 samples per frame, the frame count the frame-level targets follow
W2V2_CONV_KERNEL, W2V2_CONV_STRIDE = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)

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
    kept on the device it is first used on.

    `speeds`: at most 8 factors in [0.5, 2.0] for speed perturbation - a row at factor f is resampled from
    hostlogic.speed_rate(orig_freq, f) instead of orig_freq (`speed_index=` of the call, `draw_speeds` with the generator seeded by
    `seed`); `conv_kernel` / `conv_stride`: the encoder's frame arithmetic, which the frame-level targets follow."""

    def __init__(self, orig_freq: int, new_freq: int = 16000, normalize: bool = False, lowpass_filter_width: int = 6,
                 rolloff: float = 0.99, speeds: Optional[Sequence[float]] = None, seed: int = 0,
                 conv_kernel: Sequence[int] = W2V2_CONV_KERNEL, conv_stride: Sequence[int] = W2V2_CONV_STRIDE):
        bank = hostlogic.resample_taps(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.orig_freq, self.new_freq, self.normalize = int(orig_freq), int(new_freq), bool(normalize)
        self.orig, self.new, self.width = int(bank["orig"]), int(bank["new"]), int(bank["width"])
        self.Kc = int(bank["taps"].shape[1])
        self._check_table(orig_freq, self.orig, self.new, self.Kc)
        self._taps_host = torch.from_numpy(bank["taps"]).float().contiguous()           # rounded as hostlogic.resample rounds its bank
        self._first_host = torch.from_numpy(bank["first"]).to(torch.int32).contiguous()
        self._tables = {}                                                               # device -> (taps, first)
        self._ring = _PinnedRing()
        # speed perturbation: one bank per factor, back to back, and the int32 table aptai_resample_batch_multi reads
        self.speeds = None
        self.last_speed_index = None                                                    # loops.to_device: what the last batch got
        self.conv_kernel, self.conv_stride = tuple(conv_kernel), tuple(conv_stride)
        self._rng = np.random.RandomState(seed)
        if speeds is not None:
            speeds = tuple(float(f) for f in speeds)
            if not 1 <= len(speeds) <= ops.RESAMPLE_MAX_RATIOS:
                raise ValueError(f"speeds: 1 .. {ops.RESAMPLE_MAX_RATIOS} factors expected, got {len(speeds)}")
            if any(not 0.5 <= f <= 2.0 for f in speeds):
                raise ValueError(f"speeds: every factor must lie in [0.5, 2.0], got {speeds}")
            table = np.zeros((len(speeds), ops.RESAMPLE_ENTRY), dtype=np.int32)
            taps, first = [], []
            for r, f in enumerate(speeds):
                rate = hostlogic.speed_rate(self.orig_freq, f)
                b = hostlogic.resample_taps(rate, new_freq, lowpass_filter_width, rolloff)
                Kc = int(b["taps"].shape[1])
                self._check_table(rate, int(b["orig"]), int(b["new"]), Kc)
                table[r, :4] = (b["orig"], b["new"], Kc, b["width"])
                if b["orig"] != b["new"]:
                    table[r, 4:6] = (sum(t.size for t in taps), sum(t.size for t in first))
                    taps.append(b["taps"].astype(np.float32).reshape(-1))
                    first.append(b["first"].astype(np.int32))
            self.speeds, self._table = speeds, table
            self._speed_taps = torch.from_numpy(np.concatenate(taps)) if taps else None
            self._speed_first = torch.from_numpy(np.concatenate(first)) if first else None
            self._speed_tables = {}                                                     # device -> (taps, first, table)

    @staticmethod
    def _check_table(rate, orig, new, Kc):
        if new * Kc > ops.RESAMPLE_MAX_TABLE:
            raise ValueError(f"{rate} -> the target rate reduces to {orig} -> {new}: a table of {new} x {Kc} taps "
                             f"exceeds the {ops.RESAMPLE_MAX_TABLE} entries the device resampler takes")

    def speed_index(self, speed_index, B: int) -> np.ndarray:
        """`speed_index` checked: int32 [B] on the host, every entry an index into `speeds`."""
        if self.speeds is None:
            raise ValueError("speed_index needs a front end built with speeds=")
        raw = np.asarray(speed_index.cpu() if torch.is_tensor(speed_index) else speed_index).reshape(-1)
        idx = raw.astype(np.int64)
        if idx.size != B or not np.array_equal(idx, raw) or (idx < 0).any() or (idx >= len(self.speeds)).any():
            raise ValueError(f"speed_index needs {B} integers in [0, {len(self.speeds)})")
        return idx.astype(np.int32)

    def draw_speeds(self, B: int) -> np.ndarray:
        """B indices into `speeds`, uniform, from the instance's own generator (`seed=`).  A host draw: the batch's width and
        lengths follow from it, and nothing is read back from the device."""
        if self.speeds is None:
            raise ValueError("draw_speeds needs a front end built with speeds=")
        return self._rng.randint(0, len(self.speeds), size=int(B)).astype(np.int32)

    def out_lengths(self, lengths, speed_index=None) -> np.ndarray:
        """ceil(new * len / orig) per utterance, int64, on the host; with `speed_index`, at every row's own ratio."""
        n = np.asarray(lengths, dtype=np.int64)
        if speed_index is None:
            return (self.new * n + self.orig - 1) // self.orig
        idx = self.speed_index(speed_index, n.size)
        orig, new = self._table[idx, 0].astype(np.int64), self._table[idx, 1].astype(np.int64)
        return (new * n.reshape(-1) + orig - 1) // orig

    def frame_counts(self, sample_lengths) -> np.ndarray:
        """Encoder frames of utterances of that many 16 kHz samples (the feature extractor's length formula), at least 0."""
        n = hostlogic.feat_extract_output_lengths(np.asarray(sample_lengths, dtype=np.int64), self.conv_kernel, self.conv_stride)
        return np.clip(n, 0, None)

    def _device_tables(self, device):
        key = str(device)
        if key not in self._tables:
            self._tables[key] = (self._taps_host.to(device), self._first_host.to(device))
        return self._tables[key]

    def _device_speed_tables(self, device):
        key = str(device)
        if key not in self._speed_tables:
            self._speed_tables[key] = (None if self._speed_taps is None else self._speed_taps.to(device),
                                       None if self._speed_first is None else self._speed_first.to(device),
                                       torch.from_numpy(self._table).to(device))
        return self._speed_tables[key]

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

    def __call__(self, waves, pad_to: Optional[int] = None, window=None, device="cuda", speed_index=None):
        """(audio fp32 [B][S], lengths int64 [B]), both on the device.  `waves`: a list of 1-D CPU tensors / arrays (packed into one
        pinned buffer and uploaded in one copy), or a (packed device tensor, host offsets [B + 1]) pair.  S = the longest output,
        or `pad_to`.  `window=(starts, n)`: n columns from output sample starts[b] of each utterance (a crop), lengths
        min(n, full length - start) clamped at 0.  `speed_index` (a front end with `speeds`): host integers [B], row b is
        resampled at speeds[speed_index[b]] - every length above is then the row's own; None runs every row at factor 1.0, the
        launch of a front end without speeds."""
        arrs = packed = None
        if isinstance(waves, tuple) and len(waves) == 2 and torch.is_tensor(waves[0]) and waves[0].is_cuda:
            packed, off = waves[0], _host_offsets(waves[1], waves[0].numel())
        else:
            arrs, off = self._arrays(list(waves))
        B = off.size - 1
        idx = None if speed_index is None else self.speed_index(speed_index, B)
        full = self.out_lengths(np.diff(off), idx)
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
        # one small upload: offsets | lengths | starts | speed indices (int32, two to a word)
        words = []
        if idx is not None:
            words = [np.zeros((B + 1) // 2, dtype=np.int64)]
            words[0].view(np.int32)[:B] = idx
        meta = np.concatenate([off, lens] + ([starts] if starts is not None else []) + words).astype(np.int64)
        meta_h = self._ring.stage(meta.size, torch.int64)
        meta_h.numpy()[:] = meta
        meta_d = meta_h.to(dev, non_blocking=True)
        self._ring.sent()
        off_d, len_d = meta_d[:B + 1], meta_d[B + 1:2 * B + 1]
        st_d = meta_d[2 * B + 1:3 * B + 1] if starts is not None else None
        out = torch.empty((B, max(S, 1)), device=dev, dtype=torch.float32)[:, :S]
        ncols = S if crop is None else crop
        if S > ncols:
            out[:, ncols:].zero_()
        if ncols > 0 and idx is not None:
            taps, first, table = self._device_speed_tables(dev)
            idx_d = meta_d[meta.size - (B + 1) // 2:].view(torch.int32)[:B]
            ops.resample_batch_multi(packed, off_d, B, taps, first, table, self._table, idx_d, idx, out, ncols, st_d)
        elif ncols > 0:
            taps, first = self._device_tables(dev) if self.orig != self.new else (None, None)
            ops.resample_batch(packed, off_d, B, taps, first, self.orig, self.new, self.Kc, self.width, out, ncols, st_d)
        if ncols > 0 and self.normalize:
            ops.wave_normalize(out, len_d, S)
        return out, len_d


def raw_batch_to_device(batch: Dict[str, torch.Tensor], frontend: DeviceFrontend, device, audio_key: str, length_key: str,
                        host_lengths: bool = False, augment: bool = False, speed_index=None) -> Dict[str, torch.Tensor]:
    """A `collate_*_raw` batch (audio_packed + audio_offsets) -> the batch the model takes: every other entry moved to `device`,
    the packed audio uploaded as it is and resampled there into `audio_key`, the 16 kHz lengths under `length_key` (a host tensor
    with `host_lengths`, for the graphed runners, which size their buckets on the host).

    `augment` on a front end with `speeds`: speed perturbation.  Row b is resampled at speeds[i_b], i = `speed_index` or
    `frontend.draw_speeds(B)`, and the frame-level entries (`phn_frames_49hz`, the TV tracks) are stretched with it in one launch
    (aptai_warp_targets): from the frames of the row's unperturbed 16 kHz length (at most the tensor's width) to the frames of its
    perturbed length, padded to the longest, dtypes kept.  `phoneme_labels` stay (a fast utterance may then have fewer frames than
    labels; the CTC and forward-sum losses count such a row as zero).  The lengths are the perturbed ones and `_speed_index`
    (host int32 [B]) records what was applied.  Without `speeds`, or without `augment`, nothing changes."""
    out = {k: v.to(device) for k, v in batch.items() if k not in ("audio_packed", "audio_offsets")}
    packed = batch["audio_packed"]
    raw = np.diff(_host_offsets(batch["audio_offsets"], None if packed.is_cuda else packed.numel()))
    idx = None
    if augment and frontend.speeds is not None:
        idx = frontend.draw_speeds(raw.size) if speed_index is None else frontend.speed_index(speed_index, raw.size)
    if not packed.is_cuda:
        packed = frontend.upload_packed(packed, device)
    audio, lens = frontend((packed, batch["audio_offsets"]), speed_index=idx)
    if idx is not None:                                     # before the audio joins `out`: what is [B][T] and floating there is a track
        _warp_frame_targets(out, frontend, raw, idx, audio.device)
        out["_speed_index"] = torch.from_numpy(idx)
    out[audio_key] = audio
    out[length_key] = torch.from_numpy(frontend.out_lengths(raw, idx)) if host_lengths else lens
    return out


def _warp_frame_targets(out, frontend, raw, idx, device) -> None:
    """The frame-level entries of `out` (device tensors [B][T_in]) replaced by their stretched versions [B][max n_out]."""
    tracks = [k for k, v in out.items() if k != "phn_frames_49hz" and v.dim() == 2 and v.is_floating_point() and v.shape[0] == raw.size]
    labels = "phn_frames_49hz" if "phn_frames_49hz" in out else None
    if not tracks and labels is None:
        return
    B = raw.size
    T_in = out[labels].shape[1] if labels is not None else out[tracks[0]].shape[1]
    if any(out[k].shape[1] != T_in for k in tracks):
        raise ValueError("the frame-level entries of a batch must have one width")
    n_in = np.minimum(frontend.frame_counts(frontend.out_lengths(raw)), T_in)
    n_out = frontend.frame_counts(frontend.out_lengths(raw, idx))
    T_out = int(n_out.max())
    rows = len(tracks) + (1 if labels is not None else 0)
    meta = frontend._ring.stage(2 * rows * B, torch.int64)
    meta.numpy()[:] = np.concatenate([np.tile(n_in, rows), np.tile(n_out, rows)])
    meta_d = meta.to(device, non_blocking=True)
    frontend._ring.sent()
    trk = torch.stack([out[k].double() for k in tracks]).reshape(len(tracks) * B, T_in).contiguous() if tracks else None
    lab = out[labels].long().contiguous() if labels is not None else None
    trk_w, lab_w = ops.warp_targets(trk, lab, meta_d[:rows * B], meta_d[rows * B:], T_out)
    for j, k in enumerate(tracks):
        out[k] = trk_w[j * B:(j + 1) * B].to(out[k].dtype)
    if labels is not None:
        out[labels] = lab_w.to(out[labels].dtype)


def parse_speeds(speeds) -> Optional[Tuple[float, ...]]:
    """cfg.speed_perturb / --speed_perturb: None, '0.9,1.0,1.1' or a sequence of factors -> a tuple of floats (None when empty)."""
    if speeds is None or (isinstance(speeds, (str, tuple, list)) and len(speeds) == 0):
        return None
    if isinstance(speeds, str):
        speeds = [s for s in speeds.split(",") if s.strip()]
    return tuple(float(f) for f in speeds)


def uses_frontend(cfg) -> bool:
    """Whether the loops take `collate_*_raw` batches through a device front end: any of source_rate, normalize_audio and
    speed_perturb set (`cfg`: a loop cfg or the parsed command line)."""
    return bool(getattr(cfg, "source_rate", None) or getattr(cfg, "normalize_audio", False) or parse_speeds(getattr(cfg, "speed_perturb", None)))


def make_frontend(cfg, rank: int = 0) -> Optional[DeviceFrontend]:
    """The training loops' opt-in: with `cfg.source_rate` (the corpus' rate), `cfg.normalize_audio` or `cfg.speed_perturb` set
    the batches are `collate_*_raw` ones and pass through this front end; None with all three unset.  The speed draws are seeded
    with cfg.speed_perturb_seed + `rank` (a data-parallel rank draws its own)."""
    if not uses_frontend(cfg):
        return None
    rate, speeds = getattr(cfg, "source_rate", None), parse_speeds(getattr(cfg, "speed_perturb", None))
    if speeds is None:
        return DeviceFrontend(int(rate or 16000), 16000, normalize=bool(getattr(cfg, "normalize_audio", False)))
    w2v = getattr(cfg, "pretrain_cfg", None)
    geometry = {"conv_kernel": w2v.conv_kernel, "conv_stride": w2v.conv_stride} if hasattr(w2v, "conv_kernel") else {}
    return DeviceFrontend(int(rate or 16000), 16000, normalize=bool(getattr(cfg, "normalize_audio", False)), speeds=speeds,
                          seed=int(getattr(cfg, "speed_perturb_seed", 0) or 0) + int(rank), **geometry)
