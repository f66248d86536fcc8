"""CPU: the host side of the device audio front end (aptai_amd.frontend, csrc/frontend.hip): the entry points are declared,
exported and typed; the compact filter bank of hostlogic.resample_taps evaluates to the published resampling formula; output
lengths; the raw collates; argument errors.  The device side is tests/test_gpu_frontend.py.

Yardstick (written here from the published formula, independent of resample_taps): for output n of an utterance x at the reduced
ratio orig -> new,  y64[n] = sum_i x[i] h((i / orig - n / new) base),  base = min(orig, new) rolloff,
h(t) = sinc(pi t) cos^2(pi t / (2 lw)) base / orig for |t| < lw, else 0.

Bound for fp32 results (derived, not tuned): an fp32 dot product of Kc terms with taps rounded to fp32 is within
(Kc + 2) 2^-24 A max|x| of the exact one, A = max_p sum_j |taps64[p][j]| taken from the yardstick's own taps."""
import math

import numpy as np
import pytest
import torch

from aptai_amd import hostlogic

NEW = ("aptai_resample_batch", "aptai_wave_normalize", "aptai_wave_normalize_workspace_bytes")
RATES = (48000, 44100, 22050, 8000, 11025)
LENGTHS = (1, 5, 37, 1000, 2000)
LW, ROLLOFF = 6, 0.99


def reduced(orig_freq, new_freq=16000):
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def h_kernel(t, orig, base):
    """h of the docstring, fp64, for an array of t."""
    t = np.asarray(t, dtype=np.float64)
    pt = np.pi * t
    sinc = np.where(pt == 0, 1.0, np.sin(pt) / np.where(pt == 0, 1.0, pt))
    return np.where(np.abs(t) < LW, sinc * np.cos(pt / (2 * LW)) ** 2 * (base / orig), 0.0)


def direct_resample(x, orig_freq, new_freq=16000, n_from=0, n_to=None):
    """(y64 [n_from, n_to), A): the yardstick on the reduced ratio, only over the input samples whose h is not zero."""
    orig, new = reduced(orig_freq, new_freq)
    x = np.asarray(x, dtype=np.float64)
    base = min(orig, new) * ROLLOFF
    n_out = (new * len(x) + orig - 1) // orig
    n_to = n_out if n_to is None else min(n_to, n_out)
    half = int(math.ceil(LW * orig / base)) + 1
    n = np.arange(n_from, max(n_to, n_from), dtype=np.int64)
    centre = (n * orig) // new
    i = centre[:, None] + np.arange(-half - 1, half + 2, dtype=np.int64)[None, :]
    w = h_kernel((i / orig - n[:, None] / new) * base, orig, base)
    xi = np.where((i >= 0) & (i < len(x)), x[np.clip(i, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
    # A over the new phases: the taps of phase p are those of output n = p
    p = np.arange(new, dtype=np.int64)
    ip = ((p * orig) // new)[:, None] + np.arange(-half - 1, half + 2, dtype=np.int64)[None, :]
    A = float(np.abs(h_kernel((ip / orig - p[:, None] / new) * base, orig, base)).sum(axis=1).max())
    return (w * xi).sum(axis=1), A


def compact_eval(x, bank):
    """The compact form of hostlogic.resample_taps in numpy fp64: y[q new + p] = sum_j taps[p][j] x[q orig + first[p] + j - width]."""
    taps, first, orig, new, width = bank["taps"], bank["first"], bank["orig"], bank["new"], bank["width"]
    x = np.asarray(x, dtype=np.float64)
    n = np.arange((new * len(x) + orig - 1) // orig, dtype=np.int64)
    q, p = n // new, n % new
    idx = (q * orig + first[p] - width)[:, None] + np.arange(taps.shape[1], dtype=np.int64)[None, :]
    xi = np.where((idx >= 0) & (idx < len(x)), x[np.clip(idx, 0, len(x) - 1)], 0.0)
    return (taps[p] * xi).sum(axis=1)


def test_new_entry_points_are_declared_exported_and_typed():
    from aptai_amd import _lib, ops
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in NEW:
        assert n in names and n in _lib.ARGTYPES and hasattr(L, n), n
        assert getattr(L, n).argtypes == _lib.ARGTYPES[n]
    assert L.aptai_wave_normalize_workspace_bytes.restype is not None
    for w in ("resample_batch", "wave_normalize"):
        assert callable(getattr(ops, w))
    from aptai_amd import frontend
    assert callable(frontend.DeviceFrontend)


@pytest.mark.parametrize("rate", RATES)
def test_resample_taps_compact_bank(rate):
    bank = hostlogic.resample_taps(rate, 16000)
    orig, new = reduced(rate)
    assert (bank["orig"], bank["new"]) == (orig, new)
    taps, first = bank["taps"], bank["first"]
    Kc = taps.shape[1]
    assert taps.dtype == np.float64 and taps.shape[0] == new and first.shape == (new,)
    assert Kc <= 2 * bank["width"] + 1 and Kc % 2 == 1
    assert first.min() >= 0 and (first + Kc).max() <= 2 * bank["width"] + orig
    g = np.random.RandomState(rate)
    for n in LENGTHS:
        x = g.randn(n)
        y64, A = direct_resample(x, rate)
        assert 1.0 < A < 2.5
        yc = compact_eval(x, bank)
        assert yc.shape == y64.shape == (hostlogic.resample_out_length(n, orig, new),)
        assert np.abs(yc - y64).max() <= 1e-12 * np.abs(x).max()
        yh = hostlogic.resample(x.astype(np.float32), rate, 16000).double().numpy()
        x32 = x.astype(np.float32).astype(np.float64)
        y64_32, _ = direct_resample(x32, rate)
        bound = (Kc + 2) * 2.0 ** -24 * A * np.abs(x32).max()
        assert yh.shape == y64.shape
        assert np.abs(yh - y64_32).max() <= bound, (np.abs(yh - y64_32).max(), bound)


def test_resample_taps_identity_and_errors():
    bank = hostlogic.resample_taps(16000, 16000)
    assert (bank["orig"], bank["new"], bank["width"]) == (1, 1, 0) and bank["taps"].tolist() == [[1.0]] and bank["first"].tolist() == [0]
    with pytest.raises(ValueError):
        hostlogic.resample_taps(0, 16000)
    big = hostlogic.resample_taps(16001, 16000)              # a table beyond LDS, built row by row
    assert big["taps"].shape[0] == 16000 and big["taps"].shape[1] <= 2 * big["width"] + 1
    x = np.random.RandomState(3).randn(40)
    y64, _ = direct_resample(x, 16001)
    assert np.abs(compact_eval(x, big) - y64).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("rate", RATES + (16001, 16000))
def test_output_lengths(rate):
    from aptai_amd.frontend import DeviceFrontend
    orig, new = reduced(rate)
    fe = DeviceFrontend(rate)
    lens = sorted({k * orig + r for k in (0, 1, 7) for r in range(orig) if (new * (k * orig + r)) % orig in (0, 1, orig - 1)})[:60]
    assert {(new * n) % orig for n in lens} >= {0, 1 % orig, (orig - 1) % orig}
    for n in lens:
        want = -((-new * n) // orig)                                           # ceil in integers
        assert hostlogic.resample_out_length(n, orig, new) == want == int(fe.out_lengths([n])[0])
        if rate != 16001 and n <= 2000:
            assert hostlogic.resample(np.zeros(n, dtype=np.float32), rate, 16000).shape[0] == want


def _items(n, seed, labels):
    g = np.random.RandomState(seed)
    out = []
    for i in range(n):
        L, T = int(g.randint(1, 3000)), int(g.randint(2, 9))
        it = {"audio": g.randn(L).astype(np.float32), "audio_len": L, "phn_frames_49hz": g.randint(1, 40, size=T).astype(np.int64),
              "tvs_norm_49hz": {k: g.randn(T) for k in hostlogic.TV_NAMES}}
        if labels:
            it["phoneme_label"] = g.randint(1, 40, size=int(g.randint(1, 7))).astype(np.int32)
        out.append(it)
    return out


def test_raw_collates_carry_the_same_labels_and_targets():
    items = _items(4, 0, True)
    for raw, ref in ((hostlogic.collate_pr_raw(items), hostlogic.collate_pr(items)),
                     (hostlogic.collate_aptai_raw(items), hostlogic.collate_aptai(items)),
                     (hostlogic.collate_aptai_raw(items, with_phoneme_labels=True), hostlogic.collate_aptai(items, with_phoneme_labels=True))):
        audio_keys = {"input_values", "input_lengths", "audio_inputs", "audio_lengths"}
        assert set(raw) - {"audio_packed", "audio_offsets"} == set(ref) - audio_keys
        for k in set(ref) - audio_keys:
            assert raw[k].dtype == ref[k].dtype and torch.equal(raw[k], ref[k]), k
        lens = [it["audio_len"] for it in items]
        assert raw["audio_offsets"].dtype == torch.int64 and raw["audio_offsets"].tolist() == [0] + np.cumsum(lens).tolist()
        assert raw["audio_packed"].dtype == torch.float32
        assert torch.equal(raw["audio_packed"], torch.cat([torch.from_numpy(it["audio"]) for it in items]))
    pcm = [dict(it, audio=(it["audio"] * 1000).astype(np.int16)) for it in items]
    assert hostlogic.collate_pr_raw(pcm)["audio_packed"].dtype == torch.int16


def test_device_frontend_argument_errors():
    from aptai_amd import ops
    from aptai_amd._lib import AptaiHipError
    from aptai_amd.frontend import DeviceFrontend
    fe = DeviceFrontend(48000)
    waves = [np.zeros(300, dtype=np.float32), np.zeros(30, dtype=np.float32)]
    with pytest.raises(ValueError, match="pad_to"):
        fe(waves, pad_to=99)                                                   # the longest output has 100 samples
    with pytest.raises(ValueError):
        fe([np.zeros(3, dtype=np.float64)])
    with pytest.raises(ValueError):
        fe(waves, window=([0], 10))
    with pytest.raises(ValueError, match="table"):
        DeviceFrontend(400001, 400000)                                         # coprime: 400000 x 13 taps > 2^22 entries
    x = torch.zeros(2, 16)
    with pytest.raises(AptaiHipError):
        ops.resample_batch(torch.zeros(32), torch.tensor([0, 16, 32]), 2, None, None, 1, 1, 1, 0, x, 16)
    with pytest.raises(AptaiHipError):
        ops.wave_normalize(x, torch.tensor([16, 16]))
