"""GPU: the device audio front end (aptai_amd.frontend.DeviceFrontend, csrc/frontend.hip) - batched resampling of a packed
buffer and the feature extractor's normalisation - against the fp64 yardstick and bound of tests/test_cpu_frontend.py:

    |y - y64| <= (Kc + 2) 2^-24 A max|x_b|,   A = max_p sum_j |taps64[p][j]| from the yardstick's own taps

(an fp32 dot product of Kc terms with taps rounded to fp32).  The batch: five utterances of 1, 40, 0, 4411 and 22050 samples in
one packed buffer; the kernel's tile is 1024 outputs, so the longest utterance spans 7 tiles at 48 kHz, 8 at 44.1 kHz (the last
one partial in both), 16 at 22.05 kHz and 44 at 8 kHz.  400 kHz (25 -> 1, 303 taps) shrinks the tile to 256 outputs (4 tiles, the
last one partial) whose source span of 6703 samples still exceeds the 6144 staged in LDS, so the last outputs of every full tile
take their operands from global memory: the only case here that runs that path.  Every device result is computed once per module
and shared."""
import functools
import math

import numpy as np
import pytest
import torch

from test_cpu_frontend import direct_resample, reduced

pytestmark = pytest.mark.gpu

LENS = [1, 40, 0, 4411, 22050]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def waves(kind="f32"):
    g = np.random.RandomState(20240)
    if kind == "f32":
        return tuple(g.randn(n).astype(np.float32) for n in LENS)
    out = [g.randint(-32768, 32768, size=n).astype(np.int16) for n in LENS]
    out[4][:4] = [-32768, 32767, -32768, 32767]
    out[3][-2:] = [32767, -32768]
    out[0][0] = -32768
    return tuple(out)


@functools.lru_cache(maxsize=None)
def frontend(rate, normalize=False):
    from aptai_amd.frontend import DeviceFrontend
    return DeviceFrontend(rate, 16000, normalize=normalize)


@functools.lru_cache(maxsize=None)
def device_result(rate, kind="f32", normalize=False):
    audio, lens = frontend(rate, normalize)(list(waves(kind)))
    torch.cuda.synchronize()
    return audio, lens


def as_float64(w):
    return w.astype(np.float64) / 32768.0 if w.dtype == np.int16 else w.astype(np.float64)


def out_len(n, rate):
    orig, new = reduced(rate)
    return (new * n + orig - 1) // orig


def check_against_yardstick(rate, kind):
    audio, lens = device_result(rate, kind)
    fe = frontend(rate)
    want_lens = [out_len(n, rate) for n in LENS]
    assert lens.dtype == torch.int64 and lens.is_cuda and lens.tolist() == want_lens
    assert audio.dtype == torch.float32 and audio.is_cuda and tuple(audio.shape) == (len(LENS), max(want_lens))
    got = audio.cpu().numpy().astype(np.float64)
    for b, w in enumerate(waves(kind)):
        x = as_float64(w)
        y64, A = direct_resample(x, rate)
        assert y64.shape[0] == want_lens[b]
        if len(x) == 0:
            continue
        bound = (fe.Kc + 2) * 2.0 ** -24 * A * np.abs(x).max()
        err = np.abs(got[b, :want_lens[b]] - y64).max()
        print(f"rate {rate} {kind} utterance {b}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (rate, b, err, bound)


@pytest.mark.parametrize("rate", [48000, 44100, 22050, 8000, 16001, 400000])
def test_ratios_float32(rate):
    """16001 -> 16000 has a table of 16000 x 13 taps: beyond LDS, read through L2.  400000 -> 16000: see the module docstring."""
    check_against_yardstick(rate, "f32")


def test_steep_ratio_int16_and_isolation():
    """The global-memory path with an int16 source, and its bits against each utterance alone."""
    check_against_yardstick(400000, "i16")
    for kind in ("f32", "i16"):
        full = device_result(400000, kind)[0]
        for b, w in enumerate(waves(kind)):
            alone, _ = frontend(400000)([w])
            assert torch.equal(alone[0], full[b, :alone.shape[1]]), (kind, b)
            assert (full[b, alone.shape[1]:] == 0).all()


def test_device_pair_offsets_are_checked():
    """Offsets that point outside the packed device buffer never reach the kernel."""
    fe = frontend(44100)
    packed = torch.zeros(64, device=DEV)
    for off in ([0, 65], [-1, 10], [0, 20, 10], [5]):
        with pytest.raises(ValueError):
            fe((packed, off))
    audio, lens = fe((packed, [0, 64]))
    assert lens.tolist() == [out_len(64, 44100)] and (audio == 0).all()


def test_int16_source():
    w = waves("i16")
    assert min(int(a.min()) for a in w if a.size) == -32768 and max(int(a.max()) for a in w if a.size) == 32767
    check_against_yardstick(44100, "i16")


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_padding_is_written_as_zero(kind):
    """The operator-level call on a NaN-filled buffer wider than the batch: every column of the first `ncols` at or beyond an
    utterance's length is exactly 0.0, the zero-length row is all zeros, the columns beyond `ncols` are not touched."""
    from aptai_amd import ops
    fe = frontend(44100)
    w = waves(kind)
    off = np.zeros(len(LENS) + 1, dtype=np.int64)
    off[1:] = np.cumsum(LENS)
    packed = torch.from_numpy(np.concatenate(w)).to(DEV)
    lens = [out_len(n, 44100) for n in LENS]
    ncols, ld = max(lens) + 1037, max(lens) + 1037 + 5
    out = torch.full((len(LENS), ld), float("nan"), device=DEV)
    taps, first = fe._device_tables(out.device)
    ops.resample_batch(packed, torch.from_numpy(off).to(DEV), len(LENS), taps, first, fe.orig, fe.new, fe.Kc, fe.width, out, ncols)
    got = out.cpu()
    full = device_result(44100, kind)[0].cpu()
    for b, n in enumerate(lens):
        assert not torch.isnan(got[b, :ncols]).any()
        assert (got[b, n:ncols] == 0).all() and not torch.signbit(got[b, n:ncols]).any()
        assert torch.equal(got[b, :n], full[b, :n])
        assert torch.isnan(got[b, ncols:]).all()
    assert (got[2, :ncols] == 0).all()
    assert (full[2] == 0).all() and all((full[b, n:] == 0).all() for b, n in enumerate(lens))


@pytest.mark.parametrize("rate,kind", [(44100, "f32"), (44100, "i16"), (16001, "f32")])
def test_isolation(rate, kind):
    """Nothing leaks between neighbours in the packed buffer: each row equals the same utterance resampled alone."""
    full = device_result(rate, kind)[0]
    for b, w in enumerate(waves(kind)):
        alone, n = frontend(rate)([w])
        assert int(n[0]) == out_len(len(w), rate) and alone.shape[1] == int(n[0])
        assert torch.equal(alone[0], full[b, :alone.shape[1]]), (rate, kind, b)


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_window(kind):
    starts, n = [0, 3, 0, 1000, 7999], 1600
    full, full_lens = device_result(44100, kind)
    assert int(full_lens[4]) == 8000
    win, lens = frontend(44100)(list(waves(kind)), window=(starts, n))
    assert tuple(win.shape) == (len(LENS), n)
    want = [max(0, min(n, int(fl) - s)) for fl, s in zip(full_lens.tolist(), starts)]
    assert lens.tolist() == want == [1, 12, 0, 601, 1]
    padded = torch.nn.functional.pad(full, (0, n))
    for b, s in enumerate(starts):
        assert torch.equal(win[b], padded[b, s:s + n]), b
        assert (win[b, want[b]:] == 0).all()
    # a wider padded crop is the same crop
    win2, _ = frontend(44100)(list(waves(kind)), window=(starts, n), pad_to=n + 64)
    assert torch.equal(win2[:, :n], win) and (win2[:, n:] == 0).all()


def test_determinism_and_identity():
    for rate, kind in ((44100, "f32"), (44100, "i16"), (16001, "f32")):
        again, _ = frontend(rate)(list(waves(kind)))
        assert torch.equal(again.view(torch.int32), device_result(rate, kind)[0].view(torch.int32))
    for kind in ("f32", "i16"):
        w = [a.copy() for a in waves(kind)]
        if kind == "f32":
            w[1][:2] = [-0.0, 0.0]                       # bit for bit: the sign of a zero survives
        audio, lens = frontend(16000)(w)
        assert lens.tolist() == LENS and tuple(audio.shape) == (len(LENS), max(LENS))
        for b, a in enumerate(w):
            want = torch.from_numpy(a).float() / 32768.0 if kind == "i16" else torch.from_numpy(a)
            assert torch.equal(audio[b, :len(a)].cpu().view(torch.int32), want.view(torch.int32)), (kind, b)
            assert (audio[b, len(a):] == 0).all()


def hf_normalize64(x, n):
    """zero_mean_unit_var_norm of the HF feature extractor, numpy fp64, over the first n samples; the padding stays 0."""
    y = np.zeros_like(x, dtype=np.float64)
    if n:
        v = x[:n].astype(np.float64)
        y[:n] = (v - v.mean()) / np.sqrt(v.var() + 1e-7)
    return y


def check_normalized(got, base, lens):
    got64 = got.cpu().numpy().astype(np.float64)
    base = base.cpu().numpy()
    assert not np.isnan(got64).any()
    for b, n in enumerate(lens):
        y64 = hf_normalize64(base[b], n)
        err = np.abs(got64[b] - y64)
        tol = 2.0 ** -22 * np.maximum(1.0, np.abs(y64))
        print(f"normalise row {b} (n={n}): max error {err.max() if err.size else 0:.3e}")
        assert (err <= tol).all(), (b, float((err / tol).max()))
        assert (got64[b, n:] == 0).all()


def test_normalize():
    """2^-22 max(1, |y64|): one rounding of an fp64-computed value to fp32 (2^-24 relative) plus headroom; fp32 statistics on the
    row with mean = 50 standard deviations would miss it."""
    # (a) the resampled batch
    base, lens = device_result(44100, "f32")
    got, lens_n = device_result(44100, "f32", True)
    assert lens_n.tolist() == lens.tolist()
    check_normalized(got, base, lens.tolist())
    again, _ = frontend(44100, True)(list(waves("f32")))
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    # (b) identity ratio: mean 50 x standard deviation, a constant utterance, one sample, none, and one of several chunks
    g = np.random.RandomState(5)
    w = [(50.0 + g.randn(5000)).astype(np.float32), np.full(300, 0.7, dtype=np.float32), g.randn(1).astype(np.float32),
         np.zeros(0, dtype=np.float32), (3.0 * g.randn(20001) - 1.0).astype(np.float32)]
    assert 45 < w[0].mean() / w[0].std() < 55
    base, lens = frontend(16000)(w)
    got, _ = frontend(16000, True)(w)
    n = [len(a) for a in w]
    assert lens.tolist() == n
    check_normalized(got, base, n)
    assert (got[1] == 0).all() and (got[2] == 0).all() and (got[3] == 0).all()
    again, _ = frontend(16000, True)(w)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    # (c) the same rows at a pitch of a multiple of four elements (20004): the 16-byte path, where (b) took the scalar one
    from aptai_amd import ops
    S = base.shape[1]
    assert S % 4 == 1
    wide = torch.zeros((len(w), S + 3), device=DEV)
    wide[:, :S] = base
    ops.wave_normalize(wide, lens, S)
    check_normalized(wide[:, :S], base, n)
    assert (wide[:, S:] == 0).all() and (wide[1] == 0).all()


# ------------------------------------------------------------------------------------------------ the training loops
def _record(model, length_key):
    seen = {"lengths": [], "loss": []}
    model.register_forward_pre_hook(lambda m, a, kw: seen["lengths"].append(kw[length_key].cpu().tolist()), with_kwargs=True)
    model.register_forward_hook(lambda m, a, out: seen["loss"].append(float(out["loss"].detach())))
    return seen


def _w2v(tmp_path, **kw):
    from aptai_amd.config import W2V2Config
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    w2v = W2V2Config.base(num_hidden_layers=2, layerdrop=0.0, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., apply_spec_augment=False, **kw)
    torch.manual_seed(0)
    d = tmp_path / "w2v"
    Wav2Vec2Model(w2v).save_pretrained(str(d))
    return w2v, str(d)


def test_loop_phoneme_recognizer(tmp_path):
    import random
    from aptai_amd import hostlogic, train_phoneme_recognizer as T
    vocab = T.default_vocab()
    w2v, d = _w2v(tmp_path)

    def run(source_rate):
        cfg = T.default_cfg(num_epochs=1, batch_size=2, samples_per_epoch=4, learning_rate=2e-5, final_dropout=0.0, huggingface_model_id=d,
                            pretrain_cfg=w2v, num_warmup_epochs=2, source_rate=source_rate)
        torch.manual_seed(3)
        model, opt, sched = T.load_model_optimizer(cfg, vocab)
        seen = _record(model, "input_lengths")
        coll = hostlogic.collate_pr_raw if source_rate else hostlogic.collate_pr
        ds = T.SyntheticCommonPhone(4, 1.0, len(vocab), seed=1, source_rate=source_rate)
        tr = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, collate_fn=coll)
        va = torch.utils.data.DataLoader(T.SyntheticCommonPhone(1, 1.0, len(vocab), seed=2, source_rate=source_rate), batch_size=1,
                                         collate_fn=coll)
        random.seed(7)
        sub = tmp_path / f"run{source_rate}"
        hist = T.train(cfg, model, opt, sched, vocab, tr, va, sub / "best", sub / "last", sub / "all", log=lambda s: None)
        return ds, seen, hist

    ds, seen, hist = run(48000)
    assert len(hist) == 1 and hist[0]["trained_batches"] == 2
    assert all(np.isfinite(v) for v in seen["loss"]) and np.isfinite(hist[0]["mean_train_loss"]) and np.isfinite(hist[0]["mean_val_loss"])
    raw = [ds[i]["audio_len"] for i in range(4)]
    assert any(n % 3 for n in raw)
    assert seen["lengths"][:2] == [[-(-n // 3) for n in raw[:2]], [-(-n // 3) for n in raw[2:]]]
    # flags unset: the loop's first step is the plain collate's batch through the model, as before
    ds, seen, hist = run(None)
    cfg = T.default_cfg(num_epochs=1, batch_size=2, samples_per_epoch=4, learning_rate=2e-5, final_dropout=0.0, huggingface_model_id=d,
                        pretrain_cfg=w2v, num_warmup_epochs=2)
    torch.manual_seed(3)
    model, _, _ = T.load_model_optimizer(cfg, vocab)
    model.train()
    batch = hostlogic.collate_pr([ds[0], ds[1]])
    direct = float(model(**{k: v.to(DEV) for k, v in batch.items()})["loss"].detach())
    assert seen["lengths"][0] == batch["input_lengths"].tolist()
    assert seen["loss"][0] == direct, (seen["loss"][0], direct)


def test_loop_aptai(tmp_path):
    from aptai_amd import hostlogic, train_aptai as T
    w2v, d = _w2v(tmp_path, vocab_size=T.VOCAB_SIZE)

    def run(source_rate):
        cfg = T.default_cfg(num_epochs=1, batch_size=2, learning_rate=2e-5, huggingface_model_id=d, pretrain_cfg=w2v, num_warmup_epochs=2,
                            source_rate=source_rate)
        torch.manual_seed(3)
        model, opt, sched = T.load_model_optimizer(cfg)
        seen = _record(model, "audio_lengths")
        coll = hostlogic.collate_aptai_raw if source_rate else hostlogic.collate_aptai
        ds = T.SyntheticHPRC(4, 1.0, seed=1, cfg=w2v, source_rate=source_rate)
        tr = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, collate_fn=coll)
        va = torch.utils.data.DataLoader(T.SyntheticHPRC(1, 1.0, seed=2, cfg=w2v, source_rate=source_rate), batch_size=1, collate_fn=coll)
        hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / f"best{source_rate}", log=lambda s: None)
        return ds, seen, hist

    ds, seen, hist = run(48000)
    assert len(hist) == 1 and all(np.isfinite(v) for v in seen["loss"]) and len(seen["loss"]) == 3          # two steps + one validation file
    assert all(np.isfinite(v) for v in hist[0].values() if isinstance(v, float)), hist
    raw = [ds[i]["audio_len"] for i in range(4)]
    assert any(n % 3 for n in raw)
    assert seen["lengths"][:2] == [[-(-n // 3) for n in raw[:2]], [-(-n // 3) for n in raw[2:]]]
    ds, seen, hist = run(None)
    cfg = T.default_cfg(num_epochs=1, batch_size=2, learning_rate=2e-5, huggingface_model_id=d, pretrain_cfg=w2v, num_warmup_epochs=2)
    torch.manual_seed(3)
    model, _, _ = T.load_model_optimizer(cfg)
    model.train()
    batch = hostlogic.collate_aptai([ds[0], ds[1]])
    direct = float(model(0, **{k: v.to(DEV) for k, v in batch.items()})["loss"].detach())
    assert seen["lengths"][0] == batch["audio_lengths"].tolist()
    assert seen["loss"][0] == direct, (seen["loss"][0], direct)
