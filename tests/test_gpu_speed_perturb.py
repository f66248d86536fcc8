"""GPU: speed perturbation on the device front end (aptai_amd.frontend with `speeds=`; aptai_resample_batch_multi and
aptai_warp_targets in csrc/frontend.hip).

Resampling: the batch of tests/test_gpu_frontend.py (1, 40, 0, 4411 and 22050 samples, float32 and int16) at speeds
(0.9, 1.0, 1.1) with the indices [2, 0, 1, 2, 0], from three source rates:

    16000   9:10 and 11:10, and 1:1 (the copy path) in one launch
    48000   27:10, 3:1, 33:10
    44100   3969:1600 and 4851:1600 (1600 rows: beyond the `first` entries held in LDS, read through L2) beside 441:160 (staged)

The reference of every row is the single-ratio launch of that utterance alone at `speed_rate(rate, f)`, which
tests/test_gpu_frontend.py pins: the rows have to be its bits.  The longest row (22050 samples at 0.9) is 24500 / 8167 / 8889
samples, 24 / 8 / 9 tiles of 1024 with a partial last one.  The fp64 yardstick and its bound are those of
tests/test_cpu_frontend.py, |y - y64| <= (Kc + 2) 2^-24 A max|x|, with the row's own Kc.

Targets: aptai_warp_targets against hostlogic.warp_track / warp_frame_labels, tracks compared as bits.  Every device result is
computed once per module and shared."""
import functools

import numpy as np
import pytest
import torch

from test_cpu_frontend import direct_resample
from test_gpu_frontend import LENS, _w2v, as_float64, waves

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPEEDS = (0.9, 1.0, 1.1)
IDX = [2, 0, 1, 2, 0]
RATES = (16000, 48000, 44100)
CASES = [(r, k) for r in RATES for k in ("f32", "i16")]


@functools.lru_cache(maxsize=None)
def frontend(rate, normalize=False):
    from aptai_amd.frontend import DeviceFrontend
    return DeviceFrontend(rate, 16000, normalize=normalize, speeds=SPEEDS)


@functools.lru_cache(maxsize=None)
def single(source_rate, normalize=False):
    from aptai_amd.frontend import DeviceFrontend
    return DeviceFrontend(source_rate, 16000, normalize=normalize)


@functools.lru_cache(maxsize=None)
def device_result(rate, kind):
    audio, lens = frontend(rate)(list(waves(kind)), speed_index=IDX)
    torch.cuda.synchronize()
    return audio, lens


def source_rate(rate, b):
    from aptai_amd import hostlogic
    return hostlogic.speed_rate(rate, SPEEDS[IDX[b]])


def want_lengths(rate):
    return [-((-16000 * n) // source_rate(rate, b)) for b, n in enumerate(LENS)]          # ceil(16000 n / source rate)


def test_the_cases_are_what_the_docstring_says():
    assert [tuple(int(v) for v in row[:2]) for row in frontend(16000)._table] == [(9, 10), (1, 1), (11, 10)]
    assert [tuple(int(v) for v in row[:2]) for row in frontend(48000)._table] == [(27, 10), (3, 1), (33, 10)]
    t = frontend(44100)._table
    assert [tuple(int(v) for v in row[:2]) for row in t] == [(3969, 1600), (441, 160), (4851, 1600)]
    assert t[0, 1] > 1024 and t[2, 1] > 1024 and t[1, 1] * t[1, 2] + t[1, 1] <= 8704          # RS_FIRST, RS_TAPS of csrc/frontend.hip
    assert [want_lengths(r)[4] for r in RATES] == [24500, 8167, 8889] and all(want_lengths(r)[4] % 1024 for r in RATES)


@pytest.mark.parametrize("rate,kind", CASES)
def test_rows_are_the_single_ratio_bits(rate, kind):
    audio, lens = device_result(rate, kind)
    want = want_lengths(rate)
    assert lens.dtype == torch.int64 and lens.is_cuda and lens.tolist() == want == frontend(rate).out_lengths(LENS, IDX).tolist()
    assert audio.dtype == torch.float32 and tuple(audio.shape) == (len(LENS), max(want))
    for b, w in enumerate(waves(kind)):
        alone, n = single(source_rate(rate, b))([w])
        assert int(n[0]) == want[b] and alone.shape[1] == want[b]
        assert torch.equal(alone[0].view(torch.int32), audio[b, :want[b]].view(torch.int32)), (rate, kind, b)
        pad = audio[b, want[b]:]
        assert (pad == 0).all() and not torch.signbit(pad).any()


@pytest.mark.parametrize("rate,kind", CASES)
def test_rows_against_the_fp64_yardstick(rate, kind):
    audio, _ = device_result(rate, kind)
    got = audio.cpu().numpy().astype(np.float64)
    want = want_lengths(rate)
    for b, w in enumerate(waves(kind)):
        x = as_float64(w)
        if len(x) == 0:
            continue
        if source_rate(rate, b) == 16000:                      # the copy path is the identity, as for a front end at 16 kHz
            assert np.array_equal(got[b, :want[b]], x)
            continue
        y64, A = direct_resample(x, source_rate(rate, b))
        assert y64.shape[0] == want[b]
        Kc = int(frontend(rate)._table[IDX[b], 2])
        assert Kc == single(source_rate(rate, b)).Kc
        bound = (Kc + 2) * 2.0 ** -24 * A * np.abs(x).max()
        err = np.abs(got[b, :want[b]] - y64).max()
        print(f"rate {rate} x {SPEEDS[IDX[b]]} {kind} utterance {b}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (rate, b, err, bound)


@pytest.mark.parametrize("rate,kind", [(16000, "f32"), (44100, "i16")])
def test_window_is_a_slice(rate, kind):
    starts, n = [0, 3, 0, 1000, 7999], 1600
    full, full_lens = device_result(rate, kind)
    win, lens = frontend(rate)(list(waves(kind)), window=(starts, n), speed_index=IDX)
    assert tuple(win.shape) == (len(LENS), n)
    want = [max(0, min(n, int(fl) - s)) for fl, s in zip(full_lens.tolist(), starts)]
    assert lens.tolist() == want and want[4] == min(n, want_lengths(rate)[4] - 7999) and want[3] > 0
    padded = torch.nn.functional.pad(full, (0, n))
    for b, s in enumerate(starts):
        assert torch.equal(win[b].view(torch.int32), padded[b, s:s + n].view(torch.int32)), b
        assert (win[b, want[b]:] == 0).all()
    win2, _ = frontend(rate)(list(waves(kind)), window=(starts, n), pad_to=n + 64, speed_index=IDX)
    assert torch.equal(win2[:, :n], win) and (win2[:, n:] == 0).all()


@pytest.mark.parametrize("rate,kind", [(16000, "f32"), (48000, "i16"), (44100, "f32")])
def test_factor_one_is_the_plain_front_end(rate, kind):
    plain, plain_lens = single(rate)(list(waves(kind)))
    for speed_index in ([1] * len(LENS), None):
        got, lens = frontend(rate)(list(waves(kind)), speed_index=speed_index)
        assert lens.tolist() == plain_lens.tolist()
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), (rate, kind, speed_index)


@pytest.mark.parametrize("rate,kind", [(48000, "f32"), (44100, "i16")])
def test_two_runs_are_the_same_bits(rate, kind):
    again, lens = frontend(rate)(list(waves(kind)), speed_index=IDX)
    first, first_lens = device_result(rate, kind)
    assert lens.tolist() == first_lens.tolist() and torch.equal(again.view(torch.int32), first.view(torch.int32))


def test_normalize_and_pad_to_compose():
    from aptai_amd import ops
    base, lens = device_result(48000, "f32")
    S = base.shape[1]
    got, lens_n = frontend(48000, True)(list(waves("f32")), speed_index=IDX, pad_to=S + 40)
    assert lens_n.tolist() == lens.tolist() and tuple(got.shape) == (len(LENS), S + 40) and (got[:, S:] == 0).all()
    want = torch.nn.functional.pad(base, (0, 40))
    ops.wave_normalize(want, lens, S + 40)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError, match="pad_to"):
        frontend(48000)(list(waves("f32")), speed_index=IDX, pad_to=S - 1)


def test_library_refuses_a_bad_table():
    """The entry point's own checks on the host copies: an index outside the table, a bank outside the concatenated arrays."""
    from aptai_amd import ops
    from aptai_amd._lib import AptaiHipError
    fe = frontend(16000)
    taps, first, table = fe._device_speed_tables(torch.device(DEV, torch.cuda.current_device()))
    packed = torch.zeros(64, device=DEV)
    off = torch.tensor([0, 32, 64], device=DEV)
    out = torch.full((2, 40), float("nan"), device=DEV)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(AptaiHipError, match="ratio index"):
        ops.resample_batch_multi(packed, off, 2, taps, first, table, fe._table, idx, np.array([0, 3], dtype=np.int32), out, 40)
    bad = fe._table.copy()
    bad[2, 4] = taps.numel()
    with pytest.raises(AptaiHipError, match="outside"):
        ops.resample_batch_multi(packed, off, 2, taps, first, table, bad, idx, np.zeros(2, dtype=np.int32), out, 40)
    assert torch.isnan(out).all()                               # nothing was launched
    ops.resample_batch_multi(packed, off, 2, taps, first, table, fe._table, idx, np.zeros(2, dtype=np.int32), out, 40)
    assert (out == 0).all()


# ------------------------------------------------------------------------------------------------ aptai_warp_targets
N_IN = [0, 1, 49, 499]
T_IN, N_TV = 503, 9


@functools.lru_cache(maxsize=None)
def targets():
    """(tracks fp64 [9][4][T_IN] with -100 holes and -100 padding, labels int64 [4][T_IN] with 0 padding), numpy."""
    g = np.random.RandomState(77)
    trk = g.randn(N_TV, len(N_IN), T_IN)
    lab = g.randint(1, 46, size=(len(N_IN), T_IN)).astype(np.int64)
    trk[g.rand(*trk.shape) < 0.04] = -100.0
    trk[0, 2, [0, 48]] = -100.0
    trk[1, 3, 498] = -100.0
    trk[2, 1, 0] = -100.0
    trk[3, 2, 5] = -0.0
    for b, n in enumerate(N_IN):
        trk[:, b, n:] = -100.0
        lab[b, n:] = 0
    return trk, lab


def warp_on_device(n_out, T_out):
    from aptai_amd import ops
    trk, lab = targets()
    B = len(N_IN)
    rows = N_TV + 1
    n_in_d = torch.tensor(N_IN * rows, device=DEV)
    n_out_d = torch.tensor(list(n_out) * rows, device=DEV)
    t, l = ops.warp_targets(torch.from_numpy(trk).to(DEV).reshape(N_TV * B, T_IN), torch.from_numpy(lab).to(DEV), n_in_d, n_out_d, T_out)
    torch.cuda.synchronize()
    assert t.dtype == torch.float64 and tuple(t.shape) == (N_TV * B, T_out) and l.dtype == torch.int64 and tuple(l.shape) == (B, T_out)
    return t.cpu().numpy().reshape(N_TV, B, T_out), l.cpu().numpy()


@pytest.mark.parametrize("factor", [0.9, 1.1, 1.0])
def test_warp_targets_against_the_host_oracles(factor):
    """n_out = ceil(n_in / factor): 0, 2, 55, 555 at 0.9 and 0, 1, 45, 454 at 1.1 (so 1 -> 2 frames, and 1 -> 1, a copy); 1.0 is
    the verbatim copy of every row, holes and the sign of a zero included.  Three columns of padding beyond the longest row."""
    from aptai_amd import hostlogic
    n_out = [int(np.ceil(n / factor)) for n in N_IN]
    assert n_out == {0.9: [0, 2, 55, 555], 1.1: [0, 1, 45, 454], 1.0: N_IN}[factor]
    T_out = max(n_out) + 3
    trk, lab = targets()
    got_t, got_l = warp_on_device(tuple(n_out), T_out)
    for b, (ni, no) in enumerate(zip(N_IN, n_out)):
        want_l = np.zeros(T_out, dtype=np.int64)
        want_l[:no] = hostlogic.warp_frame_labels(lab[b], ni, no) if ni else 0
        assert np.array_equal(got_l[b], want_l), (factor, b)
        holes = 0
        for k in range(N_TV):
            want = np.full(T_out, -100.0)
            if ni:
                want[:no] = hostlogic.warp_track(trk[k, b], ni, no)
            holes += int((want[:no] == -100.0).sum()) if ni else 0
            assert np.array_equal(got_t[k, b].view(np.int64), want.view(np.int64)), (factor, k, b)
        if ni >= 49:
            assert 0 < holes < N_TV * no                          # the rows do have holes, and values
    if factor == 1.0:
        assert np.signbit(got_t[3, 2, 5]) and got_t[3, 2, 5] == 0.0
        assert np.array_equal(got_t[:, :, :T_IN - 4].view(np.int64), trk[:, :, :T_IN - 4].view(np.int64))


def test_warp_targets_tracks_or_labels_alone():
    from aptai_amd import ops
    trk, lab = targets()
    n_out = [0, 2, 55, 555]
    both_t, both_l = warp_on_device(tuple(n_out), 558)
    t, none = ops.warp_targets(torch.from_numpy(trk[4]).to(DEV).contiguous(), None, torch.tensor(N_IN, device=DEV), torch.tensor(n_out, device=DEV), 558)
    assert none is None and np.array_equal(t.cpu().numpy().view(np.int64), both_t[4].view(np.int64))
    none, l = ops.warp_targets(None, torch.from_numpy(lab).to(DEV), torch.tensor(N_IN, device=DEV), torch.tensor(n_out, device=DEV), 558)
    assert none is None and np.array_equal(l.cpu().numpy(), both_l)


# ------------------------------------------------------------------------------------------------ end to end
def _aptai(tmp_path, **cfg_kw):
    from aptai_amd import train_aptai as T
    w2v, d = _w2v(tmp_path, vocab_size=T.VOCAB_SIZE)
    cfg = T.default_cfg(num_epochs=1, batch_size=2, learning_rate=2e-5, huggingface_model_id=d, pretrain_cfg=w2v, num_warmup_epochs=2,
                        speed_perturb=SPEEDS, **cfg_kw)
    torch.manual_seed(3)
    return (T, w2v, cfg) + tuple(T.load_model_optimizer(cfg))


def test_end_to_end_batch_into_aptai(tmp_path):
    from aptai_amd import hostlogic
    from aptai_amd.frontend import make_frontend, raw_batch_to_device
    T, w2v, cfg, model, _, _ = _aptai(tmp_path, speed_perturb_seed=5)
    ds = T.SyntheticHPRC(3, 1.0, seed=1, cfg=w2v)
    items = [ds[i] for i in range(3)]
    batch = hostlogic.collate_aptai_raw(items)
    fe = make_frontend(cfg)
    assert fe.speeds == SPEEDS and (fe.conv_kernel, fe.conv_stride) == (tuple(w2v.conv_kernel), tuple(w2v.conv_stride))
    plain = raw_batch_to_device(batch, fe, DEV, "audio_inputs", "audio_lengths")
    assert "_speed_index" not in plain
    out = raw_batch_to_device(batch, fe, DEV, "audio_inputs", "audio_lengths", augment=True, speed_index=[0, 1, 2])
    assert out.pop("_speed_index").tolist() == [0, 1, 2]
    raw = [it["audio_len"] for it in items]
    lens = [-((-16000 * n) // hostlogic.speed_rate(16000, f)) for n, f in zip(raw, SPEEDS)]
    frames = lambda n: int(hostlogic.feat_extract_output_lengths(n, w2v.conv_kernel, w2v.conv_stride))
    n_in, n_out = [frames(n) for n in raw], [frames(n) for n in lens]
    assert out["audio_lengths"].tolist() == lens and out["audio_inputs"].shape[1] == max(lens) and n_out[0] > n_in[0] and n_out[2] < n_in[2]
    host = raw_batch_to_device(batch, fe, DEV, "audio_inputs", "audio_lengths", host_lengths=True, augment=True, speed_index=[0, 1, 2])
    assert not host["audio_lengths"].is_cuda and host["audio_lengths"].tolist() == lens
    assert set(out) == set(plain)
    # targets: every row against the host oracles, dtypes as the collate made them; the row at 1.0 is the unperturbed one
    for k in hostlogic.TV_NAMES + ("phn_frames_49hz",):
        assert out[k].dtype == batch[k].dtype and tuple(out[k].shape) == (3, max(n_out)), k
        got = out[k].cpu().numpy()
        for b in range(3):
            src = batch[k][b].numpy()
            if k == "phn_frames_49hz":
                want = np.zeros(max(n_out), dtype=np.int64)
                want[:n_out[b]] = hostlogic.warp_frame_labels(src, n_in[b], n_out[b])
                assert np.array_equal(got[b], want), (k, b)
            else:
                want = np.full(max(n_out), -100.0)
                want[:n_out[b]] = hostlogic.warp_track(src, n_in[b], n_out[b])
                assert np.array_equal(got[b].view(np.int64), want.view(np.int64)), (k, b)
        assert torch.equal(out[k][1, :n_in[1]], plain[k][1, :n_in[1]])
    assert torch.equal(out["audio_inputs"][1, :lens[1]].view(torch.int32), plain["audio_inputs"][1, :lens[1]].view(torch.int32))
    assert (out["audio_inputs"][1, lens[1]:] == 0).all()
    # into the model
    model.train()
    res = model(0, **out)
    assert res["tvs_pred"].shape[1] == max(n_out)
    res["loss"].backward()
    assert torch.isfinite(res["loss"]).all()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    # the same seed draws the same speeds, and the same batch
    a = raw_batch_to_device(batch, make_frontend(cfg), DEV, "audio_inputs", "audio_lengths", augment=True)
    b = raw_batch_to_device(batch, make_frontend(cfg), DEV, "audio_inputs", "audio_lengths", augment=True)
    assert a["_speed_index"].tolist() == b["_speed_index"].tolist() == np.random.RandomState(5).randint(0, 3, size=3).tolist()
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("graphed", [False, True])
def test_train_loop_sees_the_host_plan(tmp_path, monkeypatch, graphed):
    """One epoch of train_aptai with cfg.speed_perturb: the lengths that reach the model in the two train steps are the host plan
    (the seeded draws, integer arithmetic), eagerly and through the graphed runner; validation is not perturbed."""
    from aptai_amd import graphed as G, hostlogic
    from aptai_amd.frontend import DeviceFrontend
    T, w2v, cfg, model, opt, sched = _aptai(tmp_path, speed_perturb_seed=9, graphed=graphed)
    seen = {"train": [], "all": []}
    model.register_forward_pre_hook(lambda m, a, kw: seen["all"].append(kw["audio_lengths"].cpu().tolist()), with_kwargs=True)
    if graphed:
        step = G.BucketedGraphedStep.step

        def spy(self, batch):
            assert "_speed_index" not in batch and not batch["audio_lengths"].is_cuda
            seen["train"].append(batch["audio_lengths"].tolist())
            return step(self, batch)
        monkeypatch.setattr(G.BucketedGraphedStep, "step", spy)
    ds = T.SyntheticHPRC(4, 1.0, seed=1, cfg=w2v)
    tr = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, collate_fn=hostlogic.collate_aptai_raw)
    val = T.SyntheticHPRC(1, 1.0, seed=2, cfg=w2v)
    va = torch.utils.data.DataLoader(val, batch_size=1, collate_fn=hostlogic.collate_aptai_raw)
    hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lambda s: None)
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values() if isinstance(v, float)), hist
    g = np.random.RandomState(9)
    plan = DeviceFrontend(16000, speeds=SPEEDS)
    raw = [ds[i]["audio_len"] for i in range(4)]
    want = [plan.out_lengths(raw[:2], g.randint(0, 3, size=2)).tolist(), plan.out_lengths(raw[2:], g.randint(0, 3, size=2)).tolist()]
    assert want != [raw[:2], raw[2:]]                             # the seed does perturb
    if graphed:
        # model.forward itself runs once per newly captured shape (the runner's eager first step, on the batch it is captured for)
        assert seen["train"] == want and seen["all"][-1] == [val[0]["audio_len"]] and all(n in want for n in seen["all"][:-1])
    else:
        assert seen["all"] == want + [[val[0]["audio_len"]]]
