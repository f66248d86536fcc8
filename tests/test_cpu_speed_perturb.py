"""CPU: the host side of speed perturbation (aptai_amd.frontend with `speeds=`, csrc/frontend.hip): the two entry points are
declared, exported and typed; `speed_rate` and the speed-aware output lengths against integer arithmetic; the host oracles of
aptai_warp_targets (`warp_track` on `interpolate_signal`, `warp_frame_labels`); the loops' opt-in; argument errors.  The device
side is tests/test_gpu_speed_perturb.py."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from aptai_amd import hostlogic

NEW = ("aptai_resample_batch_multi", "aptai_warp_targets")
SPEEDS = (0.9, 1.0, 1.1)


def test_new_entry_points_are_declared_exported_and_typed():
    from aptai_amd import _lib, frontend, loops, ops
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in NEW:
        assert n in names and n in _lib.ARGTYPES and hasattr(L, n), n
        assert getattr(L, n).argtypes == _lib.ARGTYPES[n]
    for w in ("resample_batch_multi", "warp_targets"):
        assert callable(getattr(ops, w))
    for f in ("speed_rate", "warp_track", "warp_frame_labels"):
        assert callable(getattr(hostlogic, f))
    assert ops.RESAMPLE_MAX_RATIOS == 8
    assert callable(frontend.DeviceFrontend(16000, speeds=SPEEDS).draw_speeds) and callable(loops.uses_frontend)


def test_ops_refuse_cpu_tensors():
    from aptai_amd import ops
    from aptai_amd._lib import AptaiHipError
    table = np.array([[1, 1, 1, 0, 0, 0, 0, 0]], dtype=np.int32)
    with pytest.raises(AptaiHipError):
        ops.resample_batch_multi(torch.zeros(32), torch.tensor([0, 16, 32]), 2, None, None, torch.from_numpy(table), table,
                                 torch.zeros(2, dtype=torch.int32), np.zeros(2, dtype=np.int32), torch.zeros(2, 16), 16)
    with pytest.raises(AptaiHipError):
        ops.warp_targets(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.int64), torch.full((4,), 8), torch.full((4,), 9), 9)


def test_speed_rate_and_reduced_ratios():
    assert hostlogic.speed_rate(16000, 0.9) == 14400 and hostlogic.speed_rate(16000, 1.1) == 17600
    assert hostlogic.speed_rate(48000, 0.9) == 43200 and hostlogic.speed_rate(44100, 1.1) == 48510
    assert hostlogic.speed_rate(16000, 1.0) == 16000
    for rate in (16000, 44100, 48000, 22050):
        for f in (0.5, 0.9, 0.95, 1.0, 1.05, 1.1, 2.0):
            assert hostlogic.speed_rate(rate, f) == int(round(rate * f))
    from aptai_amd.frontend import DeviceFrontend
    got = {rate: [tuple(int(v) for v in row[:2]) for row in DeviceFrontend(rate, speeds=SPEEDS)._table] for rate in (16000, 48000)}
    assert got[16000] == [(9, 10), (1, 1), (11, 10)]
    assert got[48000] == [(27, 10), (3, 1), (33, 10)]


@pytest.mark.parametrize("rate", [16000, 48000, 44100])
def test_speed_aware_out_lengths(rate):
    from aptai_amd.frontend import DeviceFrontend
    fe = DeviceFrontend(rate, speeds=SPEEDS)
    plain = DeviceFrontend(rate)
    lens = np.array([0, 1, 2, 9, 10, 11, 40, 4411, 22050, 160000, 159999], dtype=np.int64)
    for r, f in enumerate(SPEEDS):
        src = hostlogic.speed_rate(rate, f)
        ratio = Fraction(16000, src)
        want = [math.ceil(ratio * int(n)) for n in lens]                        # exact rational arithmetic
        got = fe.out_lengths(lens, np.full(lens.size, r))
        assert got.dtype == np.int64 and got.tolist() == want
        assert got.tolist() == DeviceFrontend(src).out_lengths(lens).tolist()
    # rows with their own indices; no index = factor 1.0 = the plain front end
    idx = np.arange(lens.size) % 3
    mixed = fe.out_lengths(lens, idx)
    assert mixed.tolist() == [int(fe.out_lengths([n], [i])[0]) for n, i in zip(lens, idx)]
    assert fe.out_lengths(lens).tolist() == plain.out_lengths(lens).tolist() == fe.out_lengths(lens, np.full(lens.size, 1)).tolist()


def test_draw_speeds_is_seeded_and_uniform_over_the_indices():
    from aptai_amd.frontend import DeviceFrontend
    a, b, c = (DeviceFrontend(16000, speeds=SPEEDS, seed=s) for s in (5, 5, 6))
    da, db, dc = a.draw_speeds(64), b.draw_speeds(64), c.draw_speeds(64)
    assert da.dtype == np.int32 and da.shape == (64,) and set(da.tolist()) == {0, 1, 2}
    assert da.tolist() == db.tolist() == np.random.RandomState(5).randint(0, 3, size=64).tolist() and da.tolist() != dc.tolist()
    assert a.draw_speeds(64).tolist() == b.draw_speeds(64).tolist() != da.tolist()          # the stream goes on


def _rows(seed=0):
    g = np.random.RandomState(seed)
    return [(g.randn(n_in), n_in, n_out) for n_in in (2, 3, 49, 50, 499) for n_out in (1, 2, n_in - 1, n_in + 1, int(n_in / 0.9), int(n_in / 1.1) + 1)
            if n_out >= 1 and n_out != n_in]


def test_warp_track_is_interpolate_signal_without_holes():
    for x, n_in, n_out in _rows():
        got = hostlogic.warp_track(np.concatenate([x, [7.0, -100.0]]), n_in, n_out)          # what lies beyond n_in is not read
        want = hostlogic.interpolate_signal(x, n_out)
        assert got.dtype == np.float64 and got.shape == (n_out,)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (n_in, n_out)
        if n_out > 1:
            assert got[0] == x[0] and abs(got[-1] - x[-1]) <= 4 * np.finfo(np.float64).eps * np.abs(x[-2:]).max()


def test_warp_identity_and_degenerate_rows():
    g = np.random.RandomState(1)
    x = g.randn(49)
    x[[0, 7, 48]] = [-0.0, -100.0, -100.0]
    same = hostlogic.warp_track(x, 49, 49)
    assert np.array_equal(same.view(np.int64), x.view(np.int64)) and same is not x          # verbatim: the sign of a zero, the holes
    lab = g.randint(1, 40, size=49)
    assert np.array_equal(hostlogic.warp_frame_labels(lab, 49, 49), lab)
    # one frame in: every output is that frame; one frame out: the first frame
    assert hostlogic.warp_track([2.5, 9.0], 1, 4).tolist() == [2.5] * 4 and hostlogic.warp_frame_labels([3, 9], 1, 4).tolist() == [3] * 4
    assert hostlogic.warp_track(x[1:], 48, 1).tolist() == [x[1]] and hostlogic.warp_frame_labels(lab, 49, 1).tolist() == [lab[0]]
    assert hostlogic.warp_track([-100.0], 1, 3).tolist() == [-100.0] * 3
    # nothing in: padding out
    assert hostlogic.warp_track(x, 0, 5).tolist() == [-100.0] * 5 and hostlogic.warp_track(x, 0, 0).shape == (0,)
    assert hostlogic.warp_frame_labels(lab, 0, 5).tolist() == [0] * 5


def test_ignore_value_propagates():
    x = np.arange(10, dtype=np.float64)
    x[4] = -100.0
    n_out = 19                                                                    # p_i = i / 2: even i sit on a frame, odd i between two
    y = hostlogic.warp_track(x, 10, n_out)
    pos = np.linspace(0, 9, n_out)
    assert np.array_equal(pos, np.arange(n_out) / 2)
    for i, p in enumerate(pos):
        lo = min(int(math.floor(p)), 8)
        w = p - lo
        touched = x[lo] == -100.0 or (w > 0 and x[lo + 1] == -100.0)
        assert (y[i] == -100.0) == touched, i
        if not touched:
            assert y[i] == p                                                      # a ramp stays a ramp
    assert [i for i in range(n_out) if y[i] == -100.0] == [7, 8, 9]
    # a hole in the last frame reaches the last output only (w == 1 there), not the frame before it
    x = np.arange(10, dtype=np.float64)
    x[9] = -100.0
    y = hostlogic.warp_track(x, 10, 10 + 9)
    assert y[16] == 8.0 and y[17] == -100.0 and y[18] == -100.0
    assert hostlogic.warp_track(x, 10, 5, ignore=-1.0)[-1] == hostlogic.interpolate_signal(x, 5)[-1]


def test_warp_frame_labels_monotone_with_endpoints():
    g = np.random.RandomState(2)
    for n_in in (2, 3, 49, 499):
        lab = np.arange(n_in) * 3 + 1                                             # strictly increasing: the chosen index is visible
        for n_out in (2, n_in - 1, n_in + 1, int(n_in / 0.9), int(n_in / 1.1) + 1, 3 * n_in):
            if n_out < 2:
                continue
            out = hostlogic.warp_frame_labels(lab, n_in, n_out)
            assert out.shape == (n_out,) and out.dtype == lab.dtype
            assert out[0] == lab[0] and out[-1] == lab[-1] and (np.diff(out) >= 0).all()
            k = (out - 1) // 3
            assert np.abs(k - np.arange(n_out) * (n_in - 1) / (n_out - 1)).max() <= 0.5 + 1e-9
            if n_out >= n_in:
                assert set(out.tolist()) == set(lab.tolist())                     # stretching loses no label
    runs = np.repeat(g.randint(1, 40, size=13), 4)[:49]
    out = hostlogic.warp_frame_labels(runs, 49, 54)
    collapse = lambda a: [int(v) for i, v in enumerate(a) if i == 0 or v != a[i - 1]]
    assert collapse(out) == collapse(runs)


def test_loops_opt_in_is_unchanged_without_speeds():
    from aptai_amd import loops, train_aptai
    from aptai_amd.frontend import DeviceFrontend, make_frontend, parse_speeds
    cfg = train_aptai.default_cfg()
    assert cfg.speed_perturb is None and cfg.speed_perturb_seed == 0
    assert make_frontend(cfg) is None and not loops.uses_frontend(cfg)
    for kw, rate, norm in ((dict(source_rate=48000), 48000, False), (dict(normalize_audio=True), 16000, True),
                           (dict(source_rate=44100, normalize_audio=True), 44100, True)):
        fe = make_frontend(train_aptai.default_cfg(**kw))
        assert loops.uses_frontend(SimpleNamespace(source_rate=kw.get("source_rate"), normalize_audio=kw.get("normalize_audio", False),
                                                   speed_perturb=None))
        assert isinstance(fe, DeviceFrontend) and fe.speeds is None and (fe.orig_freq, fe.normalize) == (rate, norm)
    assert not loops.uses_frontend(SimpleNamespace(source_rate=None, normalize_audio=False, speed_perturb=None))
    assert not loops.uses_frontend(SimpleNamespace(source_rate=None, normalize_audio=False))
    # set: on its own, and together with the other two
    assert parse_speeds("0.9,1.0,1.1") == SPEEDS and parse_speeds(None) is None and parse_speeds("") is None and parse_speeds([0.9]) == (0.9,)
    fe = make_frontend(train_aptai.default_cfg(speed_perturb=SPEEDS, speed_perturb_seed=4), rank=2)
    assert fe.speeds == SPEEDS and fe.orig_freq == 16000 and not fe.normalize
    assert fe.draw_speeds(8).tolist() == np.random.RandomState(6).randint(0, 3, size=8).tolist()
    fe = make_frontend(train_aptai.default_cfg(speed_perturb="0.9,1.1", source_rate=48000, normalize_audio=True))
    assert fe.speeds == (0.9, 1.1) and fe.orig_freq == 48000 and fe.normalize
    assert loops.uses_frontend(SimpleNamespace(source_rate=None, normalize_audio=False, speed_perturb="0.9,1.1"))
    # the command line
    import argparse
    ap = argparse.ArgumentParser()
    loops.add_shared_arguments(ap)
    shared = loops.shared_arguments(ap.parse_args(["--speed_perturb", "0.9,1.0,1.1", "--speed_perturb_seed", "3"]))
    assert shared["speed_perturb"] == SPEEDS and shared["speed_perturb_seed"] == 3
    shared = loops.shared_arguments(ap.parse_args([]))
    assert shared["speed_perturb"] is None and shared["speed_perturb_seed"] == 0


def test_to_device_without_a_front_end_ignores_augment():
    from aptai_amd import loops
    batch = {"a": torch.arange(3)}
    out = loops.to_device(batch, "cpu", None, "x", "n", augment=True)
    assert set(out) == {"a"} and torch.equal(out["a"], batch["a"])


def test_argument_validation():
    from aptai_amd.frontend import DeviceFrontend
    with pytest.raises(ValueError, match="speeds"):
        DeviceFrontend(16000, speeds=(0.9, 0.92, 0.94, 0.96, 0.98, 1.0, 1.02, 1.04, 1.06))          # nine
    with pytest.raises(ValueError, match="speeds"):
        DeviceFrontend(16000, speeds=())
    for bad in (0.49, 2.01, float("nan")):
        with pytest.raises(ValueError, match=r"\[0.5, 2.0\]"):
            DeviceFrontend(16000, speeds=(1.0, bad))
    with pytest.raises(ValueError, match="table"):
        DeviceFrontend(400001, 400000, speeds=(1.0,))                            # the base bank is checked as before
    with pytest.raises(ValueError, match="table"):
        DeviceFrontend(200000, 400000, speeds=(1.0, 1.000005))                   # 1:2 is fine; 200001 -> 400000 is 400000 x 13 taps
    assert len(DeviceFrontend(16000, speeds=(0.5, 0.8, 0.9, 0.95, 1.0, 1.05, 1.1, 2.0)).speeds) == 8
    fe = DeviceFrontend(16000, speeds=SPEEDS)
    waves = [np.zeros(300, dtype=np.float32), np.zeros(30, dtype=np.float32)]
    for bad in ([0], [0, 1, 2], [0, 3], [-1, 0], [0.5, 1.0]):
        with pytest.raises(ValueError, match="speed_index"):
            fe.out_lengths([300, 30], bad)
        with pytest.raises(ValueError, match="speed_index"):
            fe(waves, speed_index=bad)                                            # refused before anything is uploaded
    plain = DeviceFrontend(16000)
    with pytest.raises(ValueError, match="speeds"):
        plain(waves, speed_index=[0, 0])
    with pytest.raises(ValueError, match="speeds"):
        plain.draw_speeds(2)
