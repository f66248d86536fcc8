"""CPU: the window plan and the seam rule of long-form inference (hostlogic.long_form_plan / long_form_ramp / long_form_stitch), the
oracle of aptai_stitch_windows.  Everything here is integer arithmetic or exact fp32: the assertions are equalities.

Blend data lies on a grid of 2^-10 within [-4, 4): x1 - x0 is then exact in fp32, so x0 + ramp (x1 - x0) lies between x0 and x1
before its last rounding and, rounding being monotone and x0, x1 representable, after it too - "between" is asserted without slack.
"""
import numpy as np
import pytest

from aptai_amd import hostlogic

CK, CS = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
SMALL = dict(window_frames=24, hop_frames=16, trim_frames=2)


def _frames(n):
    return hostlogic.conv_layer_lengths(n, CK, CS)[-1]


def _check_plan(p, n, W, hop, trim):
    s, r = hostlogic.conv_stride_and_field(CK, CS)
    F = _frames(n)
    K = 0 if F <= W else -(-(F - W) // hop)
    assert (p.n_samples, p.frames, p.K, p.stride, p.field, p.overlap) == (n, F, K, s, r, W - hop)
    assert len(p.frame_start) == len(p.window_len) == len(p.sample_start) == len(p.sample_count) == K + 1
    cover = np.zeros(F, dtype=np.int64)
    for k in range(K + 1):
        f0 = k * hop
        assert p.frame_start[k] == f0 and p.sample_start[k] == s * f0
        assert p.window_len[k] == min(W, F - f0) >= 1
        assert p.sample_count[k] == (s * (W - 1) + r if k < K else n - s * f0)
        assert p.sample_start[k] + p.sample_count[k] <= n                        # nothing past the recording's end
        assert _frames(p.sample_count[k]) == p.window_len[k]                     # the encoder gives the window exactly its frames
        # frame j of window k reads samples [s j, s j + r) of the window = [s (f0 + j), s (f0 + j) + r) of the recording: global frame f0 + j
        assert s * (p.window_len[k] - 1) + r <= p.sample_count[k]
        cover[f0:f0 + p.window_len[k]] += 1
    assert cover.min() >= 1 and cover.max() <= 2
    assert p.sample_start[K] + p.sample_count[K] == n
    if K > 0:
        assert p.window_len[K] > p.overlap
        assert all(n_ == W for n_ in p.window_len[:K])


def test_stride_and_field_come_from_the_config():
    assert hostlogic.conv_stride_and_field(CK, CS) == (320, 400)
    assert hostlogic.conv_stride_and_field((10, 3), (5, 2)) == (10, 20)          # frame j of two layers reads [10 j, 10 j + 20)
    assert hostlogic.conv_layer_lengths(20, (10, 3), (5, 2))[-1] == 1 and hostlogic.conv_layer_lengths(19, (10, 3), (5, 2))[-1] == 0


def test_plan_properties_small_windows_every_length():
    s, r = hostlogic.conv_stride_and_field(CK, CS)
    seen = set()
    for n in range(r, r + 45 * s + 1, 37):
        p = hostlogic.long_form_plan(n, CK, CS, **SMALL)
        _check_plan(p, n, 24, 16, 2)
        seen.add(p.K)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("n, K, F", [(160000, 0, 499), (160001, 0, 499), (960000, 7, 2999), (9600000, 74, 29999)])
def test_plan_properties_defaults(n, K, F):
    p = hostlogic.long_form_plan(n, CK, CS)
    assert (p.K, p.frames, p.window_frames, p.hop_frames, p.trim_frames) == (K, F, 499, 399, 25)
    _check_plan(p, n, 499, 399, 25)


def test_plan_refusals():
    with pytest.raises(ValueError, match="three windows"):
        hostlogic.long_form_plan(160000, CK, CS, window_frames=24, hop_frames=11, trim_frames=2)
    with pytest.raises(ValueError, match="three windows"):                       # whatever the recording's length
        hostlogic.long_form_plan(400, CK, CS, window_frames=24, hop_frames=11, trim_frames=2)
    with pytest.raises(ValueError, match="overlap"):
        hostlogic.long_form_plan(400 + 320 * 24, CK, CS, window_frames=24, hop_frames=16, trim_frames=4)
    hostlogic.long_form_plan(400 + 320 * 23, CK, CS, window_frames=24, hop_frames=16, trim_frames=4)       # one window: no seam to trim
    hostlogic.long_form_plan(400 + 320 * 24, CK, CS, window_frames=24, hop_frames=12, trim_frames=2)       # 2 hop == window is allowed
    with pytest.raises(ValueError, match="receptive field"):
        hostlogic.long_form_plan(399, CK, CS)
    with pytest.raises(ValueError, match="ramp"):
        hostlogic.long_form_ramp(hostlogic.long_form_plan(16000, CK, CS), "cosine")


def test_ramps():
    p = hostlogic.long_form_plan(400 + 320 * 60, CK, CS, **SMALL)
    lin, cut = hostlogic.long_form_ramp(p), hostlogic.long_form_ramp(p, "cut")
    assert lin.dtype == cut.dtype == np.float32 and lin.shape == cut.shape == (8,)
    assert lin.tolist() == [0.0, 0.0, 0.125, 0.375, 0.625, 0.875, 1.0, 1.0]      # the trimmed frames never blend
    assert cut.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    d = hostlogic.long_form_ramp(hostlogic.long_form_plan(960000, CK, CS))
    assert d.shape == (100,) and not d[:25].any() and (d[75:] == 1.0).all() and (np.diff(d[24:76]) > 0).all()
    assert d[25] == np.float32(0.5 / 50) and d[74] == np.float32(49.5 / 50)


def _grid(rng, shape):
    return (rng.integers(-4096, 4096, size=shape) / 1024.0).astype(np.float32)


def _slices(p, x):
    return [x[f0:f0 + n] for f0, n in zip(p.frame_start, p.window_len)]


@pytest.mark.parametrize("kind", ["linear", "cut"])
@pytest.mark.parametrize("F", [24, 25, 61, 72])
def test_windows_of_one_array_stitch_back_to_it(kind, F):
    p = hostlogic.long_form_plan(400 + 320 * (F - 1) + 319 * (F == 61), CK, CS, **SMALL)
    assert p.frames == F
    x = np.random.default_rng(F).standard_normal((F, 9)).astype(np.float32)
    out, am = hostlogic.long_form_stitch(_slices(p, x), p, hostlogic.long_form_ramp(p, kind))
    assert out.dtype == np.float32 and am.dtype == np.int64
    assert np.array_equal(out.view(np.int32), x.view(np.int32)) and np.array_equal(am, x.argmax(-1))


def _independent_windows(F, C, seed):
    p = hostlogic.long_form_plan(400 + 320 * (F - 1), CK, CS, **SMALL)
    rng = np.random.default_rng(seed)
    return p, [_grid(rng, (24, C))[:n] for n in p.window_len]                    # windows that disagree in their overlaps


def test_cut_takes_every_frame_from_one_window():
    p, wins = _independent_windows(72, 9, 1)
    assert p.K == 3
    out, _ = hostlogic.long_form_stitch(wins, p, hostlogic.long_form_ramp(p, "cut"))
    for t in range(72):
        k = min(t // 16, p.K)
        j = t - 16 * k
        src = wins[k - 1][j + 16] if (k > 0 and j < 4) else wins[k][j]           # the earlier window up to the middle of the overlap
        assert np.array_equal(out[t], src), t


def test_linear_trims_and_fades():
    p, wins = _independent_windows(61, 9, 2)
    assert p.K == 3 and p.window_len[-1] == 13
    ramp = hostlogic.long_form_ramp(p)
    out, am = hostlogic.long_form_stitch(wins, p, ramp)
    owned = np.zeros(61, dtype=bool)
    for k in range(1, p.K + 1):
        f0 = 16 * k
        x0, x1 = wins[k - 1][16:24], wins[k][:8]
        assert np.array_equal(out[f0:f0 + 2], x0[:2])                            # the later window's first `trim` frames are never used
        assert np.array_equal(out[f0 + 6:f0 + 8], x1[6:])                        # nor the earlier window's last `trim`
        fade = out[f0 + 2:f0 + 6]
        lo, hi = np.minimum(x0[2:6], x1[2:6]), np.maximum(x0[2:6], x1[2:6])
        assert (fade >= lo).all() and (fade <= hi).all()
        r = ramp[2:6, None]
        assert np.array_equal(fade, x0[2:6] + r * (x1[2:6] - x0[2:6]))           # the three fp32 operations, restated
        assert ((fade != x0[2:6]) | (x0[2:6] == x1[2:6])).all()                  # on this grid a weight of 1/8 always moves the value
        owned[f0:f0 + 8] = True
    for t in np.nonzero(~owned)[0]:                                              # outside the overlaps: the one covering window
        k = min(t // 16, p.K)
        assert np.array_equal(out[t], wins[k][t - 16 * k]), t
    assert np.array_equal(am, out.argmax(-1))


def test_single_window_is_a_copy():
    p = hostlogic.long_form_plan(400 + 320 * 23 + 100, CK, CS, **SMALL)
    assert (p.K, p.frames) == (0, 24)
    x = np.random.default_rng(3).standard_normal((32, 46)).astype(np.float32)   # more rows than frames: the padding is not read
    out, am = hostlogic.long_form_stitch([x], p, hostlogic.long_form_ramp(p))
    assert out.shape == (24, 46) and np.array_equal(out, x[:24]) and np.array_equal(am, x[:24].argmax(-1))
    with pytest.raises(ValueError, match="windows"):
        hostlogic.long_form_stitch([x, x], p, hostlogic.long_form_ramp(p))


def test_ties_go_to_the_lowest_index():
    p, _ = _independent_windows(40, 46, 4)
    rng = np.random.default_rng(5)
    wins = [rng.integers(0, 3, size=(n, 46)).astype(np.float32) for n in p.window_len]      # integer logits: many equal maxima
    out, am = hostlogic.long_form_stitch(wins, p, hostlogic.long_form_ramp(p, "cut"))
    top = out.max(-1)
    assert ((out == top[:, None]).sum(-1) > 1).all()                             # every frame is tied
    for t in range(40):
        assert am[t] == np.nonzero(out[t] == top[t])[0][0], t
