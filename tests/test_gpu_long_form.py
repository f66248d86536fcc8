"""GPU: long recordings - aptai_window_gather, aptai_stitch_windows and the `*_long` helpers of APTAI and Wav2Vec2_PR.

Windows of 24 frames every 16, trim 2 (overlap 8, a fade over 4 frames).  Four recordings of 24 / 25 / 72 / 61 frames, the last with 319
samples past its last frame: one window, a last window of overlap + 1 frames, a full last window, a ragged tail.  The longest has
23 120 samples.

Bounds.  Everything is demanded bit for bit:
 * the two kernels against numpy slicing / hostlogic.long_form_stitch: copies, and three fp32 operations that numpy rounds the same way;
 * end to end, a window's result must not depend on the windows it shares a forward with: tests/test_gpu_batch_invariant.py records a
   measured 0.0 for APTAI and recogniser rows, batched against alone (its TOL), and these tests lean on exactly that - the long helpers
   against the existing `get_aptai_outputs` / `get_ctc_logits` of the window slices, stitched by the numpy oracle, and groups of 2
   windows against one forward of all.  `phn_fc_probs` is torch's softmax of the stitched logits, compared with the same call on the
   oracle's logits.
Nothing here says anything about accuracy at the seams: with random weights there is nothing to say ("Long recordings").
"""
import numpy as np
import pytest
import torch

from aptai_amd import hostlogic

pytestmark = pytest.mark.gpu

CK, CS = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
PLAN = dict(window_frames=24, hop_frames=16, trim_frames=2)
FRAMES = (24, 25, 72, 61)
LENS = tuple(400 + 320 * (f - 1) + (319 if f == 61 else 0) for f in FRAMES)
PLANS = [hostlogic.long_form_plan(n, CK, CS, **PLAN) for n in LENS]
assert max(LENS) == 23120 and [p.frames for p in PLANS] == list(FRAMES) and [p.K for p in PLANS] == [0, 1, 3, 3]
assert [p.window_len[-1] for p in PLANS] == [24, 9, 24, 13]
NW = sum(p.K + 1 for p in PLANS)                                                 # 11 windows
S = 24 * 320 + 80                                                                # samples of a full window


def _wavs():
    g = torch.Generator().manual_seed(77)
    return [torch.randn(n, generator=g).numpy() for n in LENS]


def _window_table():
    rows, off = [], 0
    for p in PLANS:
        rows += [(off, a, n) for a, n in zip(p.sample_start, p.sample_count)]
        off += p.n_samples
    return rows


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32 and not np.array_equal(_bits(a), _bits(b)):
        raise AssertionError(f"{what}: max |difference| = {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3e}")
    assert np.array_equal(a, b), what


# ------------------------------------------------------------------------------------------------ 1. aptai_window_gather
def test_window_gather_equals_numpy_slicing():
    from aptai_amd import ops
    wavs = _wavs()
    table = _window_table()
    assert len(table) == NW and max(n for _, _, n in table) == S
    packed_h = np.concatenate(wavs)
    packed = torch.from_numpy(packed_h).cuda()
    tab = torch.tensor(table, dtype=torch.int64).cuda()
    ref = np.zeros((NW, S), dtype=np.float32)
    for i, (off, a, n) in enumerate(table):
        ref[i, :n] = packed_h[off + a:off + a + n]
    audio, lens = ops.window_gather(packed, tab, 0, NW, S)
    assert audio.shape == (NW, S) and lens.dtype == torch.int64
    assert np.array_equal(_bits(audio.cpu().numpy()), _bits(ref))                # the samples, and exact zeros behind them
    assert lens.cpu().tolist() == [n for _, _, n in table]
    for group in (1, 2):
        for first in range(0, NW, group):
            a, l = ops.window_gather(packed, tab, first, min(group, NW - first), S)
            assert torch.equal(a, audio[first:first + group]) and torch.equal(l, lens[first:first + group]), (group, first)
    # an odd width takes the scalar stores, a wider batch zero-fills to its width
    a, l = ops.window_gather(packed, tab, 3, 4, S + 3)
    assert torch.equal(a[:, :S], audio[3:7]) and not a[:, S:].any() and torch.equal(l, lens[3:7])
    with pytest.raises(ops._lib.AptaiHipError, match="windows"):
        ops.window_gather(packed, tab, NW - 1, 2, S)


# ------------------------------------------------------------------------------------------------ 2. aptai_stitch_windows
def _stitch_case(C, ldx, rpw, kind, data, per_recording_rows):
    """Windows of the four recordings with junk in every row and column a window does not own; device result vs the oracle."""
    from aptai_amd import ops
    rng = np.random.default_rng(C * 7 + len(kind))
    x = np.full((NW * rpw, ldx), 3.0e30, dtype=np.float32)                       # not a frame: would win every argmax
    wins, w0 = [], 0
    for p in PLANS:
        mine = []
        for k, n in enumerate(p.window_len):
            v = rng.standard_normal((n, C)).astype(np.float32) if data == "random" else rng.integers(0, 3, (n, C)).astype(np.float32)
            x[(w0 + k) * rpw:(w0 + k) * rpw + n, :C] = v
            mine.append(v)
        wins.append(mine)
        w0 += p.K + 1
    ramp = hostlogic.long_form_ramp(PLANS[2], kind)
    max_f = max(FRAMES)
    starts = [r * max_f for r in range(4)] if per_recording_rows else np.cumsum((0,) + FRAMES[:-1]).tolist()
    out_rows = 4 * max_f if per_recording_rows else sum(FRAMES)
    rec, w0 = [], 0
    for p, o0 in zip(PLANS, starts):
        rec.append((w0, p.frames, o0))
        w0 += p.K + 1
    ldo = C + 3
    out = torch.full((out_rows, ldo), -7.0, device="cuda")
    got, am = ops.stitch_windows(torch.from_numpy(x).cuda(), ldx, rpw, NW, torch.tensor(rec, dtype=torch.int64).cuda(), max_f, 24, 16,
                                 torch.from_numpy(ramp).cuda(), C, out=out)
    assert got is out and am.dtype == torch.int64 and am.shape == (out_rows,)
    got, am = got.cpu().numpy(), am.cpu().numpy()
    owned = np.zeros(out_rows, dtype=bool)
    for p, mine, o0 in zip(PLANS, wins, starts):
        ref, ref_am = hostlogic.long_form_stitch(mine, p, ramp)
        assert np.array_equal(_bits(got[o0:o0 + p.frames, :C]), _bits(ref)), (C, kind, data, p.frames)
        assert np.array_equal(am[o0:o0 + p.frames], ref_am), (C, kind, data, p.frames)
        if data == "ties":
            assert ((ref == ref.max(-1, keepdims=True)).sum(-1) > 1).any()
        owned[o0:o0 + p.frames] = True
    assert (got[:, C:] == -7.0).all() and (got[~owned] == -7.0).all() and not am[~owned].any()      # nothing else was touched
    assert (got[owned, :C] != -7.0).all()                                                           # and every owned element was written


@pytest.mark.parametrize("C, ldx, rpw", [(9, 9, 24), (46, 64, 128), (40, 64, 128)])
@pytest.mark.parametrize("kind", ["linear", "cut"])
def test_stitch_windows_equals_the_oracle(C, ldx, rpw, kind):
    _stitch_case(C, ldx, rpw, kind, "random", per_recording_rows=(C == 40))
    _stitch_case(C, ldx, rpw, kind, "ties", per_recording_rows=(C == 40))


def test_stitch_windows_refusals_and_wide_rows():
    from aptai_amd import ops
    x = torch.zeros((NW * 24, 300), device="cuda")
    rec = torch.tensor([(0, 24, 0)], dtype=torch.int64).cuda()
    ramp = torch.from_numpy(hostlogic.long_form_ramp(PLANS[2])).cuda()
    with pytest.raises(ops._lib.AptaiHipError, match="channels"):
        ops.stitch_windows(x, 300, 24, NW, rec, 24, 24, 16, ramp, 257, out_rows=24)
    with pytest.raises(ops._lib.AptaiHipError, match="hop_frames"):
        ops.stitch_windows(x, 300, 24, NW, rec, 24, 24, 11, None, 9, out_rows=24)
    with pytest.raises(ops._lib.AptaiHipError, match="rows"):
        ops.stitch_windows(x, 300, 16, NW, rec, 24, 24, 16, ramp, 9, out_rows=24)
    # 256 channels: four per lane, the argmax across all of them
    v = torch.randn(24, 256, generator=torch.Generator().manual_seed(1))
    x[:24, :256] = v.cuda()
    out, am = ops.stitch_windows(x, 300, 24, NW, rec, 24, 24, 16, None, 256, out_rows=24)
    assert torch.equal(out.cpu(), v) and torch.equal(am.cpu(), v.argmax(-1))


# ------------------------------------------------------------------------------------------------ 3. APTAI end to end
@pytest.fixture(scope="module", params=["large", "base"])
def aptai(request):
    from test_gpu_batch_invariant import build_aptai
    model = build_aptai(request.param)[0]
    wavs = _wavs()
    with torch.no_grad():
        alls = [model.get_aptai_output_long(w, **PLAN) for w in wavs]            # all windows of a recording in one forward
    return model, wavs, alls


def _same_output(a, b, what):
    assert set(a) == set(b) == {"phn_fc_probs", "phn_fc_logits", "phn_fc_pred", "tvs_pred"}
    for k in ("phn_fc_probs", "phn_fc_logits", "phn_fc_pred"):
        _same(a[k], b[k], (what, k))
    assert list(a["tvs_pred"]) == list(b["tvs_pred"])
    for name in a["tvs_pred"]:
        _same(np.asarray(a["tvs_pred"][name]), np.asarray(b["tvs_pred"][name]), (what, name))


def test_a_short_recording_is_the_short_helper_with_the_switch_on(aptai):
    model, wavs, alls = aptai
    model.batch_invariant = True
    try:
        one = model.get_aptai_output(wavs[0])
    finally:
        model.batch_invariant = False
    assert one["phn_fc_logits"].shape == (24, 46) and one["phn_fc_probs"].shape == (46, 24, 1) and one["phn_fc_pred"].shape == (24,)
    assert one["phn_fc_pred"].dtype == np.int64 and len(one["tvs_pred"]["LA"]) == 24
    _same_output(alls[0], one, "24 frames")
    assert model.batch_invariant is False and model.wav2vec2.batch_invariant is False


@pytest.mark.parametrize("r", [1, 2, 3])
def test_long_recordings_equal_the_stitched_window_results(aptai, r):
    model, wavs, alls = aptai
    p, got = PLANS[r], alls[r]
    per_window = model.get_aptai_outputs([wavs[r][a:a + n] for a, n in zip(p.sample_start, p.sample_count)])
    assert [len(w["phn_fc_pred"]) for w in per_window] == list(p.window_len)
    ramp = hostlogic.long_form_ramp(p)
    logits, pred = hostlogic.long_form_stitch([w["phn_fc_logits"] for w in per_window], p, ramp)
    tvs, _ = hostlogic.long_form_stitch([np.stack([np.asarray(w["tvs_pred"][n]) for n in hostlogic.TV_NAMES], -1) for w in per_window], p, ramp)
    assert got["phn_fc_logits"].shape == (p.frames, 46) and got["phn_fc_probs"].shape == (46, p.frames, 1)
    _same(got["phn_fc_logits"], logits, (r, "logits"))
    _same(got["phn_fc_pred"], pred, (r, "pred"))
    probs = torch.softmax(torch.from_numpy(logits).cuda(), dim=-1).cpu().numpy()
    _same(got["phn_fc_probs"], probs[None].transpose(2, 1, 0), (r, "probs"))
    for i, name in enumerate(hostlogic.TV_NAMES):
        _same(np.asarray(got["tvs_pred"][name]), tvs[:, i], (r, name))
    # a seam is a seam: inside the fade the stitched logits are neither window's
    f0 = 16
    assert not np.array_equal(logits[f0 + 2:f0 + 6], per_window[0]["phn_fc_logits"][18:22])
    assert not np.array_equal(logits[f0 + 2:f0 + 6], per_window[1]["phn_fc_logits"][2:6])
    # groups of two windows, results carried across the groups' seams
    with torch.no_grad():
        _same_output(model.get_aptai_output_long(wavs[r], windows_per_forward=2, **PLAN), got, (r, "groups of 2"))
        cut = model.get_aptai_output_long(wavs[r], ramp="cut", **PLAN)
    _same(cut["phn_fc_logits"], hostlogic.long_form_stitch([w["phn_fc_logits"] for w in per_window], p, hostlogic.long_form_ramp(p, "cut"))[0],
          (r, "cut"))


def test_the_list_helper_equals_the_single_calls(aptai):
    model, wavs, alls = aptai
    with torch.no_grad():
        many = model.get_aptai_outputs_long(wavs, **PLAN)
        many3 = model.get_aptai_outputs_long(wavs, windows_per_forward=3, **PLAN)
    assert len(many) == len(many3) == 4 and model.get_aptai_outputs_long([]) == []
    for r in range(4):
        _same_output(many[r], alls[r], (r, "list"))
        _same_output(many3[r], alls[r], (r, "list, groups of 3"))


def test_refusals(aptai):
    model, wavs, _ = aptai
    with pytest.raises(ValueError, match="three windows"):
        model.get_aptai_output_long(wavs[1], window_frames=24, hop_frames=11, trim_frames=2)
    with pytest.raises(ValueError, match="windows_per_forward"):
        model.get_aptai_output_long(wavs[1], windows_per_forward=0, **PLAN)
    with pytest.raises(ValueError, match="receptive field"):
        model.get_aptai_output_long(wavs[1][:399], **PLAN)
    w = model.wav2vec2
    prec = w._encoder_precision
    w._encoder_precision = "f32x3"
    try:
        with pytest.raises(NotImplementedError, match="f32x3"):
            model.get_aptai_output_long(wavs[1], **PLAN)
    finally:
        w._encoder_precision = prec


# ------------------------------------------------------------------------------------------------ 4. the recogniser
@pytest.fixture(scope="module", params=["large", "base"])
def recogniser(request):
    from test_gpu_batch_invariant import build_pr
    model = build_pr(request.param)[0]
    model.vocab = {("(blank)" if i == 0 else "(...)" if i == 5 else f"p{i}"): i for i in range(40)}
    return model, _wavs()


def test_recogniser_short_recording_is_the_short_helper_with_the_switch_on(recogniser):
    model, wavs = recogniser
    model.batch_invariant = True
    try:
        one = model.get_ctc_logits(wavs[0])
        dur = model.predict_phonemes_durations(wavs[0], model.vocab)
        seq = model.pred_phn_seq(wavs[0], model.vocab)
    finally:
        model.batch_invariant = False
    _same(model.get_ctc_logits_long(wavs[0], **PLAN), one, "logits")
    got = model.predict_phonemes_durations_long(wavs[0], model.vocab, **PLAN)
    assert list(got["phn_seq_idx"]) == list(dur["phn_seq_idx"]) and got["phn_seq_ipa"] == dur["phn_seq_ipa"]
    assert got["phn_seq_dur"] == dur["phn_seq_dur"]
    got = model.pred_phn_seq_long(wavs[0], model.vocab, **PLAN)
    assert list(got["phn_seq_idx"]) == list(seq["phn_seq_idx"]) and got["phn_seq_ipa"] == seq["phn_seq_ipa"]
    assert model.batch_invariant is False and model.wav2vec2.batch_invariant is False


@pytest.mark.parametrize("r", [1, 2, 3])
def test_recogniser_long_logits_and_decodes(recogniser, r):
    from aptai_amd import ops
    model, wavs = recogniser
    p, wav = PLANS[r], wavs[r]
    model.batch_invariant = True
    try:
        per_window = [model.get_ctc_logits(wav[a:a + n]) for a, n in zip(p.sample_start, p.sample_count)]       # each window alone
    finally:
        model.batch_invariant = False
    ref, ref_am = hostlogic.long_form_stitch(per_window, p, hostlogic.long_form_ramp(p))
    logits = model.get_ctc_logits_long(wav, **PLAN)
    _same(logits, ref, (r, "logits"))
    _same(model.get_ctc_logits_long(wav, windows_per_forward=2, **PLAN), ref, (r, "groups of 2"))
    # the decodes, fed by hand with the stitched matrix as one row of F frames
    F, V = p.frames, 40
    dev = torch.from_numpy(ref).cuda()
    ratio = len(wav) / F / 16000
    ids, ts, n = ops.ctc_greedy_decode(dev, V, F, 1, F, V, 0, F + 2, want_timesteps=True)
    n = int(n[0])
    ids, ts = ids[0, :n].cpu().tolist(), ts[0, :n].cpu().tolist()
    assert ids == hostlogic.ctc_best_path(ref, F, 0).tolist() and ids == hostlogic.ctc_bracketed_best_path(ref, F, 0)[0].tolist()
    got = model.predict_phonemes_durations_long(wav, model.vocab, **PLAN)
    assert list(got["phn_seq_idx"]) == ids and got["phn_seq_dur"] == [t * ratio for t in ts]
    assert got["phn_seq_ipa"] == [f"p{i}" if i not in (0, 5) else "(...)" for i in ids]
    assert list(model.pred_phn_seq_long(wav, model.vocab, **PLAN)["phn_seq_idx"]) == ids
    model.decoder = "beam"
    try:
        beam = model.predict_phonemes_durations_long(wav, model.vocab, **PLAN)
    finally:
        model.decoder = "best_path"
    tokens, timesteps, n_tok, _, _ = ops.ctc_beam_search(dev, V, F, 1, F, V, 0, 5, max_n=F + 2, **model.beam_options)
    n = int(n_tok[0, 0])
    assert list(beam["phn_seq_idx"]) == tokens[0, 0, :n].cpu().tolist()
    assert beam["phn_seq_dur"] == [t * ratio for t in timesteps[0, 0, :n].cpu().tolist()]
    assert model.decoder == "best_path" and model.batch_invariant is False
