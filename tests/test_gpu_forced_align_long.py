"""GPU: forced alignment of long recordings - aptai_ctc_viterbi_wide at operator level and Wav2Vec2_PR.force_align_long /
align_phonemes_durations_long end to end.

The PATH (frame_token, spans) is demanded bit for bit against hostlogic.ctc_forced_align: both sides perform the same single fp32
addition per state and frame and the same tie rule, whatever the kernel's decomposition into threads, waves and backtrace chunks.
For label rows the narrow kernel takes (ldt <= 255) all four outputs are demanded equal to aptai_ctc_viterbi's.

Score bounds (restated from tests/test_gpu_forced_align.py; the wide kernel takes lz from the narrow kernel's reduction and sums in
its orders).  u = unit roundoff of fp32, EPS = 2u (a factor 2 of margin for <= 1 ulp expf / logf), A = max |logit|, V classes:
 * one frame's d = x - lz:  x_j - mx: 2A u;  expf of it: 2A u (argument) + 2u;  the sum of V positive terms (<= 3 per-lane additions
   + 6 shuffle levels): 10u  ->  relative error of se <= (2A + 12) u = absolute error of log(se);  logf: 2u ln V;  lz = mx + log se:
   u (A + ln V);  d = x - lz: u (2A + ln V).  Sum: u (5A + 4 ln V + 12)                                             (_frame_bound)
 * score = sum of Tb terms d_t <= 0, so sum |d_t| = |score|: 256 threads add ceil(Tb / 256) terms each in order, then 8 levels of a
   fixed tree: (ceil(Tb / 256) + 8) u |score|, plus Tb per-frame errors                                             (_score_bound)
 * token_score = (sequential sum of n terms) / n: (n - 1) u |mean| + u |mean| for the division + one per-frame error (_token_bound)

The logits carry 3e30 in every column beyond V and every row beyond a recording's length (rows_per_b > T, ldl = 64 > V = 46): a read
outside the operands would win every maximum.  Nothing here says anything about accuracy at the seams (random weights).
"""
import functools
import math

import numpy as np
import pytest
import torch

from aptai_amd import hostlogic

pytestmark = pytest.mark.gpu

V, LDL, JUNK = 46, 64, 3.0e30
EPS = 2.0 ** -23
CHUNK = 256                                                       # frames per backtrace chunk of the kernel (csrc/ctc.hip)
# label counts: the first beyond the narrow kernel (2 states per thread), then one per wider instantiation (4, 8, 16 states per
# thread: 2 L + 1 > 1024, > 2048, > 4096)
SIZES = [(256, 600), (700, 900), (1500, 1700), (4100, 4300)]
CK, CS = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
PLAN = dict(window_frames=24, hop_frames=16, trim_frames=2)
FRAMES = (24, 25, 72, 61)
LENS = tuple(400 + 320 * (f - 1) + (319 if f == 61 else 0) for f in FRAMES)
PLANS = [hostlogic.long_form_plan(n, CK, CS, **PLAN) for n in LENS]


def _frame_bound(A, Vb):
    return EPS * (5.0 * A + 4.0 * math.log(max(Vb, 2)) + 12.0)


def _score_bound(A, Vb, Tb, score):
    return Tb * _frame_bound(A, Vb) + (math.ceil(Tb / 256) + 8) * EPS * abs(score)


def _token_bound(A, Vb, n, mean):
    return _frame_bound(A, Vb) + (n + 1) * EPS * abs(mean)


def _distinct(rng, n, Vb=V):
    """n labels in 1 .. Vb-1, no two neighbours equal: every odd state may be entered from two states below."""
    out = rng.randint(1, Vb, size=n)
    for k in range(1, n):
        while out[k] == out[k - 1]:
            out[k] = rng.randint(1, Vb)
    return [int(v) for v in out]


def _logits(rng, B, T, in_lens, *, col0=0, integer_rows=(), nv=V, ldl=LDL):
    """[B][T + 3][ldl]: N(0, 2) (rows in `integer_rows`: values in {0, 1, 2}, ties everywhere) in the nv columns from col0 on of each
    row's own frames, JUNK everywhere else."""
    x = np.full((B, T + 3, ldl), JUNK, dtype=np.float32)
    for b in range(B):
        n = max(0, min(in_lens[b], T))
        v = rng.randint(0, 3, size=(n, nv)).astype(np.float32) if b in integer_rows else (rng.randn(n, nv) * 2).astype(np.float32)
        x[b, :n, col0:col0 + nv] = v
    return x


def _launch(x, targets, in_lens, T, *, ldt=None, vocab_sizes=None, col0=0, narrow=False, topology="ctc", nv=V):
    from aptai_amd import ops
    B, rows_per_b, ldl = x.shape
    ldt = max([len(t) for t in targets] + [1]) if ldt is None else ldt
    tg = np.full((B, ldt), -100, dtype=np.int32)
    for b, t in enumerate(targets):
        tg[b, :len(t)] = t
    xd = torch.from_numpy(x).cuda().reshape(B * rows_per_b, ldl)
    tgd = torch.from_numpy(tg).cuda()
    lens = torch.tensor(in_lens, dtype=torch.int32).cuda()
    tl = torch.tensor([len(t) for t in targets], dtype=torch.int32).cuda()
    vs = None if vocab_sizes is None else torch.tensor(vocab_sizes, dtype=torch.int32).cuda()
    fn = ops.ctc_viterbi if narrow else ops.ctc_viterbi_wide
    out = fn(xd[:, col0:] if col0 else xd, ldl, rows_per_b, tgd, lens, tl, B, T, nv, vocab_sizes_i32=vs, topology=topology)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _oracle(x, targets, in_lens, T, *, vocab_sizes=None, col0=0, ldt=None, nv=V):
    """Per row: (frame_token, spans, fp64 score, per-frame fp64 log-probabilities, A, Vb, Tb)."""
    ldt = max([len(t) for t in targets] + [1]) if ldt is None else ldt
    rows = []
    for b in range(x.shape[0]):
        Vb = nv if vocab_sizes is None else vocab_sizes[b]
        xb = x[b, :T, col0:col0 + Vb]
        ft, score = hostlogic.ctc_forced_align(xb, in_lens[b], targets[b])
        Tb = max(0, min(int(in_lens[b]), T))
        x64 = xb[:Tb].astype(np.float64)
        mx = x64.max(axis=1) if Tb else np.zeros(0)
        lp = x64 - (mx + np.log(np.exp(x64 - mx[:, None]).sum(axis=1)))[:, None]
        rows.append((ft, hostlogic.alignment_spans(ft, ldt), score, lp, float(np.abs(xb[:Tb]).max()) if Tb else 0.0, Vb, Tb))
    return rows


def _assert_path(out, ref):
    ft, spans = out[0].numpy(), out[1].numpy()
    for b, (r_ft, r_sp, *_) in enumerate(ref):
        assert np.array_equal(ft[b], r_ft), (b, int((ft[b] != r_ft).sum()), int(np.nonzero(ft[b] != r_ft)[0][0]))
        assert np.array_equal(spans[b], r_sp), b


def _assert_scores(out, ref, targets):
    score, tsc = out[2].numpy(), out[3].numpy()
    worst = worst_tok = 0.0
    for b, (_, r_sp, r_score, lp, A, Vb, Tb) in enumerate(ref):
        if not np.isfinite(r_score):
            assert score[b] == -np.inf and np.all(tsc[b] == -np.inf), b
            continue
        bound = _score_bound(A, Vb, Tb, r_score)
        print(f"[wide align] b={b} score {float(score[b]):.6f} fp64 {r_score:.6f} bound {bound:.3e}")
        assert abs(float(score[b]) - r_score) <= bound, (b, float(score[b]), r_score, bound)
        worst = max(worst, abs(float(score[b]) - r_score) / max(bound, 1e-30))
        for k in range(r_sp.shape[0]):
            f0, f1 = r_sp[k]
            if f0 < 0:
                assert tsc[b, k] == -np.inf, (b, k)
                continue
            mean = float(lp[f0:f1, targets[b][k]].mean())
            tb = _token_bound(A, Vb, f1 - f0, mean)
            assert abs(float(tsc[b, k]) - mean) <= tb, (b, k, float(tsc[b, k]), mean, tb)
            worst_tok = max(worst_tok, abs(float(tsc[b, k]) - mean) / tb)
    print(f"[wide align] worst |score - fp64| / bound = {worst:.3f}, worst |token_score - fp64| / bound = {worst_tok:.3f}")


# ------------------------------------------------------------------------------------------------ operator level
def _transcripts(rng, L):
    """Four transcripts of a size: (0) no two neighbours equal and barely more frames than labels: the path climbs two states per
    frame; (1) five labels, long stays; (2) a run of 20 equal labels, then a repeat at every multiple of 8 labels - the first label
    of a thread of 16 states, of every second thread of 8, of every fourth of 4, and with the multiples of 64 the first of a wave of
    2-state threads (every multiple of 512: the first of a wave of 16-state threads) - so the forbidden skip is asked for across
    every boundary of the layout; (3) integer logits, every comparison a tie somewhere."""
    rep = _distinct(rng, L - L // 4)
    rep[:20] = [rep[0]] * 20
    for k in range(24, len(rep), 8):
        rep[k] = rep[k - 1]
    return [_distinct(rng, L), _distinct(rng, 5), rep, _distinct(rng, L)]


@functools.lru_cache(maxsize=None)
def _case(L, T):
    """One launch and one oracle per size, shared by the path, score and determinism tests."""
    rng = np.random.RandomState(L + T)
    targets = _transcripts(rng, L)
    in_lens = [L + 2, T, T - 1, T]
    x = _logits(rng, 4, T, in_lens, integer_rows=(3,))
    return x, targets, in_lens, _launch(x, targets, in_lens, T), _oracle(x, targets, in_lens, T)


@pytest.mark.parametrize("L, T", SIZES)
def test_path_equals_the_host_oracle(L, T):
    x, targets, in_lens, out, ref = _case(L, T)
    assert T > 2 * CHUNK and out[0].shape == (4, T) and out[1].shape == (4, L, 2) and out[3].shape == (4, L)
    assert all(np.isfinite(r[2]) for r in ref)                                    # every transcript fits: there is a path to compare
    _assert_path(out, ref)
    ft = out[0].numpy()
    assert (ft[0, :L + 2] >= 0).sum() >= L and (ft[0, L + 2:] == -2).all()         # row 0 has no room to dwell: two states per frame


@pytest.mark.parametrize("L, T", SIZES)
def test_scores_beyond_255_labels(L, T):
    x, targets, in_lens, out, ref = _case(L, T)
    _assert_scores(out, ref, targets)


@pytest.mark.parametrize("ldt", [20, 100, 255])
def test_all_outputs_equal_the_narrow_kernel(ldt):
    rng = np.random.RandomState(ldt)
    T = 300
    in_lens = [300, 280, 290]
    targets = [[int(v) for v in rng.randint(1, V, size=n)] for n in (ldt, ldt // 2, max(ldt - 3, 1))]
    x = _logits(rng, 3, T, in_lens)
    wide = _launch(x, targets, in_lens, T, ldt=ldt)
    narrow = _launch(x, targets, in_lens, T, ldt=ldt, narrow=True)
    assert torch.isfinite(narrow[2][:2]).all()
    for name, a, b in zip(("frame_token", "spans", "score", "token_score"), wide, narrow):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32)), name        # bits, also of the floats


@pytest.mark.parametrize("vocab_sizes, col0", [(None, 0), ([46, 30, 46, 20, 40], 0), (None, 3)])
def test_edges_in_one_batch(vocab_sizes, col0):
    """A wide row, a row without frames, a row without labels, a transcript that does not fit, a label outside the vocabulary."""
    rng = np.random.RandomState(17 + col0)
    T = 400
    in_lens = [T, 0, 50, 30, T]
    vs = vocab_sizes or [V] * 5
    targets = [_distinct(rng, 300, vs[0]), _distinct(rng, 10, vs[1]), [], _distinct(rng, 40, vs[3]), _distinct(rng, 20, vs[4])]
    targets[4][7] = vs[4] + 3 if vocab_sizes else 50                                 # no such class
    x = _logits(rng, 5, T, in_lens, col0=col0)
    out = _launch(x, targets, in_lens, T, vocab_sizes=vocab_sizes, col0=col0)
    ref = _oracle(x, targets, in_lens, T, vocab_sizes=vocab_sizes, col0=col0)
    _assert_path(out, ref)
    _assert_scores(out, ref, targets)
    ft, spans, score, tsc = out
    assert np.isfinite(float(score[0])) and float(score[2]) < 0 and ft[2, :50].eq(-1).all() and ft[2, 50:].eq(-2).all()
    for b in (1, 3, 4):
        assert score[b] == -np.inf and ft[b].eq(-2).all() and spans[b].eq(-1).all() and tsc[b].eq(-np.inf).all(), b
    # the wide row alone: its neighbours did not touch it
    alone = _launch(x[:1], targets[:1], in_lens[:1], T, vocab_sizes=None if vocab_sizes is None else vocab_sizes[:1], col0=col0)
    for a, b in zip(out, alone):
        assert np.array_equal(a[:1].numpy().view(np.int32), b.numpy().view(np.int32))


def test_a_vocabulary_of_more_than_64_classes():
    """V = 200: four staged columns per lane where every other case here has one; row pitch 256, a per-row vocabulary on one row."""
    rng = np.random.RandomState(200)
    T, nv = 530, 200
    vs = [200, 130, 200]
    in_lens = [T, T - 9, 300]
    targets = [_distinct(rng, 400, vs[0]), _distinct(rng, 300, vs[1]), [int(v) for v in rng.randint(1, 200, size=120)]]
    x = _logits(rng, 3, T, in_lens, nv=nv, ldl=256)
    out = _launch(x, targets, in_lens, T, vocab_sizes=vs, nv=nv)
    ref = _oracle(x, targets, in_lens, T, vocab_sizes=vs, nv=nv)
    assert all(np.isfinite(r[2]) for r in ref)
    _assert_path(out, ref)
    _assert_scores(out, ref, targets)


def test_at_the_label_cap_and_refusals():
    from aptai_amd import ops
    assert ops.CTC_VITERBI_WIDE_MAX_LABELS == 8191
    rng = np.random.RandomState(8191)
    L, T = 8191, 8400
    targets = [_distinct(rng, L)]
    x = _logits(rng, 1, T, [T])
    ft, spans, score, tsc = _launch(x, targets, [T], T)
    ft, sp = ft[0].numpy(), spans[0].numpy()
    assert (ft >= -1).all()
    tok = ft[ft >= 0]
    first = np.concatenate([[True], tok[1:] != tok[:-1]])
    assert np.array_equal(tok[first], np.arange(L))                                  # collapses to the transcript, position by position
    assert (sp[:, 0] < sp[:, 1]).all() and (sp[1:, 0] >= sp[:-1, 1]).all() and sp[0, 0] >= 0 and sp[-1, 1] <= T   # ordered, disjoint
    assert np.array_equal(sp, hostlogic.alignment_spans(ft, L))
    lp = torch.log_softmax(torch.from_numpy(x[0, :T, :V]).double(), dim=-1)
    cls = torch.from_numpy(np.where(ft >= 0, np.asarray(targets[0])[np.maximum(ft, 0)], 0).astype(np.int64))
    want = float(lp[torch.arange(T), cls].sum())
    bound = _score_bound(float(np.abs(x[0, :T, :V]).max()), V, T, want)
    print(f"[wide align] cap: score {float(score[0]):.6f} fp64 {want:.6f} bound {bound:.3e}")
    assert abs(float(score[0]) - want) <= bound
    assert torch.isfinite(tsc).all()
    small = _logits(rng, 1, 8, [8])
    with pytest.raises(ops._lib.AptaiHipError, match="8191"):
        _launch(small, [[1]], [8], 8, ldt=8192)
    with pytest.raises(ops._lib.AptaiHipError, match="topology"):
        _launch(small, [[1]], [8], 8, topology="monotonic")


def test_same_inputs_same_bits():
    x, targets, in_lens, out, _ = _case(700, 900)
    again = _launch(x, targets, in_lens, 900)
    for a, b in zip(out, again):
        assert np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))


# ------------------------------------------------------------------------------------------------ end to end
def _wavs():
    g = torch.Generator().manual_seed(77)
    return [torch.randn(n, generator=g).numpy() for n in LENS]


@pytest.fixture(scope="module")
def aligned():
    """The recogniser of tests/test_gpu_long_form.py, the four recordings aligned to transcripts of 12 .. 20 labels in one call, and
    the numpy oracle over each recording's per-window logits."""
    from test_gpu_batch_invariant import build_pr
    model = build_pr("base")[0]
    model.vocab = {("(blank)" if i == 0 else "(...)" if i == 5 else f"p{i}"): i for i in range(40)}
    wavs = _wavs()
    rng = np.random.RandomState(5)
    seqs = [_distinct(rng, n, 40) for n in (12, 20, 17, 15)]
    res = model.force_align_long(wavs, seqs, **PLAN)
    assert all(v.is_cuda for v in res.values())
    ref = []
    model.batch_invariant = True
    try:
        for p, wav, q in zip(PLANS, wavs, seqs):
            per_window = [model.get_ctc_logits(wav[a:a + n]) for a, n in zip(p.sample_start, p.sample_count)]      # each window alone
            ref.append(hostlogic.long_form_force_align(per_window, p, "linear", q, blank=0))
    finally:
        model.batch_invariant = False
    return model, wavs, seqs, res, ref


def test_force_align_long_equals_the_oracle(aligned):
    model, wavs, seqs, res, ref = aligned
    ft, sp = res["frame_token"].cpu().numpy(), res["spans"].cpu().numpy()
    score, tsc, fp = res["score"].cpu().numpy(), res["token_score"].cpu().numpy(), res["frame_phns"].cpu().numpy()
    assert res["frame_seq_lens"].dtype == torch.int32 and res["frame_seq_lens"].cpu().tolist() == list(FRAMES)
    assert ft.shape == fp.shape == (4, 72) and sp.shape == (4, 20, 2) and tsc.shape == (4, 20) and ft.dtype == fp.dtype == np.int32
    for r, (q, (r_ft, r_sp, r_score, logits)) in enumerate(zip(seqs, ref)):
        F, n = FRAMES[r], len(q)
        assert np.isfinite(r_score)
        assert np.array_equal(ft[r, :F], r_ft) and (ft[r, F:] == -2).all(), r
        assert np.array_equal(sp[r, :n], r_sp) and (sp[r, n:] == -1).all(), r
        A = float(np.abs(logits).max())
        assert abs(float(score[r]) - r_score) <= _score_bound(A, 40, F, r_score), (r, float(score[r]), r_score)
        x64 = logits.astype(np.float64)
        mx = x64.max(axis=1)
        lp = x64 - (mx + np.log(np.exp(x64 - mx[:, None]).sum(axis=1)))[:, None]
        for k in range(n):
            mean = float(lp[r_sp[k, 0]:r_sp[k, 1], q[k]].mean())
            assert abs(float(tsc[r, k]) - mean) <= _token_bound(A, 40, r_sp[k, 1] - r_sp[k, 0], mean), (r, k)
        assert (tsc[r, n:] == -np.inf).all()
        # frame_phns and frame_seq_lens as the force_align test reads them
        valid, tok = fp[r, :F], ft[r, :F]
        assert (fp[r, F:] == 0).all() and (tok >= -1).all() and (valid[tok == -1] == 0).all()
        assert [int(p) for i, p in enumerate(valid) if tok[i] >= 0 and (i == 0 or tok[i] != tok[i - 1])] == q


def test_one_window_is_force_align_with_the_switch_on(aligned):
    model, wavs, seqs, _, _ = aligned
    one = model.force_align_long(wavs[:1], seqs[:1], **PLAN)
    model.batch_invariant = True
    try:
        short = model.force_align(torch.from_numpy(wavs[0])[None].cuda(), torch.tensor([len(wavs[0])]).cuda(),
                                  torch.tensor([seqs[0]], dtype=torch.int32))
    finally:
        model.batch_invariant = False
    assert set(one) == set(short)
    for k in short:
        assert one[k].dtype == short[k].dtype and one[k].shape == short[k].shape, k
        assert np.array_equal(one[k].cpu().numpy().view(np.int32), short[k].cpu().numpy().view(np.int32)), k
    assert np.isfinite(float(one["score"][0])) and model.batch_invariant is False


def test_single_waveform_helper_and_errors(aligned):
    model, wavs, seqs, res, _ = aligned
    r = 2
    d = model.align_phonemes_durations_long(wavs[r], seqs[r], model.vocab, **PLAN)
    one = model.force_align_long([wavs[r]], [seqs[r]], **PLAN)
    F, n = FRAMES[r], len(seqs[r])
    assert torch.equal(one["frame_token"][0, :F], res["frame_token"][r, :F])        # a recording alone is its row of the batch
    assert torch.equal(one["spans"][0, :n], res["spans"][r, :n]) and torch.equal(one["token_score"][0, :n], res["token_score"][r, :n])
    assert torch.equal(one["score"][0], res["score"][r])
    ratio = len(wavs[r]) / F / 16000
    sp = one["spans"][0, :n].cpu().numpy()
    assert list(d["phn_seq_idx"]) == seqs[r] and d["phn_seq_ipa"] == [f"p{i}" if i != 5 else "(...)" for i in seqs[r]]
    assert d["phn_start"] == [int(a) * ratio for a in sp[:, 0]] and d["phn_end"] == [int(a) * ratio for a in sp[:, 1]]
    assert d["phn_score"] == one["token_score"][0, :n].cpu().numpy().tolist() and d["score"] == float(one["score"][0])
    filled = hostlogic.fill_blank_frames(one["frame_token"][0, :F].cpu().numpy())
    assert d["phn_frames"] == [seqs[r][k] for k in filled] and len(d["phn_frames"]) == F
    with pytest.raises(ValueError, match="do not fit"):
        model.align_phonemes_durations_long(wavs[0], _distinct(np.random.RandomState(1), 30, 40), model.vocab, **PLAN)   # 30 phonemes, 24 frames
    with pytest.raises(ValueError, match="8191"):
        model.force_align_long(wavs[:1], [[1, 2] * 4096], **PLAN)
