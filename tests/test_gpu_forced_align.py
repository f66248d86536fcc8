"""Forced alignment on the MI355X (aptai_ctc_viterbi) against the host restatement of its contract, hostlogic.ctc_forced_align:
the PATH (frame_token, spans) must be torch.equal on every frame - both sides perform the same single fp32 additions and the same
tie rule -, the scores agree within bounds derived below from the fp32 operations the kernel performs, and the public surface
(Wav2Vec2_PR.force_align / align_phonemes_durations, Force_APTAI.alignment_readout) does what INTEGRATION.md says."""
import json
import math
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
TV = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")
EPS = 2.0 ** -23          # one fp32 ulp at 1 = TWICE the unit roundoff u of a correctly rounded operation (margin for <= 1 ulp expf / logf)


def _frame_bound(A, V):
    """Absolute error of one frame's log-probability d = x - lz as the kernel computes it, in units of u (here EPS = 2u, a factor 2
    of margin), A = max |logit|:  x_j - mx: u * 2A;  expf of it: relative 2A u (argument) + 2u (<= 1 ulp);  the sum of the V
    positive terms (<= 3 per-lane additions + 6 shuffle levels): + 10u relative  ->  relative error of se <= (2A + 12) u, which is
    the absolute error of log(se);  logf itself: 2u * ln V;  lz = mx + log se: u * (A + ln V);  d = x - lz: u * (2A + ln V).
    Sum: u * (5A + 4 ln V + 12)."""
    return EPS * (5.0 * A + 4.0 * math.log(max(V, 2)) + 12.0)


def _score_bound(A, V, Tb, score):
    """score = sum of Tb per-frame terms d_t <= 0 (so sum |d_t| = |score|): each thread of 256 adds ceil(Tb / 256) terms in order, then
    8 levels of a fixed tree -> summation error <= (ceil(Tb/256) + 8) u |score|, plus Tb per-frame errors (_frame_bound)."""
    return Tb * _frame_bound(A, V) + (math.ceil(Tb / 256) + 8) * EPS * abs(score)


def _token_bound(A, V, n, mean):
    """token_score = (sequential sum of n terms) / n: (n - 1) u |mean| from the additions, u |mean| from the division, plus the
    per-frame error of the terms themselves."""
    return _frame_bound(A, V) + (n + 1) * EPS * abs(mean)


def _run(x, targets, in_lens, V, *, blank=0, topology="ctc", vocab_sizes=None, T=None, col0=0, ldt=None):
    """x: float32 array [B][rows_per_b][ldl] (the kernel reads columns col0 .. col0 + V of the first T rows of each utterance).
    Returns the device outputs."""
    from aptai_amd import ops
    B, rows_per_b, ldl = x.shape
    assert B == len(targets) == len(in_lens)
    T = rows_per_b if T is None else T
    ldt = max([len(t) for t in targets] + [1]) if ldt is None else ldt
    tg = np.full((B, ldt), -100, dtype=np.int32)
    for b, t in enumerate(targets):
        tg[b, :len(t)] = t
    xd = torch.from_numpy(x).cuda().reshape(B * rows_per_b, ldl)
    tgd = torch.from_numpy(tg).cuda()
    lens = torch.tensor(in_lens, dtype=torch.int32).cuda()
    tl = torch.tensor([len(t) for t in targets], dtype=torch.int32).cuda()
    vs = None if vocab_sizes is None else torch.tensor(vocab_sizes, dtype=torch.int32).cuda()
    keep = (xd.clone(), tgd.clone())
    out = ops.ctc_viterbi(xd[:, col0:] if col0 else xd, ldl, rows_per_b, tgd, lens, tl, B, T, V, blank=blank, topology=topology,
                          vocab_sizes_i32=vs)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep[0]) and torch.equal(tgd, keep[1])                 # the call leaves its inputs untouched
    return out, ldt


def _check(x, targets, in_lens, V, *, blank=0, topology="ctc", vocab_sizes=None, T=None, col0=0, ldt=None):
    """Path exact, scores within the derived bounds, for every utterance.  Returns (device outputs, reference frame_token rows)."""
    from aptai_amd import hostlogic
    (ft, spans, score, tsc), ldt = _run(x, targets, in_lens, V, blank=blank, topology=topology, vocab_sizes=vocab_sizes, T=T, col0=col0,
                                        ldt=ldt)
    B = x.shape[0]
    T = x.shape[1] if T is None else T
    assert ft.shape == (B, T) and spans.shape == (B, ldt, 2) and score.shape == (B,) and tsc.shape == (B, ldt)
    ref_ft = np.empty((B, T), dtype=np.int32)
    ref_sp = np.empty((B, ldt, 2), dtype=np.int32)
    score_h, tsc_h = score.cpu().numpy(), tsc.cpu().numpy()
    worst = worst_tok = 0.0
    for b in range(B):
        Vb = V if vocab_sizes is None else vocab_sizes[b]
        xb = x[b, :T, col0:col0 + Vb]
        r_ft, r_score = hostlogic.ctc_forced_align(xb, in_lens[b], targets[b], blank=blank, topology=topology)
        ref_ft[b], ref_sp[b] = r_ft, hostlogic.alignment_spans(r_ft, ldt)
        Tb = max(0, min(int(in_lens[b]), T))
        if not np.isfinite(r_score):
            assert score_h[b] == -np.inf, (b, score_h[b])
            assert np.all(tsc_h[b] == -np.inf)
            continue
        A = float(np.abs(xb[:Tb]).max()) if Tb else 0.0
        bound = _score_bound(A, Vb, Tb, r_score)
        print(f"[forced align] b={b} score {float(score_h[b]):.6f} fp64 {r_score:.6f} bound {bound:.3e}")
        assert abs(float(score_h[b]) - r_score) <= bound, (b, float(score_h[b]), r_score, bound)
        worst = max(worst, abs(float(score_h[b]) - r_score) / max(bound, 1e-30))
        # token_score against the fp64 mean over the span
        x64 = xb[:Tb].astype(np.float64)
        mx = x64.max(axis=1) if Tb else np.zeros(0)
        lp = x64 - (mx + np.log(np.exp(x64 - mx[:, None]).sum(axis=1)))[:, None]
        for k in range(ldt):
            f0, f1 = ref_sp[b, k]
            if f0 < 0:
                assert tsc_h[b, k] == -np.inf
                continue
            mean = float(lp[f0:f1, targets[b][k]].mean())
            tb = _token_bound(A, Vb, f1 - f0, mean)
            assert abs(float(tsc_h[b, k]) - mean) <= tb, (b, k, float(tsc_h[b, k]), mean, tb)
            worst_tok = max(worst_tok, abs(float(tsc_h[b, k]) - mean) / tb)
    print(f"[forced align] worst |score - fp64| / bound = {worst:.3f}, worst |token_score - fp64| / bound = {worst_tok:.3f}")
    assert torch.equal(ft.cpu(), torch.from_numpy(ref_ft))                        # every frame of every utterance, no margin
    assert torch.equal(spans.cpu(), torch.from_numpy(ref_sp))
    return (ft, spans, score, tsc), ref_ft


def _transcripts(rng, B, lo, hi, V, first=1):
    return [[int(v) for v in rng.randint(first, V, size=int(rng.randint(lo, hi + 1)))] for _ in range(B)]


def test_exact_path_flagship_shape():
    rng = np.random.RandomState(11)
    B, T, V = 16, 499, 46
    x = (rng.randn(B, T, V) * 3).astype(np.float32)
    targets = _transcripts(rng, B, 1, 60, V)
    in_lens = [T] + [int(v) for v in rng.randint(150, T + 1, size=B - 1)]
    (ft, _, score, _), _ = _check(x, targets, in_lens, V)
    assert torch.isfinite(score).all()


@pytest.mark.parametrize("topology,Lmax,T", [("ctc", 20, 120), ("ctc", 100, 300), ("ctc", 255, 499), ("ctc", 255, 700),
                                             ("monotonic", 100, 260), ("monotonic", 255, 499), ("monotonic", 255, 1100)])
def test_exact_path_for_every_states_per_lane_instantiation(topology, Lmax, T):
    """Label rows of <= 63 / <= 127 / <= 255 slots (CTC) and <= 128 / <= 255 (monotonic) select 2 / 4 / 8 states per lane; the
    longest T of each topology does not fit the on-chip backpointer storage of its instantiation and takes the workspace route."""
    rng = np.random.RandomState(Lmax + T)
    B, V = 4, 46
    x = (rng.randn(B, T, V) * 2).astype(np.float32)
    first = 1 if topology == "ctc" else 0
    targets = [[int(v) for v in rng.randint(first, V, size=Lmax)]] + _transcripts(rng, B - 1, Lmax // 2, Lmax, V, first)
    in_lens = [T, T, T - 7, T - 31]
    (_, _, score, _), _ = _check(x, targets, in_lens, V, topology=topology)
    assert torch.isfinite(score).all()


def test_edge_lengths():
    rng = np.random.RandomState(3)
    T, V = 12, 5
    targets = [[], [2], [3], [1, 2], [], [4], [1, 2, 3]]
    in_lens = [10, 1, 7, 1, 0, 0, 12]
    x = rng.randn(len(targets), T, V).astype(np.float32)
    (ft, spans, score, _), _ = _check(x, targets, in_lens, V)
    s = score.cpu().numpy()
    assert np.isfinite(s[[0, 1, 2, 6]]).all() and s[3] == -np.inf and s[4] == 0.0 and s[5] == -np.inf
    assert ft[0, :10].eq(-1).all() and ft[0, 10:].eq(-2).all() and ft[1, 0] == 0 and ft[3].eq(-2).all()
    _check(x[:4], [[0], [], [1, 1], [2]], [3, 4, 2, 0], V, topology="monotonic")


def test_repeated_labels():
    rng = np.random.RandomState(4)
    T, V = 60, 6
    targets = [[3, 3, 3, 5, 5, 1], [2] * 20, [1, 1], [4, 4, 4]]
    x = (rng.randn(4, T, V) * 2).astype(np.float32)
    (ft, _, score, _), _ = _check(x, targets, [60, 45, 3, 4], V)
    assert ft[2, :3].tolist() == [0, -1, 1] and score[3] == -np.inf         # a a in three frames; a a a does not fit four
    _check(x, targets, [60, 45, 3, 4], V, topology="monotonic")


def test_infeasible_utterance_leaves_its_neighbours_alone():
    rng = np.random.RandomState(5)
    T, V = 200, 46
    x = (rng.randn(3, T, V) * 2).astype(np.float32)
    targets = _transcripts(rng, 3, 30, 30, V)
    (ft, spans, score, tsc), _ = _check(x, targets, [200, 20, 170], V)
    assert score[1] == -np.inf and ft[1].eq(-2).all() and spans[1].eq(-1).all()
    (ft2, spans2, score2, tsc2), _ = _check(np.ascontiguousarray(x[[0, 2]]), [targets[0], targets[2]], [200, 170], V)
    for a, b in ((ft, ft2), (spans, spans2), (score, score2), (tsc, tsc2)):
        assert torch.equal(a[[0, 2]], b)


def test_per_sample_vocabulary_sizes():
    rng = np.random.RandomState(6)
    B, T, V = 6, 150, 46
    x = (rng.randn(B, T, V) * 2).astype(np.float32)
    vs = [46, 10, 23, 30, 12, 46]
    targets = [[int(v) for v in rng.randint(1, vs[b], size=25)] for b in range(B)]
    targets[4][7] = 30                                                      # outside this utterance's 12 classes: no path
    (_, _, score, _), _ = _check(x, targets, [150, 140, 150, 99, 150, 80], V, vocab_sizes=vs)
    assert score[4] == -np.inf and torch.isfinite(score[[0, 1, 2, 3, 5]]).all()


def test_padded_pitches():
    rng = np.random.RandomState(7)
    B, T, V = 5, 99, 40
    x = (rng.randn(B, T + 13, 64) * 2).astype(np.float32)                   # rows_per_b > T, ldl > V; the padding holds large values
    x[:, T:] = 50.0
    x[:, :, V:] = 50.0
    _check(x, _transcripts(rng, B, 5, 30, V), [99, 98, 64, 65, 99], V, T=T)


def test_monotonic_on_offset_rows_of_pitch_64():
    """The layout of the forward-sum rows of Force_APTAI: [blank | N <= 63 log-attention columns | padding] in 64 floats, the pointer
    offset by one float, identity targets, vocab_sizes = N_b."""
    rng = np.random.RandomState(8)
    B, T = 6, 150
    Ns = [60, 1, 17, 59, 63, 40]
    x = np.zeros((B, T + 2, 64), dtype=np.float32)
    x[:, :, 0] = -1.0
    x[:, :, 1:] = np.log(rng.dirichlet(np.ones(63) * 0.3, size=(B, T + 2)) + 1e-30).astype(np.float32)
    targets = [list(range(n)) for n in Ns]
    (ft, _, score, _), ref = _check(x, targets, [150, 150, 149, 58, 150, 120], 63, topology="monotonic", vocab_sizes=Ns, T=T, col0=1, ldt=63)
    assert score[3] == -np.inf                                              # 59 phonemes, 58 frames
    for b in (0, 1, 2, 4, 5):
        path = ref[b][ref[b] >= 0]
        assert path[0] == 0 and path[-1] == Ns[b] - 1 and set(np.diff(path).tolist()) <= {0, 1}


def test_long_utterance_off_chip_beside_a_short_one_on_chip():
    rng = np.random.RandomState(9)
    V = 46
    x = (rng.randn(2, 1499, V) * 2).astype(np.float32)
    targets = _transcripts(rng, 2, 200, 200, V)
    _check(x, targets, [1499, 1301], V)                                     # 1499 frames x 401 states: backpointers in the workspace
    ts = [t[:60] for t in targets]
    _check(np.ascontiguousarray(x[:, :499]), ts, [499, 433], V)             # 499 frames x 121 states: backpointers in LDS
    # one and the same problem through both routes: 600 frames with a 255-slot label row (8 states per lane, 512 frames fit on chip:
    # workspace) and with a 60-slot label row (2 states per lane, 1024 frames fit: LDS) -> identical results
    x6 = np.ascontiguousarray(x[:1, :600])
    (a, sa, ca, ta), _ = _check(x6, [ts[0]], [600], V, ldt=255)
    (b, sb, cb, tb), _ = _check(x6, [ts[0]], [600], V, ldt=60)
    assert torch.equal(a, b) and torch.equal(sa[:, :60], sb) and torch.equal(ca, cb) and torch.equal(ta[:, :60], tb)


def test_same_inputs_same_bits():
    rng = np.random.RandomState(10)
    B, T, V = 16, 499, 46
    x = (rng.randn(B, T, V) * 3).astype(np.float32)
    targets = _transcripts(rng, B, 1, 60, V)
    in_lens = [int(v) for v in rng.randint(100, T + 1, size=B)]
    one, _ = _run(x, targets, in_lens, V)
    two, _ = _run(x, targets, in_lens, V)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    x2 = np.ascontiguousarray(np.tile(x[:2], (1, 3, 1))[:, :1400])           # the workspace route
    t2 = [t * 4 for t in targets[:2]]
    one, _ = _run(x2, t2, [1400, 1222], V)
    two, _ = _run(x2, t2, [1400, 1222], V)
    for a, b in zip(one, two):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- Wav2Vec2_PR
def _build_pr(cfg, sd, vocab_n=40):
    from aptai_amd.w2v2_pr import Wav2Vec2_PR
    from safetensors.torch import save_file
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "config.json"), "w") as f:
            json.dump(cfg.to_dict(), f)
        save_file({k[len("wav2vec2."):]: v.contiguous() for k, v in sd.items() if k.startswith("wav2vec2.")},
                  os.path.join(tmp, "model.safetensors"))
        model = Wav2Vec2_PR(cfg, None, tmp, {f"p{i}": i for i in range(vocab_n)})
    model.load_state_dict(sd)
    return model.cuda()


def _pr_model():
    from aptai_amd.config import W2V2Config
    from oracle import synth
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0.,
                          final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=40)
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 3)
    return _build_pr(cfg, sd), cfg


def test_force_align_of_the_models_own_best_path_is_the_frame_argmax():
    """Two utterances of different length, each aligned to its own best-path decode: the best path through the lattice of that
    transcript is the unconstrained best path, i.e. the frame argmax, on every valid frame."""
    from aptai_amd import hostlogic
    model, cfg = _pr_model()
    g = torch.Generator().manual_seed(21)
    wavs = [torch.randn(16000, generator=g).numpy(), torch.randn(11111, generator=g).numpy()]
    for wav in wavs:
        logits = model.get_ctc_logits(wav)                                  # (T, V) of this utterance alone
        ids = hostlogic.ctc_best_path(logits, logits.shape[0], 0)
        assert 1 <= len(ids) <= 255
        res = model.force_align(torch.from_numpy(wav)[None].cuda(), torch.tensor([len(wav)]).cuda(),
                                torch.from_numpy(ids[None].astype(np.int32)))
        assert all(v.is_cuda for v in res.values())
        n = int(res["frame_seq_lens"][0])
        assert n == logits.shape[0] and np.isfinite(float(res["score"][0]))
        np.testing.assert_array_equal(res["frame_phns"][0, :n].cpu().numpy(), logits.argmax(axis=-1))


def test_force_align_batch_of_two_lengths_and_durations():
    from aptai_amd import hostlogic
    model, cfg = _pr_model()
    g = torch.Generator().manual_seed(22)
    lens = [16000, 12345]
    audio = torch.randn(2, 16000, generator=g)
    audio[1, lens[1]:] = 0
    rng = np.random.RandomState(2)
    seqs = [[int(v) for v in rng.randint(1, 40, size=17)], [int(v) for v in rng.randint(1, 40, size=9)]]
    labels = torch.full((2, 17), -100, dtype=torch.int32)
    for b, q in enumerate(seqs):
        labels[b, :len(q)] = torch.tensor(q, dtype=torch.int32)
    res = model.force_align(audio.cuda(), torch.tensor(lens).cuda(), labels)
    fl = res["frame_seq_lens"].cpu().tolist()
    want_fl = [int(hostlogic.feat_extract_output_lengths(n, cfg.conv_kernel, cfg.conv_stride)) for n in lens]
    assert fl == want_fl and fl[1] < fl[0] == res["frame_token"].shape[1]
    for b, q in enumerate(seqs):
        assert np.isfinite(float(res["score"][b]))
        fp = res["frame_phns"][b].cpu().numpy()
        ft = res["frame_token"][b].cpu().numpy()
        assert (ft[fl[b]:] == -2).all() and (fp[fl[b]:] == 0).all() and (ft[:fl[b]] >= -1).all()       # padding beyond the length
        valid, tok = fp[:fl[b]], ft[:fl[b]]
        col = [int(p) for i, p in enumerate(valid) if tok[i] >= 0 and (i == 0 or tok[i] != tok[i - 1])]
        assert col == q                                                                                # collapses to the transcript
        assert (valid[tok == -1] == 0).all()
        sp = res["spans"][b, :len(q)].cpu().numpy()
        assert (sp[:, 0] < sp[:, 1]).all() and (sp[1:, 0] >= sp[:-1, 1]).all() and sp[0, 0] >= 0 and sp[-1, 1] <= fl[b]   # ordered, disjoint
        assert res["spans"][b, len(q):].eq(-1).all()
        assert torch.isfinite(res["token_score"][b, :len(q)]).all() and (res["token_score"][b, :len(q)] <= 0).all()
    # the single-waveform helper agrees with force_align on the same waveform
    wav = audio[0].numpy()
    vocab = model.vocab
    one = model.force_align(audio[:1].cuda(), torch.tensor(lens[:1]).cuda(), labels[:1])
    d = model.align_phonemes_durations(wav, seqs[0], vocab)
    ratio = len(wav) / one["frame_token"].shape[1] / 16000
    sp = one["spans"][0, :len(seqs[0])].cpu().numpy()
    assert list(d["phn_seq_idx"]) == seqs[0] and d["phn_seq_ipa"] == [f"p{i}" for i in seqs[0]]
    assert d["phn_start"] == [int(a) * ratio for a in sp[:, 0]] and d["phn_end"] == [int(a) * ratio for a in sp[:, 1]]
    assert d["phn_score"] == one["token_score"][0, :len(seqs[0])].cpu().numpy().tolist()
    filled = hostlogic.fill_blank_frames(one["frame_token"][0].cpu().numpy())
    assert d["phn_frames"] == [seqs[0][k] for k in filled] and len(d["phn_frames"]) == fl[0]
    with pytest.raises(ValueError):
        model.align_phonemes_durations(wav[:4000], list(range(1, 30)), vocab)                           # 29 phonemes, 12 frames
    # the existing read-out keeps its result
    p = model.predict_phonemes_durations(wav, vocab)
    idx, ts = hostlogic.ctc_bracketed_best_path(model.get_ctc_logits(wav), fl[0], 0, None)
    assert list(p["phn_seq_idx"]) == list(idx) and p["phn_seq_dur"] == [t * ratio for t in ts]


# ----------------------------------------------------------------------------------------------- Force_APTAI
def _pr_ckpt(tmp, pr_cfg, sd, vocab):
    from safetensors.torch import save_file
    mdir = os.path.join(tmp, "w2v2")
    os.makedirs(mdir)
    with open(os.path.join(mdir, "config.json"), "w") as f:
        json.dump(pr_cfg.to_dict(), f)
    save_file({k[len("w2v2_pr.wav2vec2."):]: v.contiguous() for k, v in sd.items() if k.startswith("w2v2_pr.wav2vec2.")},
              os.path.join(mdir, "model.safetensors"))
    ck = os.path.join(tmp, "pr", "best-model-ckpt")
    os.makedirs(ck)
    torch.save({k[len("w2v2_pr."):]: v for k, v in sd.items() if k.startswith("w2v2_pr.")}, os.path.join(ck, "pytorch_model.bin"))
    with open(os.path.join(ck, "model_cfg.pkl"), "wb") as f:
        pickle.dump({"pretrain_cfg": pr_cfg.to_dict(), "cache_dir": None, "huggingface_model_id": mdir}, f)
    return os.path.join(tmp, "pr")


def _force_model():
    from aptai_amd.config import W2V2Config
    from aptai_amd.force_aptai import Force_APTAI
    from oracle import synth
    z, meta = load_golden("force_aptai_1x2s")
    pr_cfg = W2V2Config.from_any(meta["pr_cfg"])
    sd = synth.make_state_dict(synth.force_aptai_param_shapes(pr_cfg, meta["vocab_len"]), meta["seed"])
    sd["w2v2_pr.pr_head.bias"][0] += meta["blank_bias"]
    vocab = {"(blank)": 0, "(...)": 1}
    vocab.update({f"p{i}": i for i in range(2, 40)})
    with tempfile.TemporaryDirectory() as tmp:
        model = Force_APTAI(_pr_ckpt(tmp, pr_cfg, sd, vocab), "cuda", vocab)
    model.load_state_dict(sd)
    return model.cuda(), pr_cfg


def _force_batch(pr_cfg, B=2):
    from oracle import synth
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(pr_cfg, B, 24000, seed=5, n_phn=40).items()}
    batch["phoneme_labels"] = torch.zeros(B, 4, dtype=torch.int32).cuda()
    return batch


def test_force_aptai_default_readout_is_what_it_was():
    """alignment_readout = "argmax" (the default) against a model object whose head state never carries the new fields: same seed,
    same batch, training mode with its dropouts -> losses, tvs_pred, the lists and the gradients are equal bit for bit."""
    from aptai_amd.force_aptai import Force_APTAI
    assert Force_APTAI.alignment_readout == "argmax"
    model, pr_cfg = _force_model()
    plain, _ = _force_model()
    inner = plain._heads_state

    def heads_state(*a, **k):
        st, P = inner(*a, **k)
        del st.readout, st.mono_targets
        return st, P
    plain._heads_state = heads_state
    batch = _force_batch(pr_cfg)
    outs = []
    for m in (model, plain):
        m.train()
        out = m(0, **batch)
        out["loss"].backward()
        outs.append(out)
    torch.cuda.synchronize()
    a, b = outs
    for k in ("loss", "tv_loss", "align_loss", "tvs_pred"):
        assert torch.equal(a[k], b[k]), k
    assert a["pred_frame_phns"] == b["pred_frame_phns"]
    assert [list(map(int, q)) for q in a["pred_ctc_phn_seq"]] == [list(map(int, q)) for q in b["pred_ctc_phn_seq"]]
    for (n, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), n


def test_force_aptai_monotonic_readout():
    from aptai_amd import hostlogic
    model, pr_cfg = _force_model()
    batch = _force_batch(pr_cfg)
    model.eval()
    with torch.no_grad():
        base = model(0, **batch)
        model.alignment_readout = "monotonic"
        mono = model(0, **batch)
    for k in ("loss", "tv_loss", "align_loss", "tvs_pred"):
        assert torch.equal(base[k], mono[k]), k                                # the read-out feeds nothing but the lists
    assert [list(map(int, q)) for q in base["pred_ctc_phn_seq"]] == [list(map(int, q)) for q in mono["pred_ctc_phn_seq"]]
    # per utterance, alone (get_alignment runs a batch of one): exactly the host Viterbi of the same log-attention rows
    for b in range(2):
        n = int(batch["audio_lengths"][b])
        wav = batch["audio_inputs"][b, :n].cpu().numpy()
        n_frames = int(hostlogic.feat_extract_output_lengths(n, pr_cfg.conv_kernel, pr_cfg.conv_stride))
        one = {}
        for k, v in batch.items():
            one[k] = v[b:b + 1, :n] if k == "audio_inputs" else v[b:b + 1, :n_frames] if (k in TV or k == "phn_frames_49hz") else v[b:b + 1]
        with torch.no_grad():
            out = model(0, **one)
        att = model.get_alignment(wav)["alignment"]                            # (N, T) log-attention
        ids = [int(v) for v in out["pred_ctc_phn_seq"][0]]
        N, T = att.shape
        assert N == len(ids) and 1 <= N <= T == n_frames
        ft, score = hostlogic.ctc_forced_align(np.ascontiguousarray(att.T), T, list(range(N)), topology="monotonic")
        assert np.isfinite(score)
        assert out["pred_frame_phns"][0] == [ids[k] for k in ft]
        assert ft[0] == 0 and ft[-1] == N - 1 and set(np.diff(ft).tolist()) <= {0, 1}   # non-decreasing, steps of at most one, 0 .. N-1
        single = model.get_faptai_output(wav)
        assert single["pred_frame_phns"] == out["pred_frame_phns"][0]
    model.alignment_readout = "viterbi"
    with pytest.raises(ValueError):
        model(0, **batch)
    model.alignment_readout = "argmax"
    with torch.no_grad():
        again = model(0, **batch)
    assert again["pred_frame_phns"] == base["pred_frame_phns"]
